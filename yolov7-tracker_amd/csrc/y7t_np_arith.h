// y7t_np_arith.h -- the arithmetic of the appearance trackers' costs and stores, restated as numpy 2.2 / OpenBLAS 0.3.29 (AVX-512 kernels) / scipy 1.15 evaluate
// it in the environment the golden sequences were recorded in.  The costs of similar objects differ by a few ulps and the assignment follows them, so each sum
// is pinned operand by operand and the goldens compare bit for bit: tests/golden/np_norms.npz holds numpy's own bits of both float32 norms at 18 widths
// (tests/test_deepsort_feat_cpu.py), tests/test_strongsort_cpu.py and tests/test_botsort_reid_cpu.py compare the float64 forms with numpy / scipy.
// Every function is named for what it restates, not for the tracker that uses it (y7t_track_*.h).  Portable text (device: hipcc; CPU tests: -DY7T_HOSTSIM).
#pragma once
#include "y7t_track_core.h"

// contraction off in the text itself, so no compiler flag decides the rounding of a product that feeds a sum
#if Y7T_DEVICE
#define Y7T_NO_CONTRACT _Pragma("clang fp contract(off)")      // (hipcc contracts a * b + c by default; the library's build switches that off for y7t_tracker.hip as well)
#else
#define Y7T_NO_CONTRACT                                        // (the CPU build is compiled with -ffp-contract=off)
#endif

// numpy's pairwise reduction, float32: np.linalg.norm(mat, axis=1) -- x * x rounded to float32, then add.reduce's PAIRWISE sum
// (numpy/_core/src/umath/loops_utils.h.src: 8 running sums for blocks <= 128, recursive halving above), sqrt (the caller's).
Y7T_NOINL float y7t_np_pairwise_sumsq(const float* x, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r = r + x[i] * x[i];
        return r;
    }
    if (n <= 128) {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = x[j] * x[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] = r[j] + x[i + j] * x[i + j];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res = res + x[i] * x[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return y7t_np_pairwise_sumsq(x, n2) + y7t_np_pairwise_sumsq(x + n2, n - n2);
}

#if Y7T_DEVICE
// The wave forms share one vector among the 64 lanes of a wave (every lane calls; every lane gets the result) -- bit-identical to the serial forms: each partial
// sum is built from the same operands in the same order, only by different lanes.  The float32 ones take these widths.
Y7T_FN bool y7t_dim_wave_ok(int dim) { return dim == 128 || dim == 256 || dim == 512 || dim == 1024; }
// y7t_np_pairwise_sumsq of the vector x[i] / div (div = 1: x itself) by one wave: lane (block, j) owns running sum j of its 128-element block
Y7T_FN float y7t_np_wave_pairwise_sumsq(const float* x, int dim, float div, int lane) {
    const int nblk = dim >> 7, blk = lane >> 3, j = lane & 7;
    float r = 0.f;
    if (blk < nblk) {
        const float* xb = x + blk * 128;
        const float t0 = xb[j] / div;
        r = t0 * t0;
        for (int i = 8; i < 128; i += 8) { const float t = xb[i + j] / div; r = r + t * t; }
    }
    r = r + __shfl_xor(r, 1, 64); r = r + __shfl_xor(r, 2, 64); r = r + __shfl_xor(r, 4, 64);      // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))
    for (int m = 1; m < nblk; m <<= 1) r = r + __shfl_xor(r, 8 * m, 64);                          // the recursive halving over blocks
    return __shfl(r, 0, 64);
}
#endif

// numpy's pairwise reduction, float64: mat / np.linalg.norm(mat, axis=1, keepdims=True) of float32 rows cast to float64 (cal_cosine_distance) --
// sqrt(np.add.reduce(x * x, axis=1)): the products are exact (float32 values), the reduction is the same PAIRWISE sum: blocks of at most 128 elements, eight
// interleaved accumulators a block combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the block's tail added one by one, a longer run halved (the left half rounded
// down to a multiple of 8) and the halves' sums added; then one division per element.
template <class LeafFn>
Y7T_FN double y7t_np_pairwise_f64(int n, LeafFn leaf /* (offset, count <= 128) -> that block's sum */) {
    int so[20], sn[20], sd[20], sp = 1, vd[20], vp = 0;
    double vv[20];
    so[0] = 0; sn[0] = n; sd[0] = 0;
    while (sp > 0) {      // depth-first, left to right; two finished neighbours of one depth are their parent's halves
        --sp;
        const int o = so[sp], m = sn[sp], d = sd[sp];
        if (m > 128) {
            int n2 = m / 2;
            n2 -= n2 % 8;
            so[sp] = o + n2; sn[sp] = m - n2; sd[sp] = d + 1; ++sp;
            so[sp] = o; sn[sp] = n2; sd[sp] = d + 1; ++sp;
            continue;
        }
        double v = leaf(o, m);
        int dd = d;
        while (vp > 0 && vd[vp - 1] == dd) { v = vv[vp - 1] + v; --vp; --dd; }
        vv[vp] = v; vd[vp] = dd; ++vp;
    }
    return vv[0];
}
Y7T_FN double y7t_np_sq_f64(float x) { return (double)x * (double)x; }      // (exact: 24-bit factors)
Y7T_FN double y7t_np_pairwise_leaf_f64(const float* x, int o, int m) {
    double res = 0.0;
    int i = 0;
    if (m >= 8) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = y7t_np_sq_f64(x[o + k]);
        for (i = 8; i < m - (m % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] = r[k] + y7t_np_sq_f64(x[o + i + k]);
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    }
    for (; i < m; ++i) res = res + y7t_np_sq_f64(x[o + i]);
    return res;
}
Y7T_FN double y7t_np_norm_f64(const float* x, int dim) { return sqrt(y7t_np_pairwise_f64(dim, [&](int o, int m) { return y7t_np_pairwise_leaf_f64(x, o, m); })); }
Y7T_FN bool y7t_np_norm_ok(double nrm) { return nrm > 0.0 && nrm < HUGE_VAL; }      // (false for NaN: an element that is not finite makes the sum so)
// out[k] = x[k] / |x| -> is the row usable (a zero or non-finite norm gives the reference NaN costs, which it hands to lapjv)
Y7T_FN bool y7t_np_normalize_f64(const float* x, int dim, double* out) {
    const double nrm = y7t_np_norm_f64(x, dim);
    for (int k = 0; k < dim; ++k) out[k] = (double)x[k] / nrm;
    return y7t_np_norm_ok(nrm);
}
#if Y7T_DEVICE
// the same by one wave: lanes 0..7 own a block's eight accumulators, every lane leaves with the block's sum; the divisions a lane per element
Y7T_FN bool y7t_np_wave_normalize_f64(const float* x, int dim, double* out, int lane) {
    const double sum = y7t_np_pairwise_f64(dim, [&](int o, int m) {
        double res = 0.0;
        int i = 0;
        if (m >= 8) {
            const int k = lane & 7;
            double r = y7t_np_sq_f64(x[o + k]);
            for (i = 8; i < m - (m % 8); i += 8) r = r + y7t_np_sq_f64(x[o + i + k]);
            const double r0 = __shfl(r, 0, 64), r1 = __shfl(r, 1, 64), r2 = __shfl(r, 2, 64), r3 = __shfl(r, 3, 64);
            const double r4 = __shfl(r, 4, 64), r5 = __shfl(r, 5, 64), r6 = __shfl(r, 6, 64), r7 = __shfl(r, 7, 64);
            res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        }
        for (; i < m; ++i) res = res + y7t_np_sq_f64(x[o + i]);
        return res;
    });
    const double nrm = sqrt(sum);
    for (int k = lane; k < dim; k += 64) out[k] = (double)x[k] / nrm;
    return y7t_np_norm_ok(nrm);
}
#endif

// OpenBLAS's sdot: np.linalg.norm(vec) of a 1-D float32 feature (STrack.update, basetrack.py:325) = sqrt(sdot(x, x)).  The SkylakeX sdot kernel over the
// first n & -32 elements -- four 16-lane accumulators over 64 elements per step (FMA), folded 16 -> 8 lanes, summed ((a0 + a1) + a2) + a3, halves added, two
// horizontal adds -- and its driver (kernel/x86_64/sdot.c) for the n & 31 that remain: their float32 products summed into a DOUBLE, the kernel's float32 sum
// added in double, one rounding to float32.  One restatement for every tracker: a tail summed in float32 is one ulp off at widths such as 100.
Y7T_FN float y7t_fmaf(float a, float b, float c) {
#if Y7T_DEVICE
    return __builtin_fmaf(a, b, c);
#else
    return fmaf(a, b, c);
#endif
}

// the driver's tail: `kern` is the kernel's sum of the first n1 = n & -32 elements
Y7T_FN float y7t_blas_sdot_tail(const float* x, int n1, int n, float kern) {
    if (n1 == n) return kern;
    double tail = 0.0;
    for (int k = n1; k < n; ++k) { const float p = x[k] * x[k]; tail = tail + (double)p; }
    return (float)(tail + (double)kern);
}

Y7T_FN float y7t_blas_sdot_self(const float* x, int n) {
    const int n1 = n & -32, n64 = n1 & ~63;
    float a5[4][16], a[4][8];
    for (int v = 0; v < 4; ++v) for (int l = 0; l < 16; ++l) a5[v][l] = 0.f;
    int i = 0;
    for (; i < n64; i += 64)
        for (int v = 0; v < 4; ++v) for (int l = 0; l < 16; ++l) { const float t = x[i + 16 * v + l]; a5[v][l] = y7t_fmaf(t, t, a5[v][l]); }
    for (int v = 0; v < 4; ++v) for (int l = 0; l < 8; ++l) a[v][l] = a5[v][l] + a5[v][l + 8];
    for (; i < n1; i += 32)
        for (int v = 0; v < 4; ++v) for (int l = 0; l < 8; ++l) { const float t = x[i + 8 * v + l]; a[v][l] = y7t_fmaf(t, t, a[v][l]); }
    float sv[8], hv[4];
    for (int l = 0; l < 8; ++l) sv[l] = ((a[0][l] + a[1][l]) + a[2][l]) + a[3][l];
    for (int l = 0; l < 4; ++l) hv[l] = sv[l] + sv[l + 4];
    const float d = (hv[0] + hv[1]) + (hv[2] + hv[3]);
    return y7t_blas_sdot_tail(x, n1, n, d);
}

#if Y7T_DEVICE
// The kernel by one wave: lane 16 v + l owns accumulator (v, l) of the 64-element steps -- its own sum a5 of elements lane, lane + 64, ... in order.
// the 16 -> 8 lane halving behind the 64-element steps (meaningful on l < 8) ...
Y7T_FN float y7t_blas_wave_sdot_halve(float a5, int lane) { return a5 + __shfl(a5, (lane + 8) & 63, 64); }
// ... and the fold of the halved accumulators a (lane 16 v + l, l < 8: accumulator (v, l))
Y7T_FN float y7t_blas_wave_sdot_fold(float a, int lane) {
    const int l = lane & 15;
    const float a0 = __shfl(a, l & 7, 64), a1 = __shfl(a, 16 + (l & 7), 64), a2 = __shfl(a, 32 + (l & 7), 64), a3 = __shfl(a, 48 + (l & 7), 64);
    const float sv = ((a0 + a1) + a2) + a3;                                                     // sv[l & 7] on every lane
    const float hv = sv + __shfl(sv, (lane & 48) + (((l & 7) + 4) & 7), 64);                    // l & 7 < 4: sv[l] + sv[l + 4]
    const float h0 = __shfl(hv, 0, 64), h1 = __shfl(hv, 1, 64), h2 = __shfl(hv, 2, 64), h3 = __shfl(hv, 3, 64);
    return (h0 + h1) + (h2 + h3);
}

// y7t_blas_sdot_self by one wave
Y7T_FN float y7t_blas_wave_sdot_self(const float* x, int n, int lane) {
    const int n1 = n & -32, n64 = n1 & ~63;
    const int v = lane >> 4, l = lane & 15;
    float a5 = 0.f;
    for (int i = 0; i < n64; i += 64) { const float t = x[i + lane]; a5 = y7t_fmaf(t, t, a5); }
    float a = y7t_blas_wave_sdot_halve(a5, lane);
    if (n1 > n64 && l < 8) { const float t = x[n64 + 8 * v + l]; a = y7t_fmaf(t, t, a); }      // the kernel's last, 32-element step
    const float d = y7t_blas_wave_sdot_fold(a, lane);
    return y7t_blas_sdot_tail(x, n1, n, d);      // (no wave width has a tail; every lane would walk it alike)
}
#endif

// One-chain FMA dot products: np.dot(mat1, mat2.T) per output element.  float32 (sgemm): one sequential fused-multiply-add chain over k -- y7t_fmaf above,
// written out where the products are taken (y7t_embed_slot, k_embed_dist).  float64 (dgemm): what OpenBLAS's dgemm does depends on the shapes (its small-matrix
// kernels, gemv for a single row or column, 256-deep k blocks for large ones), so no one chain is numpy's; ONE sequential FMA chain over k = 0 .. dim-1 per pair
// meets np.dot to a few units of the last place of 1 (DESIGN.md section 4 records the largest difference measured, and the goldens keep both thresholds that far
// from every pair).  The contraction is stated (fma), whatever the build's -ffp-contract says.
Y7T_FN double y7t_np_dotstep_f64(double s, double a, double b) { return __builtin_fma(a, b, s); }
Y7T_FN double y7t_np_dot_f64(const double* a, const double* b, int dim) {
    double s = 0.0;
    int k = 0;
#if Y7T_DEVICE
    if ((dim & 1) == 0 && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0) {      // 16-byte loads, a 128-byte line of each row at a time: the same chain
        for (; k + 16 <= dim; k += 16) {
            double2 av[8], bv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { av[q] = *(const double2*)(a + k + 2 * q); bv[q] = *(const double2*)(b + k + 2 * q); }
#pragma unroll
            for (int q = 0; q < 8; ++q) { s = y7t_np_dotstep_f64(s, av[q].x, bv[q].x); s = y7t_np_dotstep_f64(s, av[q].y, bv[q].y); }
        }
    }
#endif
    for (; k < dim; ++k) s = y7t_np_dotstep_f64(s, a[k], b[k]);
    return s;
}

// scipy's cdist, metric 'euclidean' (matching.embedding_distance), float64 as scipy 1.15 evaluates it: per pair ONE sequential chain over k = 0 .. dim-1 of
// d = u[k] - v[k]; s += d * d (the product rounded before the sum: no FMA), then sqrt, then np.maximum(0.0, .).  Both operands are float32 values cast to
// float64 (the casts are exact).
Y7T_FN double y7t_scipy_sqstep(double s, float u, float v) {
    Y7T_NO_CONTRACT
    const double d = (double)u - (double)v;
    const double p = d * d;
    return s + p;
}
Y7T_FN double y7t_scipy_root(double s) {
    const double d = sqrt(s);      // (correctly rounded on the device as on the host)
    return d > 0.0 ? d : (d != d ? d : 0.0);      // np.maximum(0.0, d): NaN passes
}
Y7T_FN double y7t_scipy_euclidean(const float* u, const float* v, int dim) {
    double s = 0.0;
    for (int k = 0; k < dim; ++k) s = y7t_scipy_sqstep(s, u[k], v[k]);
    return y7t_scipy_root(s);
}

// The float32 moving average of STrack.update (basetrack.py:324-332, use_avg_of_feature = True): smooth = 0.9 * features[-1] + (1 - 0.9) * f -- the scalars
// round to float32(0.9) / float32(0.1), the products and the sum are three separate roundings.
Y7T_FN float y7t_np_mix_f32(float prev, float f) {
    Y7T_NO_CONTRACT
    const float a = 0.9f * prev, b = 0.1f * f;
    return a + b;
}
