// y7t_gsi.h -- GSI, the Gaussian-smoothed interpolation of StrongSORT++ (the reference ships no GSI code: `use_GSI` is never read in tracker/strongsort.py; the
// procedure is this project's restatement of the StrongSORT release's GSI.py, DESIGN.md section 4 "GSI", and tests/gsi_np.py is its NumPy statement).  This file
// states the interpolation arithmetic and the per-track smoother ONCE, for the device kernels (csrc/y7t_gsi.hip) and for the CPU build of the same bodies
// (tests/_hostsim/gsi.py): a workgroup program over an execution context (thread of nt, wave of nw, lane of nl) whose strided loops run at nt = nw = nl = 1 on the host.  The only
// difference between the two builds is y7t_gsi_tile: v_mfma_f64_16x16x4_f64 on the device, the same sixteen products summed in the same k order on the host.
//
// Interpolation is ONE correctly rounded float64 operation at a time (subtract, divide, multiply, add; contraction off), so device, host build and NumPy agree bit
// for bit.  The smoother is float64 throughout with one fixed summation order, so a track's result is the same bits from call to call and whatever its slot.
// Portable text: the host build needs no HIP header.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define Y7T_GSI_FN __device__ __forceinline__
#define Y7T_GSI_HD __host__ __device__ inline
#define Y7T_GSI_DEVICE 1
#else
#define Y7T_GSI_FN static inline
#define Y7T_GSI_HD static inline
#define Y7T_GSI_DEVICE 0
#endif
#if defined(__clang__)
#define Y7T_GSI_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define Y7T_GSI_NO_CONTRACT
#endif

enum {
    Y7T_GSI_COLS = 5,                  // a run's row: [frame, x, y, w, h]
    Y7T_GSI_PANEL = 16,                // panel width of the blocked Cholesky = the tile of v_mfma_f64_16x16x4_f64
    Y7T_GSI_LDS_LEN = 128,             // tracks of up to this many rows keep their triangle in the LDS, longer ones in the object's pool
    Y7T_GSI_LDS_PAD = 2,               // doubles added to an LDS row, so that the sixteen rows of a tile do not share a bank
    Y7T_GSI_MAX_LEN = 4096,            // the longest track an object can be sized for (its frames stay in the LDS: 32 KiB)
    Y7T_GSI_MAX_TRACKS = 32768,
    Y7T_GSI_CLASSES = 6,               // padded-length classes: <= 128 (LDS), 256, 512, 1024, 2048, 4096
    // status word of y7t_gsi_interpolate
    Y7T_GSI_ROWS_OVERFLOW = 1,         // more rows after interpolation than max_rows: the output is not whole
    Y7T_GSI_LEN_OVERFLOW = 2,          // a track is longer than max_len after interpolation
    // status word per track of y7t_gsi_smooth
    Y7T_GSI_NOT_PD = 1,                // a non-positive pivot: the track's columns are left as they came
    Y7T_GSI_TOO_LONG = 2,              // the track is longer than the call's `longest`: left as it came
    Y7T_GSI_PENDING = 4,               // no launch reached the track (the table holds more rows than the object was sized for): left as it came
};

// rows a gap (f0, f1) of one track receives: every frame in between when f0 + 1 < f1 < f0 + interval
Y7T_GSI_HD int y7t_gsi_fill(double f0, double f1, int interval) {
    const long long a = (long long)f0, b = (long long)f1;
    return (a + 1 < b && b < a + interval) ? (int)(b - a - 1) : 0;
}

// v0 + (v1 - v0) / (f1 - f0) * i, in exactly that order
Y7T_GSI_HD double y7t_gsi_lerp(double v0, double v1, double span, double i) {
    Y7T_GSI_NO_CONTRACT
    const double d = v1 - v0;
    const double q = d / span;
    const double m = q * i;
    return v0 + m;
}

// K[i][j] = exp(-0.5 * ((t_i - t_j) / len_scale)**2)
Y7T_GSI_HD double y7t_gsi_kernel(double ti, double tj, double ls) {
    Y7T_GSI_NO_CONTRACT
    const double d = ti - tj;
    const double q = d / ls;
    const double s = q * q;
    const double e = -0.5 * s;
    return exp(e);
}

Y7T_GSI_HD int y7t_gsi_pad(int n) { return (n + Y7T_GSI_PANEL - 1) / Y7T_GSI_PANEL * Y7T_GSI_PANEL; }
// padded-length class of a track of n >= 1 rows: 0 = LDS, c >= 1 = a pool slot of 128 << c rows
Y7T_GSI_HD int y7t_gsi_class(int n) {
    int c = 0;
    while ((Y7T_GSI_LDS_LEN << c) < n) ++c;
    return c;
}

struct Y7TGsiExec { int tid, nt, wave, nw, lane, nl; };      // thread of nt, wave of nw, lane of nl

Y7T_GSI_FN void y7t_gsi_sync() {
#if Y7T_GSI_DEVICE
    __syncthreads();
#endif
}

// one 16 x 16 tile of the trailing update: A[r0.., c0..] -= L[r0.., k0..k0+15] L[c0.., k0..k0+15]^T, by one wave, four matrix instructions of K = 4
#if Y7T_GSI_DEVICE
typedef double y7t_f64x4 __attribute__((ext_vector_type(4)));
// operands: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one double each; C / D: column = l & 15, row = (l >> 4) + 4 reg
Y7T_GSI_FN void y7t_gsi_tile(double* A, size_t ld, int r0, int c0, int k0, int lane) {
    const int q = lane & 15, h = lane >> 4;
    y7t_f64x4 acc;
    double* c = A + (size_t)(r0 + h) * ld + c0 + q;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = c[(size_t)4 * r * ld];
    const double* a = A + (size_t)(r0 + q) * ld + k0 + h;
    const double* b = A + (size_t)(c0 + q) * ld + k0 + h;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[4 * kk], b[4 * kk], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) c[(size_t)4 * r * ld] = acc[r];
}
#else
static inline void y7t_gsi_tile(double* A, size_t ld, int r0, int c0, int k0, int) {
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            double s = A[(size_t)(r0 + i) * ld + c0 + j];
            for (int k = 0; k < 16; ++k) s = fma(-A[(size_t)(r0 + i) * ld + k0 + k], A[(size_t)(c0 + j) * ld + k0 + k], s);
            A[(size_t)(r0 + i) * ld + c0 + j] = s;
        }
}
#endif

// The smoother of ONE track, by one workgroup.  run: n x 5 [frame, x, y, w, h]; A: np x ld doubles (np = n padded to 16 with identity rows), Y: np x 4, t: np,
// D: 16 x 16 + 16 doubles; out: n x 4.  Returns 0 or Y7T_GSI_NOT_PD, the same value in every thread; every barrier is reached by the whole workgroup.
//   1. A = K + reg I, lower triangle (whole diagonal blocks, so that a tile never reads what nobody wrote)
//   2. A = L L^T, right-looking in panels of 16: the diagonal block in D (column by column), the panel below it (a thread per row), the trailing update in tiles
//   3. L z = Y, L^T a = z in panels of 16
//   4. out = K a, K recomputed, j ascending
Y7T_GSI_FN int y7t_gsi_track(const Y7TGsiExec& ex, double* A, size_t ld, double* Y, double* t, double* D, const double* run, int n, double ls, double reg,
                             double* out) {
    Y7T_GSI_NO_CONTRACT
    const int np = y7t_gsi_pad(n), nb = np / Y7T_GSI_PANEL;
    double* Ld = D + 256;
    for (int i = ex.tid; i < np; i += ex.nt) {
        t[i] = i < n ? run[(size_t)i * Y7T_GSI_COLS] : 0.0;
        for (int c = 0; c < 4; ++c) Y[i * 4 + c] = i < n ? run[(size_t)i * Y7T_GSI_COLS + 1 + c] : 0.0;
    }
    y7t_gsi_sync();
    for (long long e = ex.tid; e < (long long)np * np; e += ex.nt) {
        const int i = (int)(e / np), j = (int)(e % np);
        if (j >= (i / Y7T_GSI_PANEL + 1) * Y7T_GSI_PANEL) continue;
        double v;
        if (i < n && j < n) {
            v = y7t_gsi_kernel(t[i], t[j], ls);
            if (i == j) v = v + reg;
        } else {
            v = i == j ? 1.0 : 0.0;
        }
        A[(size_t)i * ld + j] = v;
    }
    y7t_gsi_sync();
    int fail = 0;
    for (int p = 0; p < nb && !fail; ++p) {
        const int k0 = p * Y7T_GSI_PANEL;
        for (int e = ex.tid; e < 256; e += ex.nt) D[e] = A[(size_t)(k0 + (e >> 4)) * ld + k0 + (e & 15)];
        y7t_gsi_sync();
        for (int j = 0; j < 16; ++j) {
            const double d = D[j * 16 + j];      // (read by every thread after a barrier: the branch below is uniform)
            if (!(d > 0.0)) { fail = 1; break; }
            const double l = sqrt(d);
            if (ex.wave == 0) {      // (the block is the first wave's; the other waves only keep the barriers)
                for (int i = j + 1 + ex.lane; i < 16; i += ex.nl) D[i * 16 + j] = D[i * 16 + j] / l;
                if (ex.lane == 0) Ld[j] = l;
            }
            y7t_gsi_sync();
            if (ex.wave == 0)
                for (int e = ex.lane; e < 256; e += ex.nl) {
                    const int i = e >> 4, k = e & 15;
                    if (j < k && k <= i) {
                        const double m = D[i * 16 + j] * D[k * 16 + j];
                        D[i * 16 + k] = D[i * 16 + k] - m;
                    }
                }
            y7t_gsi_sync();
        }
        if (fail) break;
        // the factored diagonal block back into A; the panel below it: L21 L11^T = A21, a thread per row
        for (int e = ex.tid; e < 256; e += ex.nt) {
            const int i = e >> 4, k = e & 15;
            if (k <= i) A[(size_t)(k0 + i) * ld + k0 + k] = i == k ? Ld[i] : D[e];
        }
        for (int i = k0 + 16 + ex.tid; i < np; i += ex.nt) {
            double* row = A + (size_t)i * ld + k0;
            double x[16];
#if Y7T_GSI_DEVICE
#pragma unroll
#endif
            for (int c = 0; c < 16; ++c) {
                double s = row[c];
#if Y7T_GSI_DEVICE
#pragma unroll
#endif
                for (int m = 0; m < c; ++m) {
                    const double pr = x[m] * D[c * 16 + m];
                    s = s - pr;
                }
                x[c] = s / Ld[c];
            }
#if Y7T_GSI_DEVICE
#pragma unroll
#endif
            for (int c = 0; c < 16; ++c) row[c] = x[c];
        }
        y7t_gsi_sync();
        for (int ti = p + 1; ti < nb; ++ti)
            for (int tj = p + 1 + ex.wave; tj <= ti; tj += ex.nw) y7t_gsi_tile(A, ld, ti * 16, tj * 16, k0, ex.lane);
        y7t_gsi_sync();
    }
    if (fail) {
        for (int e = ex.tid; e < n * 4; e += ex.nt) out[e] = run[(size_t)(e >> 2) * Y7T_GSI_COLS + 1 + (e & 3)];
        return Y7T_GSI_NOT_PD;
    }
    // L z = Y
    for (int p = 0; p < nb; ++p) {
        const int k0 = p * Y7T_GSI_PANEL;
        for (int c = ex.tid; c < 4; c += ex.nt)
            for (int r = 0; r < 16; ++r) {
                const double* row = A + (size_t)(k0 + r) * ld + k0;
                double s = Y[(k0 + r) * 4 + c];
                for (int m = 0; m < r; ++m) {
                    const double pr = row[m] * Y[(k0 + m) * 4 + c];
                    s = s - pr;
                }
                Y[(k0 + r) * 4 + c] = s / row[r];
            }
        y7t_gsi_sync();
        for (int i = k0 + 16 + ex.tid; i < np; i += ex.nt) {
            const double* row = A + (size_t)i * ld + k0;
            double s[4] = {Y[i * 4], Y[i * 4 + 1], Y[i * 4 + 2], Y[i * 4 + 3]};
            for (int m = 0; m < 16; ++m) {
                const double l = row[m];
                for (int c = 0; c < 4; ++c) {
                    const double pr = l * Y[(k0 + m) * 4 + c];
                    s[c] = s[c] - pr;
                }
            }
            for (int c = 0; c < 4; ++c) Y[i * 4 + c] = s[c];
        }
        y7t_gsi_sync();
    }
    // L^T a = z
    for (int p = nb - 1; p >= 0; --p) {
        const int k0 = p * Y7T_GSI_PANEL;
        for (int c = ex.tid; c < 4; c += ex.nt)
            for (int r = 15; r >= 0; --r) {
                double s = Y[(k0 + r) * 4 + c];
                for (int m = r + 1; m < 16; ++m) {
                    const double pr = A[(size_t)(k0 + m) * ld + k0 + r] * Y[(k0 + m) * 4 + c];
                    s = s - pr;
                }
                Y[(k0 + r) * 4 + c] = s / A[(size_t)(k0 + r) * ld + k0 + r];
            }
        y7t_gsi_sync();
        for (int i = ex.tid; i < k0; i += ex.nt) {
            double s[4] = {Y[i * 4], Y[i * 4 + 1], Y[i * 4 + 2], Y[i * 4 + 3]};
            for (int m = 0; m < 16; ++m) {
                const double l = A[(size_t)(k0 + m) * ld + i];
                for (int c = 0; c < 4; ++c) {
                    const double pr = l * Y[(k0 + m) * 4 + c];
                    s[c] = s[c] - pr;
                }
            }
            for (int c = 0; c < 4; ++c) Y[i * 4 + c] = s[c];
        }
        y7t_gsi_sync();
    }
    // out = K a
    for (int i = ex.tid; i < n; i += ex.nt) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        const double ti = t[i];
        for (int j = 0; j < n; ++j) {
            const double k = y7t_gsi_kernel(ti, t[j], ls);
            for (int c = 0; c < 4; ++c) {
                const double pr = k * Y[j * 4 + c];
                s[c] = s[c] + pr;
            }
        }
        for (int c = 0; c < 4; ++c) out[(size_t)i * 4 + c] = s[c];
    }
    return 0;
}
