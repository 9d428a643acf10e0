// y7t_orb.h -- feature-based camera-motion estimation (GMC.applyFeaures of the reference, tracker/botsort.py:111-235: FAST corners, rotated-BRIEF descriptors,
// Hamming 2-NN matching, three filters, a 4-DOF RANSAC) stated once for the device kernels (y7t_orb.hip) and for the CPU build of the same bodies
// (tests/_hostsim/orb.py).  DESIGN.md section 4 "GMC / features" is the specification and tests/orb_np.py its NumPy restatement; every stage is integer arithmetic or
// single correctly-rounded float64 operations, so the three agree bit for bit.  Contraction: this file is compiled with -ffp-contract=off on both sides, and the
// float64 stages (plane, direction, rotation, statistics, refinement) also carry `#pragma clang fp contract(off)`; the inlier test is integers.
#pragma once
#include "y7t_ecc.h"      // the gray level and the resize taps are ECC's
#define Y7T_ORB_HD Y7T_ECC_HD
#if defined(__HIPCC__)
#define Y7T_ORB_TABLE static __device__ __constant__ const
#else
#define Y7T_ORB_TABLE static const
#endif
#include "y7t_orb_pattern.h"
#if defined(__clang__)
#define Y7T_ORB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define Y7T_ORB_NO_CONTRACT
#endif

enum {
    Y7T_ORB_FAST_T = 20,         // a corner scores above this
    Y7T_ORB_EDGE = 31,           // ORB's border: the patch (15) and the rotated pattern (13 sqrt 2 -> 19) stay inside
    Y7T_ORB_HALF = 15,
    Y7T_ORB_NHYP = 2000,         // RANSAC hypotheses (OpenCV's maxIters), no early exit
    Y7T_ORB_MAX_DIM = 8192,      // plane sides: the integer inlier test is exact below 2^13
    Y7T_ORB_MAX_CAP = 65536,     // keypoint capacity: the integer sums stay below 2^63
    Y7T_ORB_NTAP = 12,           // offsets y7t_orb_layout reports
};
enum { Y7T_ORB_OK = 0, Y7T_ORB_NO_MATCHES = 1, Y7T_ORB_NOT_ENOUGH = 2, Y7T_ORB_NO_MODEL = 3 };

// a keypoint / descriptor STATE: header, cap descriptors of 32 bytes, cap keypoints {x, y}
struct Y7TOrbHdr { int n, total, truncated, h, w, pad[3]; };
struct Y7TOrbKp { int x, y; };
struct alignas(16) Y7TOrbMatch { int j1, d1, j2, d2; };      // best two of a previous descriptor among the current ones, ordered by (distance, index)
struct alignas(16) Y7TOrbPair { int px, py, cx, cy; };       // a good match: previous and current keypoint
struct Y7TOrbEst { int n_good, flag, n_first, winner, n_inliers, pad[3]; };      // the estimate's header in the workspace

Y7T_ORB_HD size_t y7t_orb_state_size(int cap) { return sizeof(Y7TOrbHdr) + (size_t)cap * 40; }
Y7T_ORB_HD unsigned long long* y7t_orb_desc(void* st) { return (unsigned long long*)((char*)st + sizeof(Y7TOrbHdr)); }
Y7T_ORB_HD Y7TOrbKp* y7t_orb_kps(void* st, int cap) { return (Y7TOrbKp*)((char*)st + sizeof(Y7TOrbHdr) + (size_t)cap * 32); }

// the workspace: byte offsets of {plane, scores, keep, smooth (h w uint8 each), row counts, row offsets (h ints each), moments (cap x 2 ints), matches (cap x 16),
// good (cap x 16), estimate header (32), hypothesis counts (2000 ints)}, then the total
Y7T_ORB_HD void y7t_orb_layout(int h, int w, int cap, size_t* off) {
    const size_t px = ((size_t)h * w + 15) / 16 * 16, rows = ((size_t)h * 4 + 15) / 16 * 16;
    size_t o = 0;
    for (int i = 0; i < 4; ++i) { off[i] = o; o += px; }
    off[4] = o; o += rows;
    off[5] = o; o += rows;
    off[6] = o; o += (size_t)cap * 8;
    off[7] = o; o += (size_t)cap * 16;
    off[8] = o; o += (size_t)cap * 16;
    off[9] = o; o += sizeof(Y7TOrbEst);
    off[10] = o; o += (size_t)Y7T_ORB_NHYP * 4;
    off[11] = o;
}

// -- 1. plane: gray, bilinear resize with ECC's source-coordinate rule, round half up --------------------------------------------------------------------------
Y7T_ORB_HD uint8_t y7t_orb_plane_px(const uint8_t* bgr, int H, int W, int ds, int h, int w, int y, int x) {
    Y7T_ORB_NO_CONTRACT
    if (ds <= 1) return (uint8_t)y7t_ecc_gray(bgr, W, y, x);
    int x0, x1, y0, y1;
    double fx, fy;
    y7t_ecc_resize_tap(x, W, w, &x0, &x1, &fx);
    y7t_ecc_resize_tap(y, H, h, &y0, &y1, &fy);
    const double p00 = y7t_ecc_gray(bgr, W, y0, x0), p01 = y7t_ecc_gray(bgr, W, y0, x1), p10 = y7t_ecc_gray(bgr, W, y1, x0), p11 = y7t_ecc_gray(bgr, W, y1, x1);
    const double top = (1.0 - fx) * p00 + fx * p01, bot = (1.0 - fx) * p10 + fx * p11;
    return (uint8_t)(int)floor((1.0 - fy) * top + fy * bot + 0.5);
}

// -- 2. FAST-9/16 -------------------------------------------------------------------------------------------------------------------------------------------------
// c points at the centre pixel of a buffer with `stride` bytes a row; the ring of radius 3 around it must be readable.  The score, or 0 when it is not above the
// threshold.  An arc of 9 of the 16 ring pixels holds ring pixel i or i + 8 for every i, so a pair (i, i + 8) with both differences within the threshold rules a corner out.
Y7T_ORB_HD int y7t_orb_fast_score(const uint8_t* c, int stride) {
    const int o[16] = {-3 * stride, -3 * stride + 1, -2 * stride + 2, -stride + 3, 3, stride + 3, 2 * stride + 2, 3 * stride + 1,
                       3 * stride, 3 * stride - 1, 2 * stride - 2, stride - 3, -3, -stride - 3, -2 * stride - 2, -3 * stride - 1};
    const int centre = c[0];
    int d[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = (int)c[o[i]] - centre;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int a = d[i] < 0 ? -d[i] : d[i], b = d[i + 8] < 0 ? -d[i + 8] : d[i + 8];
        if (a <= Y7T_ORB_FAST_T && b <= Y7T_ORB_FAST_T) return 0;
    }
    int best = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        int lo = d[s], hi = d[s];
#pragma unroll
        for (int k = 1; k < 9; ++k) {
            const int v = d[(s + k) & 15];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        best = lo > best ? lo : best;            // the brighter arc: its minimum difference
        best = -hi > best ? -hi : best;          // the darker arc: the minimum of the negated differences
    }
    return best > Y7T_ORB_FAST_T ? best : 0;
}

// strictly greater than the 8 neighbours (s points into the score map; (y, x) at least one pixel inside it)
Y7T_ORB_HD bool y7t_orb_is_max(const uint8_t* s, int w) {
    const int v = s[0];
    return v > 0 && v > s[-w - 1] && v > s[-w] && v > s[-w + 1] && v > s[-1] && v > s[1] && v > s[w - 1] && v > s[w] && v > s[w + 1];
}

// -- 3. mask (botsort.py:126-132 per keypoint) and ORB's border ----------------------------------------------------------------------------------------------------
Y7T_ORB_HD int y7t_orb_trunc(double v) {      // astype(int) of a box coordinate: toward zero (NaN 0, clipped to +-1e9)
    if (!(v == v)) return 0;
    return (int)(v > 1e9 ? 1e9 : v < -1e9 ? -1e9 : v);
}
Y7T_ORB_HD int y7t_orb_slice_bound(int i, int n) {      // a bound of a Python slice on an axis of n
    if (i < 0) { i += n; return i < 0 ? 0 : i; }
    return i > n ? n : i;
}
// dets: n_dets rows of 6 float32 (tlbr first), full-resolution pixels.  true: the keypoint is kept
Y7T_ORB_HD bool y7t_orb_unmasked(const float* dets, int n_dets, int ds, int h, int w, int x, int y) {
    if (!(y >= (int)(0.02 * (double)h) && y < (int)(0.98 * (double)h) && x >= (int)(0.02 * (double)w) && x < (int)(0.98 * (double)w))) return false;
    if (!(x >= Y7T_ORB_EDGE && x < w - Y7T_ORB_EDGE && y >= Y7T_ORB_EDGE && y < h - Y7T_ORB_EDGE)) return false;
    for (int k = 0; k < n_dets; ++k) {
        const float* d = dets + (size_t)k * 6;
        const int x0 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[0] / (double)ds), w), y0 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[1] / (double)ds), h);
        const int x1 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[2] / (double)ds), w), y1 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[3] / (double)ds), h);
        if (x >= x0 && x < x1 && y >= y0 && y < y1) return false;
    }
    return true;
}

// -- 5. orientation -----------------------------------------------------------------------------------------------------------------------------------------------
Y7T_ORB_HD int y7t_orb_umax(int a) {
    const int u[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    return u[a];
}
// patch position idx in [0, 961) of the keypoint at c (a pointer into the plane): adds to m10, m01
Y7T_ORB_HD void y7t_orb_moment_term(const uint8_t* c, int w, int idx, int* m10, int* m01) {
    const int r = idx / 31, dy = r - Y7T_ORB_HALF, dx = idx - r * 31 - Y7T_ORB_HALF;
    if ((dx < 0 ? -dx : dx) > y7t_orb_umax(dy < 0 ? -dy : dy)) return;
    const int v = c[dy * w + dx];
    *m10 += dx * v;
    *m01 += dy * v;
}
Y7T_ORB_HD void y7t_orb_direction(int m10, int m01, double* c, double* s) {
    Y7T_ORB_NO_CONTRACT
    if (m10 == 0 && m01 == 0) { *c = 1.0; *s = 0.0; return; }
    const double r = sqrt((double)((long long)m10 * m10 + (long long)m01 * m01));
    *c = (double)m10 / r;
    *s = (double)m01 / r;
}

// -- 6. smoothing: 7 x 7 Gaussian sigma 2, taps {72, 134, 195, 222, 195, 134, 72} / 2^10 both ways, reflect-101, one rounding: (sum + 2^19) >> 20 -----------------------
Y7T_ORB_HD int y7t_orb_tap(int k) {
    const int t[7] = {72, 134, 195, 222, 195, 134, 72};
    return t[k];
}
Y7T_ORB_HD uint8_t y7t_orb_smooth_px(const uint8_t* plane, int h, int w, int y, int x) {
    int acc = 0;
    for (int j = 0; j < 7; ++j) {
        const uint8_t* row = plane + (size_t)y7t_ecc_reflect101(y - 3 + j, h) * w;
        int r = 0;
        for (int k = 0; k < 7; ++k) r += y7t_orb_tap(k) * (int)row[y7t_ecc_reflect101(x - 3 + k, w)];
        acc += y7t_orb_tap(j) * r;
    }
    return (uint8_t)((acc + (1 << 19)) >> 20);
}

// -- 7. descriptor --------------------------------------------------------------------------------------------------------------------------------------------------
// bit i of the keypoint at c (a pointer into the SMOOTHED plane): I(rot(a_i)) < I(rot(b_i)), rot rounded half to even
Y7T_ORB_HD int y7t_orb_bit(const uint8_t* c, int w, int i, double co, double si) {
    Y7T_ORB_NO_CONTRACT
    const double ax = y7t_orb_pattern[i][0], ay = y7t_orb_pattern[i][1], bx = y7t_orb_pattern[i][2], by = y7t_orb_pattern[i][3];
    const int rax = (int)rint(ax * co - ay * si), ray = (int)rint(ax * si + ay * co);
    const int rbx = (int)rint(bx * co - by * si), rby = (int)rint(bx * si + by * co);
    return c[ray * w + rax] < c[rby * w + rbx] ? 1 : 0;
}

// -- 8. matching ----------------------------------------------------------------------------------------------------------------------------------------------------
Y7T_ORB_HD int y7t_orb_popc(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
Y7T_ORB_HD int y7t_orb_hamming(const unsigned long long* a, const unsigned long long* b) {
    return y7t_orb_popc(a[0] ^ b[0]) + y7t_orb_popc(a[1] ^ b[1]) + y7t_orb_popc(a[2] ^ b[2]) + y7t_orb_popc(a[3] ^ b[3]);
}
// candidates arrive with ascending index j, so strict comparisons give the (distance, index) order
Y7T_ORB_HD void y7t_orb_best_two(Y7TOrbMatch* m, int j, int d) {
    if (d < m->d1) { m->j2 = m->j1; m->d2 = m->d1; m->j1 = j; m->d1 = d; }
    else if (d < m->d2) { m->j2 = j; m->d2 = d; }
}

// -- 9. filters (botsort.py:169-195) --------------------------------------------------------------------------------------------------------------------------------
Y7T_ORB_HD bool y7t_orb_first_tests(const Y7TOrbMatch m, int dx, int dy, int h, int w) {
    return (double)m.d1 < 0.9 * (double)m.d2 && (double)(dx < 0 ? -dx : dx) < 0.25 * (double)w && (double)(dy < 0 ? -dy : dy) < 0.25 * (double)h;
}
// mean and standard deviation of n integers from their exact sums: mean = S / n, std = sqrt(n S2 - S^2) / n
Y7T_ORB_HD void y7t_orb_mean_std(long long n, long long s, long long s2, double* mean, double* sd) {
    Y7T_ORB_NO_CONTRACT
    *mean = (double)s / (double)n;
    *sd = sqrt((double)(n * s2 - s * s)) / (double)n;
}
Y7T_ORB_HD bool y7t_orb_one_sided(int d, double mean, double sd) {      // (d - mean) < 2.5 std, no absolute value, as written there
    Y7T_ORB_NO_CONTRACT
    const double a = (double)d - mean, b = 2.5 * sd;
    return a < b;
}

// -- 10. RANSAC -----------------------------------------------------------------------------------------------------------------------------------------------------
Y7T_ORB_HD uint32_t y7t_orb_fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
// point c (0 or 1) of hypothesis k among n
Y7T_ORB_HD int y7t_orb_pick(int k, int c, int n) { return (int)(y7t_orb_fmix32(((uint32_t)(2 * k + c) * 0x9E3779B1u) ^ ((uint32_t)n * 0x85EBCA77u)) % (uint32_t)n); }

// the similarity through two matches, scaled by D = |source difference|^2 so that it is integers: D a = A, D b = B
struct Y7TOrbModel { long long A, B, D; int x1, y1, u1, v1; };
Y7T_ORB_HD bool y7t_orb_model(const Y7TOrbPair p, const Y7TOrbPair q, Y7TOrbModel* m) {
    const long long dx = q.px - p.px, dy = q.py - p.py, ex = q.cx - p.cx, ey = q.cy - p.cy;
    m->D = dx * dx + dy * dy;
    m->A = dx * ex + dy * ey;
    m->B = dx * ey - dy * ex;
    m->x1 = p.px; m->y1 = p.py; m->u1 = p.cx; m->v1 = p.cy;
    return m->D != 0;
}
// squared reprojection error <= 9, multiplied through by D^2.  Coordinates below 2^13: |A|, |B|, D < 2^27, the residuals < 2^43; a residual above 3 D is no
// inlier, and below that the squares stay under 2^58
Y7T_ORB_HD bool y7t_orb_inlier(const Y7TOrbModel& m, const Y7TOrbPair g) {
    const long long x = g.px - m.x1, y = g.py - m.y1, u = g.cx - m.u1, v = g.cy - m.v1;
    long long rx = m.A * x - m.B * y - m.D * u, ry = m.B * x + m.A * y - m.D * v;
    rx = rx < 0 ? -rx : rx;
    ry = ry < 0 ? -ry : ry;
    const long long lim = 3 * m.D;
    return rx <= lim && ry <= lim && rx * rx + ry * ry <= lim * lim;
}

// -- 11. refinement: the least-squares similarity over the inliers from S = {sum x, sum y, sum u, sum v, sum (x^2 + y^2), sum (x u + y v), sum (x v - y u)} ------------
Y7T_ORB_HD bool y7t_orb_refine(long long n, const long long* S, int ds, double* warp6) {
    Y7T_ORB_NO_CONTRACT
    const long long q = n * S[4] - S[0] * S[0] - S[1] * S[1];
    const long long sa = n * S[5] - S[0] * S[2] - S[1] * S[3];
    const long long sb = n * S[6] - S[0] * S[3] + S[1] * S[2];
    if (q == 0) return false;
    const double a = (double)sa / (double)q, b = (double)sb / (double)q;
    const double tx = (((double)S[2] - a * (double)S[0]) + b * (double)S[1]) / (double)n;
    const double ty = (((double)S[3] - b * (double)S[0]) - a * (double)S[1]) / (double)n;
    warp6[0] = a; warp6[1] = 0.0 - b; warp6[2] = tx * (double)ds; warp6[3] = b; warp6[4] = a; warp6[5] = ty * (double)ds;
    return true;
}
Y7T_ORB_HD void y7t_orb_finish(int n_prev, int n_cur, int trunc, const Y7TOrbEst* e, bool have, double* warp6, double* status6) {
    if (!have) { warp6[0] = 1.0; warp6[1] = 0.0; warp6[2] = 0.0; warp6[3] = 0.0; warp6[4] = 1.0; warp6[5] = 0.0; }
    status6[0] = n_prev; status6[1] = n_cur; status6[2] = e->n_good; status6[3] = e->n_inliers; status6[4] = e->flag; status6[5] = trunc;
}
