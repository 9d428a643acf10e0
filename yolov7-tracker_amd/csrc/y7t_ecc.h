// y7t_ecc.h -- camera-motion estimation by ECC maximisation (cv2.findTransformECC, MOTION_EUCLIDEAN, as GMC.applyEcc of the reference calls it:
// tracker/botsort.py:78-109), stated once for the device kernels (y7t_ecc.hip) and for the CPU build of the same bodies (tests/_hostsim/ecc.py).
// DESIGN.md section 4 "GMC / ECC" is the specification; in short
//   prepare : BGR uint8 -> gray (round half up) -> 3x3 Gaussian sigma 1.5, reflect-101 (round half up) -> bilinear resize to (W / ds, H / ds), pixel-centre
//             convention (round half up) -> float32 I; gx, gy with the taps [-0.5, 0, 0.5], reflect-101.  float64 arithmetic in one fixed order, so I is the
//             integer and gx, gy the half-integers that the float64 restatement (tests/ecc_np.py) gives.
//   iterate : one pass over the template grid per Gauss-Newton iteration: float32 warp, bilinear sample (border 0) and Jacobian row per pixel, the 21 raw
//             sums of the iteration in float64, reduced in an order that depends on (h, w) only; the 3x3 solve in float64 from those sums.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define Y7T_ECC_HD __host__ __device__ inline
#else
#define Y7T_ECC_HD inline
#endif

enum {
    Y7T_ECC_NSUM = 21,           // N, sum I, sum I^2, sum T, sum T^2, sum I T, sum J (3), sum J I (3), sum J T (3), sum J J^T (00 01 02 11 12 22)
    Y7T_ECC_SLAB = 24,           // doubles per workgroup slab (21 used; 192 bytes)
    Y7T_ECC_THREADS = 1024,      // sixteen waves a workgroup: four a SIMD with one workgroup per compute unit, so that the gathers of several pixels are in flight
    Y7T_ECC_WAVE = 64,
    Y7T_ECC_NWAVE = Y7T_ECC_THREADS / Y7T_ECC_WAVE,
    Y7T_ECC_MAX_WG = 256,        // one workgroup per compute unit at 960 x 540 and above: at most 256 slabs to re-sum
    Y7T_ECC_PIX_PER_WG = 2048,   // below that, 2 pixels per work-item
    Y7T_ECC_CGROUPS = Y7T_ECC_THREADS / 32,      // the slab combine: 32 groups of 32 work-items (24 used), group g sums slabs g, g + 32, ...
};
enum { Y7T_ECC_RUNNING = 0, Y7T_ECC_CONVERGED = 1, Y7T_ECC_EXHAUSTED = 2, Y7T_ECC_FAILED = 3 };

// one pixel of a prepared plane: a bilinear tap of the iteration is one 16-byte load
struct alignas(16) Y7TEccPix { float I, gx, gy, pad; };

// the state one iteration hands to the next (two copies in the workspace, written alternately)
struct Y7TEccHdr {
    double p[3];          // theta, tx, ty
    double rho, rho_last;
    int iters, flag;      // iterations whose update has been applied; Y7T_ECC_*
    double pad;
};

// -- geometry: functions of (h, w) only --------------------------------------------------------------------------------------------------------------
Y7T_ECC_HD int y7t_ecc_num_wg(int h, int w) {
    const long long n = (long long)h * w, g = (n + Y7T_ECC_PIX_PER_WG - 1) / Y7T_ECC_PIX_PER_WG;
    return g < 1 ? 1 : g > Y7T_ECC_MAX_WG ? Y7T_ECC_MAX_WG : (int)g;
}
// pixels per workgroup: a contiguous run, a multiple of the workgroup size (trailing workgroups may be ragged or empty)
Y7T_ECC_HD long long y7t_ecc_chunk(int h, int w) {
    const long long n = (long long)h * w, g = y7t_ecc_num_wg(h, w), c = (n + g - 1) / g;
    return (c + Y7T_ECC_THREADS - 1) / Y7T_ECC_THREADS * Y7T_ECC_THREADS;
}
Y7T_ECC_HD size_t y7t_ecc_ws_bytes(int h, int w) { return 2 * sizeof(Y7TEccHdr) + (size_t)2 * y7t_ecc_num_wg(h, w) * Y7T_ECC_SLAB * sizeof(double); }
Y7T_ECC_HD Y7TEccHdr* y7t_ecc_hdr(void* ws, int k) { return (Y7TEccHdr*)ws + (k & 1); }
Y7T_ECC_HD double* y7t_ecc_slabs(void* ws, int h, int w, int k) {
    return (double*)((Y7TEccHdr*)ws + 2) + (size_t)(k & 1) * y7t_ecc_num_wg(h, w) * Y7T_ECC_SLAB;
}

// The combine of the slabs of one launch, the same order everywhere: partial[g][j] = sum over i of slab[g + i * CGROUPS][j] (i ascending, from 0.0), then
// S[j] = sum over g of partial[g][j] (g ascending, from 0.0).  This is the sequential statement (host build); k_ecc_iter runs the g's side by side.
Y7T_ECC_HD void y7t_ecc_combine(const double* slabs, int nwg, double* S) {
    for (int j = 0; j < Y7T_ECC_NSUM; ++j) {
        double a = 0.0;
        for (int g = 0; g < Y7T_ECC_CGROUPS; ++g) {
            double part = 0.0;
            for (int s = g; s < nwg; s += Y7T_ECC_CGROUPS) part += slabs[(size_t)s * Y7T_ECC_SLAB + j];
            a += part;
        }
        S[j] = a;
    }
}

// -- frame preparation -------------------------------------------------------------------------------------------------------------------------------
Y7T_ECC_HD int y7t_ecc_reflect101(int i, int n) {
    if (n == 1) return 0;
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : i > n - 1 ? n - 1 : i;      // (the clamp only serves tile overhang that is never written)
}
// Y = 0.114 B + 0.587 G + 0.299 R rounded half up, in integers
Y7T_ECC_HD int y7t_ecc_gray(const uint8_t* bgr, int W, int y, int x) {
    const uint8_t* p = bgr + ((size_t)y * W + x) * 3;
    return (114 * (int)p[0] + 587 * (int)p[1] + 299 * (int)p[2] + 500) / 1000;
}
// 3x3 Gaussian sigma 1.5: [a, b, a] x [a, b, a], a = e^(-1/4.5) / (1 + 2 e^(-1/4.5)); rows first, then columns; round half up
#define Y7T_ECC_GA 0.30780132912346997
#define Y7T_ECC_GB (1.0 - 2.0 * Y7T_ECC_GA)
Y7T_ECC_HD double y7t_ecc_blur(const uint8_t* bgr, int H, int W, int y, int x) {
    const int xl = y7t_ecc_reflect101(x - 1, W), xr = y7t_ecc_reflect101(x + 1, W);
    double r[3];
    for (int k = 0; k < 3; ++k) {
        const int yy = y7t_ecc_reflect101(y - 1 + k, H);
        const double l = y7t_ecc_gray(bgr, W, yy, xl), c = y7t_ecc_gray(bgr, W, yy, x), rr = y7t_ecc_gray(bgr, W, yy, xr);
        r[k] = Y7T_ECC_GA * (l + rr) + Y7T_ECC_GB * c;
    }
    return floor(Y7T_ECC_GA * (r[0] + r[2]) + Y7T_ECC_GB * r[1] + 0.5);
}
// source coordinate of a destination index (cv2.resize, INTER_LINEAR): lower tap, upper tap, fraction
Y7T_ECC_HD void y7t_ecc_resize_tap(int d, int n_src, int n_dst, int* i0, int* i1, double* f) {
    const double s = ((double)d + 0.5) * ((double)n_src / (double)n_dst) - 0.5;
    double fl = floor(s);
    double fr = s - fl;
    int a = (int)fl;
    if (a < 0) { a = 0; fr = 0.0; }
    if (a >= n_src - 1) { a = n_src - 1; fr = 0.0; }
    *i0 = a;
    *i1 = a + 1 < n_src ? a + 1 : n_src - 1;
    *f = fr;
}
// I of the plane at (y, x): (h, w) = (H / ds, W / ds); ds == 1 skips blur and resize
Y7T_ECC_HD float y7t_ecc_plane_I(const uint8_t* bgr, int H, int W, int ds, int h, int w, int y, int x) {
    if (ds <= 1) return (float)y7t_ecc_gray(bgr, W, y, x);
    int x0, x1, y0, y1;
    double fx, fy;
    y7t_ecc_resize_tap(x, W, w, &x0, &x1, &fx);
    y7t_ecc_resize_tap(y, H, h, &y0, &y1, &fy);
    const double p00 = y7t_ecc_blur(bgr, H, W, y0, x0), p01 = y7t_ecc_blur(bgr, H, W, y0, x1);
    const double p10 = y7t_ecc_blur(bgr, H, W, y1, x0), p11 = y7t_ecc_blur(bgr, H, W, y1, x1);
    const double top = (1.0 - fx) * p00 + fx * p01, bot = (1.0 - fx) * p10 + fx * p11;
    return (float)floor((1.0 - fy) * top + fy * bot + 0.5);
}

// -- one pixel of an iteration -----------------------------------------------------------------------------------------------------------------------
struct Y7TEccWarpF { float c, s, tx, ty; };

// our own sine / cosine and principal angle in plain float64 operations: the device's and the host's math libraries may round differently, and the
// host build is compared bit for bit
Y7T_ECC_HD void y7t_ecc_sincos(double th, double* s_out, double* c_out) {
    const double k = floor(th / 1.5707963267948966 + 0.5);
    const double r = (th - k * 1.5707963267948966) - k * 6.123233995736766e-17;
    const double r2 = r * r;
    double s = 0.0, c = 0.0;
    // Taylor series to r^23 / r^22 on |r| <= pi / 4 (truncation below 1e-19), Horner
    for (int n = 23; n >= 3; n -= 2) s = (s + 1.0) * (-r2 / (double)(n * (n - 1)));
    s = (s + 1.0) * r;
    for (int n = 22; n >= 2; n -= 2) c = (c + 1.0) * (-r2 / (double)(n * (n - 1)));
    c = c + 1.0;
    const long long q = (long long)k & 3;
    *s_out = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    *c_out = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}
// asin(sin(theta)): the angle folded into [-pi/2, pi/2]
Y7T_ECC_HD double y7t_ecc_principal(double th) {
    double t = th - 6.283185307179586 * floor(th / 6.283185307179586 + 0.5);
    if (t > 1.5707963267948966) t = 3.141592653589793 - t;
    if (t < -1.5707963267948966) t = -3.141592653589793 - t;
    return t;
}
Y7T_ECC_HD Y7TEccWarpF y7t_ecc_warp_f32(const double* p) {
    double s, c;
    y7t_ecc_sincos(p[0], &s, &c);
    Y7TEccWarpF wp;
    wp.c = (float)c; wp.s = (float)s; wp.tx = (float)p[1]; wp.ty = (float)p[2];
    return wp;
}

Y7T_ECC_HD Y7TEccPix y7t_ecc_tap(const Y7TEccPix* p, bool inside) {
    Y7TEccPix v = *p;
    if (!inside) { v.I = 0.0f; v.gx = 0.0f; v.gy = 0.0f; }
    return v;
}
// adds pixel (x, y) of the template grid to the 21 per-lane sums; reads img only inside [0, h) x [0, w)
Y7T_ECC_HD void y7t_ecc_pixel(const Y7TEccPix* img, const Y7TEccPix* tmpl, int h, int w, int x, int y, const Y7TEccWarpF wp, double* acc) {
    const float xf = (float)x, yf = (float)y;
    const float xw = wp.c * xf - wp.s * yf + wp.tx;
    const float yw = wp.s * xf + wp.c * yf + wp.ty;
    if (!(xw > -1.0f && xw < (float)w && yw > -1.0f && yw < (float)h)) return;      // (also NaN)
    const float xr = floorf(xw + 0.5f), yr = floorf(yw + 0.5f);
    if (!(xr >= 0.0f && xr < (float)w && yr >= 0.0f && yr < (float)h)) return;      // the mask: the rounded position lies inside the image
    const float x0f = floorf(xw), y0f = floorf(yw);
    const float fx = xw - x0f, fy = yw - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;                                          // in [-1, w - 1] x [-1, h - 1]
    // four taps, constant 0 border: each is one 16-byte load from a clamped (always valid) address, zeroed when the tap lies outside
    const int xc0 = x0 < 0 ? 0 : x0, xc1 = x0 + 1 < w ? x0 + 1 : w - 1, yc0 = y0 < 0 ? 0 : y0, yc1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const bool xa = x0 >= 0, xb = x0 + 1 < w, ya = y0 >= 0, yb = y0 + 1 < h;
    const Y7TEccPix p00 = y7t_ecc_tap(img + (size_t)yc0 * w + xc0, xa && ya);
    const Y7TEccPix p01 = y7t_ecc_tap(img + (size_t)yc0 * w + xc1, xb && ya);
    const Y7TEccPix p10 = y7t_ecc_tap(img + (size_t)yc1 * w + xc0, xa && yb);
    const Y7TEccPix p11 = y7t_ecc_tap(img + (size_t)yc1 * w + xc1, xb && yb);
    const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy), w10 = (1.0f - fx) * fy, w11 = fx * fy;
    const float Iw = w00 * p00.I + w01 * p01.I + w10 * p10.I + w11 * p11.I;
    const float gxw = w00 * p00.gx + w01 * p01.gx + w10 * p10.gx + w11 * p11.gx;
    const float gyw = w00 * p00.gy + w01 * p01.gy + w10 * p10.gy + w11 * p11.gy;
    const float j0 = -gxw * (xf * wp.s + yf * wp.c) + gyw * (xf * wp.c - yf * wp.s);
    const double I = Iw, T = tmpl[(size_t)y * w + x].I, J0 = j0, J1 = gxw, J2 = gyw;
    acc[0] += 1.0;
    acc[1] += I;
    acc[2] += I * I;
    acc[3] += T;
    acc[4] += T * T;
    acc[5] += I * T;
    acc[6] += J0; acc[7] += J1; acc[8] += J2;
    acc[9] += J0 * I; acc[10] += J1 * I; acc[11] += J2 * I;
    acc[12] += J0 * T; acc[13] += J1 * T; acc[14] += J2 * T;
    acc[15] += J0 * J0; acc[16] += J0 * J1; acc[17] += J0 * J2;
    acc[18] += J1 * J1; acc[19] += J1 * J2; acc[20] += J2 * J2;
}

// -- the 3x3 solve ---------------------------------------------------------------------------------------------------------------------------------
// inverse of the symmetric 3x3 (00 01 02 11 12 22) by cofactors; a zero determinant gives zeros (cv::Mat::inv)
Y7T_ECC_HD void y7t_ecc_inv3(const double* a, double* inv) {
    const double a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    if (det != 0.0) {
        const double d = 1.0 / det;
        inv[0] = c00 * d; inv[1] = c01 * d; inv[2] = c02 * d; inv[3] = c11 * d; inv[4] = c12 * d; inv[5] = c22 * d;
    } else {
        for (int i = 0; i < 6; ++i) inv[i] = 0.0;
    }
}
Y7T_ECC_HD void y7t_ecc_symv(const double* m, const double* v, double* out) {
    out[0] = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
    out[1] = m[1] * v[0] + m[3] * v[1] + m[4] * v[2];
    out[2] = m[2] * v[0] + m[4] * v[1] + m[5] * v[2];
}
// one iteration's update from its 21 combined sums: rho_last <- rho, rho, the failure tests, p += dp, iters += 1
Y7T_ECC_HD void y7t_ecc_solve(const double* S, Y7TEccHdr* hd) {
    const double N = S[0], mI = S[1] / N, mT = S[3] / N;
    const double in2 = S[2] - N * mI * mI, tn2 = S[4] - N * mT * mT;        // imgNorm^2 = N sigma_I^2, tmpNorm^2
    const double corr = S[5] - N * mI * mT;
    double JI[3], JT[3], Hinv[6], ip[3], tp[3], e[3], dp[3];
    for (int k = 0; k < 3; ++k) { JI[k] = S[9 + k] - mI * S[6 + k]; JT[k] = S[12 + k] - mT * S[6 + k]; }
    hd->iters += 1;
    hd->rho_last = hd->rho;
    hd->rho = corr / (sqrt(in2) * sqrt(tn2));
    if (!(fabs(hd->rho) <= 1.7976931348623157e308)) { hd->flag = Y7T_ECC_FAILED; return; }      // NaN or infinite
    y7t_ecc_inv3(S + 15, Hinv);
    y7t_ecc_symv(Hinv, JI, ip);
    y7t_ecc_symv(Hinv, JT, tp);
    const double lam_n = in2 - (JI[0] * ip[0] + JI[1] * ip[1] + JI[2] * ip[2]);
    const double lam_d = corr - (JI[0] * tp[0] + JI[1] * tp[1] + JI[2] * tp[2]);
    if (lam_d <= 0.0) { hd->flag = Y7T_ECC_FAILED; return; }
    const double lam = lam_n / lam_d;
    for (int k = 0; k < 3; ++k) e[k] = lam * JT[k] - JI[k];
    y7t_ecc_symv(Hinv, e, dp);
    hd->p[0] = y7t_ecc_principal(hd->p[0]) + dp[0];
    hd->p[1] += dp[1];
    hd->p[2] += dp[2];
}
// the loop condition of findTransformECC before iteration iters + 1: for (i = 1; i <= max_iters && |rho - rho_last| >= eps; i++)
Y7T_ECC_HD void y7t_ecc_check(Y7TEccHdr* hd, int max_iters, double eps) {
    if (hd->flag) return;
    if (!(fabs(hd->rho - hd->rho_last) >= eps)) hd->flag = Y7T_ECC_CONVERGED;
    else if (hd->iters + 1 > max_iters) hd->flag = Y7T_ECC_EXHAUSTED;
}
Y7T_ECC_HD void y7t_ecc_start(Y7TEccHdr* hd, double th, double tx, double ty, double eps) {
    hd->p[0] = th; hd->p[1] = tx; hd->p[2] = ty;
    hd->rho = -1.0;
    hd->rho_last = -eps;
    hd->iters = 0; hd->flag = Y7T_ECC_RUNNING; hd->pad = 0.0;
}
// the 2x3 warp and the status {iterations, flag, rho, |rho - rho_last|}; identity on failure (the reference catches the exception, botsort.py:104-107)
Y7T_ECC_HD void y7t_ecc_finish(const Y7TEccHdr* hd, double* warp6, double* status4) {
    double s = 0.0, c = 1.0, tx = 0.0, ty = 0.0;
    if (hd->flag != Y7T_ECC_FAILED) { y7t_ecc_sincos(hd->p[0], &s, &c); tx = hd->p[1]; ty = hd->p[2]; }
    warp6[0] = c; warp6[1] = 0.0 - s; warp6[2] = tx; warp6[3] = s; warp6[4] = c; warp6[5] = ty;
    status4[0] = (double)hd->iters; status4[1] = (double)hd->flag; status4[2] = hd->rho; status4[3] = fabs(hd->rho - hd->rho_last);
}
