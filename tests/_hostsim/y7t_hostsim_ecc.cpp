// tests/_hostsim/y7t_hostsim_ecc.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of the ECC kernel bodies of yolov7-tracker_amd/csrc/y7t_ecc.h: the per-pixel programs of the prepare and the iteration launch run one "lane" at a
// time, and the reductions follow the device's order (per lane over its pixels; the shuffle tree of the 64 lanes of a wave; the waves of a workgroup in order;
// the workgroups' slabs in the order of y7t_ecc_combine), so that the sums and the warp can be compared with the device's bit for bit.  The product package never loads this library.
#include <string.h>
#include <vector>
#include "../../yolov7-tracker_amd/csrc/y7t_ecc.h"

// launch k of the iteration kernel over the whole grid (csrc/y7t_ecc.hip: k_ecc_iter)
static void hs_iter_launch(const Y7TEccPix* tmpl, const Y7TEccPix* img, int h, int w, int k, int solve_prev, int max_iters, double eps, void* ws) {
    const int nwg = y7t_ecc_num_wg(h, w);
    const long long chunk = y7t_ecc_chunk(h, w), npix = (long long)h * w;
    const Y7TEccHdr* prev = y7t_ecc_hdr(ws, k - 1);
    Y7TEccHdr* cur = y7t_ecc_hdr(ws, k);
    if (prev->flag) { *cur = *prev; return; }
    double S[Y7T_ECC_SLAB] = {0};
    if (solve_prev) y7t_ecc_combine(y7t_ecc_slabs(ws, h, w, k - 1), nwg, S);
    Y7TEccHdr hd = *prev;      // (every workgroup computes the same: once is enough here)
    if (solve_prev) y7t_ecc_solve(S, &hd);
    y7t_ecc_check(&hd, max_iters, eps);
    *cur = hd;
    if (hd.flag) return;
    const Y7TEccWarpF wp = y7t_ecc_warp_f32(hd.p);
    std::vector<double> lanes((size_t)Y7T_ECC_THREADS * Y7T_ECC_NSUM);
    double* out = y7t_ecc_slabs(ws, h, w, k);
    for (int b = 0; b < nwg; ++b) {
        const long long lo = (long long)b * chunk, hi = lo + chunk < npix ? lo + chunk : npix;
        for (int t = 0; t < Y7T_ECC_THREADS; ++t) {
            double* acc = &lanes[(size_t)t * Y7T_ECC_NSUM];
            for (int i = 0; i < Y7T_ECC_NSUM; ++i) acc[i] = 0.0;
            for (long long i = lo + t; i < hi; i += Y7T_ECC_THREADS) {
                const int y = (int)(i / w), x = (int)(i - (long long)y * w);
                y7t_ecc_pixel(img, tmpl, h, w, x, y, wp, acc);
            }
        }
        double waves[Y7T_ECC_NWAVE][Y7T_ECC_NSUM];
        for (int wv = 0; wv < Y7T_ECC_NWAVE; ++wv) {
            double* L = &lanes[(size_t)wv * Y7T_ECC_WAVE * Y7T_ECC_NSUM];
            for (int off = Y7T_ECC_WAVE / 2; off >= 1; off >>= 1)      // __shfl_down: lane l adds lane l + off (what reaches lane 0 needs only l < off)
                for (int l = 0; l < off; ++l)
                    for (int i = 0; i < Y7T_ECC_NSUM; ++i) L[(size_t)l * Y7T_ECC_NSUM + i] += L[(size_t)(l + off) * Y7T_ECC_NSUM + i];
            for (int i = 0; i < Y7T_ECC_NSUM; ++i) waves[wv][i] = L[i];
        }
        for (int j = 0; j < Y7T_ECC_SLAB; ++j) {
            double a = 0.0;
            if (j < Y7T_ECC_NSUM)
                for (int wv = 0; wv < Y7T_ECC_NWAVE; ++wv) a += waves[wv][j];
            out[(size_t)b * Y7T_ECC_SLAB + j] = a;
        }
    }
}

extern "C" {
int hs_ecc_pix_bytes(void) { return (int)sizeof(Y7TEccPix); }
int hs_ecc_num_wg(int h, int w) { return y7t_ecc_num_wg(h, w); }
size_t hs_ecc_ws_bytes(int h, int w) { return y7t_ecc_ws_bytes(h, w); }

void hs_ecc_prepare(const uint8_t* bgr, int H, int W, int ds, float* plane) {
    const int h = H / ds, w = W / ds;
    std::vector<float> I((size_t)h * w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) I[(size_t)y * w + x] = y7t_ecc_plane_I(bgr, H, W, ds, h, w, y, x);
    Y7TEccPix* out = (Y7TEccPix*)plane;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int xl = y7t_ecc_reflect101(x - 1, w), xr = y7t_ecc_reflect101(x + 1, w), yu = y7t_ecc_reflect101(y - 1, h), yd = y7t_ecc_reflect101(y + 1, h);
            Y7TEccPix o;
            o.I = I[(size_t)y * w + x];
            o.gx = 0.5f * (I[(size_t)y * w + xr] - I[(size_t)y * w + xl]);
            o.gy = 0.5f * (I[(size_t)yd * w + x] - I[(size_t)yu * w + x]);
            o.pad = 0.0f;
            out[(size_t)y * w + x] = o;
        }
}

void hs_ecc_sums(const void* tmpl, const void* img, int h, int w, double th, double tx, double ty, double* sums21) {
    std::vector<double> ws(y7t_ecc_ws_bytes(h, w) / 8 + 1);
    y7t_ecc_start(y7t_ecc_hdr(ws.data(), 0), th, tx, ty, -1.0);
    hs_iter_launch((const Y7TEccPix*)tmpl, (const Y7TEccPix*)img, h, w, 1, 0, 1, -1.0, ws.data());
    y7t_ecc_combine(y7t_ecc_slabs(ws.data(), h, w, 1), y7t_ecc_num_wg(h, w), sums21);
}

void hs_ecc_align(const void* tmpl, const void* img, int h, int w, int max_iters, double eps, double* warp6, double* status4) {
    std::vector<double> ws(y7t_ecc_ws_bytes(h, w) / 8 + 1);
    y7t_ecc_start(y7t_ecc_hdr(ws.data(), 0), 0.0, 0.0, 0.0, eps);
    for (int k = 1; k <= max_iters + 1; ++k) hs_iter_launch((const Y7TEccPix*)tmpl, (const Y7TEccPix*)img, h, w, k, k > 1, max_iters, eps, ws.data());
    y7t_ecc_finish(y7t_ecc_hdr(ws.data(), max_iters + 1), warp6, status4);
}

// the 3x3 solve on its own: state = {theta, tx, ty, rho, rho_last}, iters_flag = {iters, flag}
void hs_ecc_solve(const double* sums21, double* state5, int* iters_flag) {
    Y7TEccHdr hd;
    memset(&hd, 0, sizeof(hd));
    for (int i = 0; i < 3; ++i) hd.p[i] = state5[i];
    hd.rho = state5[3]; hd.rho_last = state5[4]; hd.iters = iters_flag[0]; hd.flag = iters_flag[1];
    y7t_ecc_solve(sums21, &hd);
    for (int i = 0; i < 3; ++i) state5[i] = hd.p[i];
    state5[3] = hd.rho; state5[4] = hd.rho_last; iters_flag[0] = hd.iters; iters_flag[1] = hd.flag;
}
void hs_ecc_sincos(double th, double* sc) { y7t_ecc_sincos(th, sc, sc + 1); }
double hs_ecc_principal(double th) { return y7t_ecc_principal(th); }
}
