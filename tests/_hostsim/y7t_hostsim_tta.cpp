// tests/_hostsim/y7t_hostsim_tta.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of yolov7-tracker_amd/csrc/y7t_tta.h: the scale + layout body of k_tta_scale_layout run one output pixel at a time (the SAME function the device's
// threads call; the kernel's float -> fp16 rounding is left to the caller, one numpy astype) and the de-scale / de-flip of k_decode_append on rows of xywh.
// The product package never loads this library.
#include "../../yolov7-tracker_amd/csrc/y7t_tta.h"
#include <stddef.h>

extern "C" {
// -> out (B, Ho, Wo, ldout) float32, Ho x Wo = Hp x Wp (/ 2 with reorg)
void hs_tta_scale_layout(const void* img, int is_u8, int B, int H, int W, int flip, int hs, int ws, int Hp, int Wp, int reorg, float* out, int ldout) {
    const Y7TTtaGeom g = {H, W, flip, hs, ws, Hp, Wp};
    const int Ho = reorg ? Hp / 2 : Hp, Wo = reorg ? Wp / 2 : Wp;
    for (int b = 0; b < B; ++b)
        for (int yo = 0; yo < Ho; ++yo)
            for (int xo = 0; xo < Wo; ++xo) {
                float v[16];
                y7t_tta_layout_px(img, is_u8, b, g, reorg, yo, xo, v);
                float* o = out + (((size_t)b * Ho + yo) * Wo + xo) * ldout;
                for (int c = 0; c < ldout; ++c) o[c] = v[c];
            }
}

// n rows of {x, y, w, h}, transformed in place
void hs_tta_descale_deflip(float* xywh, int n, float scale, int flip, float flip_extent) {
    const Y7TTtaPass p = {scale, flip, flip_extent, 0};
    for (int i = 0; i < n; ++i) y7t_tta_descale_deflip(xywh + (size_t)i * 4, p);
}

// the taps of one axis: i0, i1 (n ints each), l0, l1 (n floats each)
void hs_tta_taps(int in, int out, int* i0, int* i1, float* l0, float* l1) {
    for (int d = 0; d < out; ++d) {
        const Y7TTtaTap t = y7t_tta_tap(d, in, out);
        i0[d] = t.i0; i1[d] = t.i1; l0[d] = t.l0; l1[d] = t.l1;
    }
}
// rows [0, n) of a pass -> their rows in the concatenation
void hs_tta_rows(int n, int row_base, int* out) {
    const Y7TTtaPass p = {1.f, 0, 0.f, row_base};
    for (int i = 0; i < n; ++i) out[i] = y7t_tta_row(p, i);
}
float hs_tta_pad(void) { return Y7T_TTA_PAD; }
}
