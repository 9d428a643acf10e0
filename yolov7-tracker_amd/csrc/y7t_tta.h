// y7t_tta.h -- test-time augmentation (Model.forward(x, augment=True) of the reference, models/yolo.py:301-317, with scale_img of utils/torch_utils.py:247-257),
// the per-element arithmetic stated once for the device kernels (y7t_tta.hip) and for the CPU build of the same bodies (tests/_hostsim/tta.py).
//   scale + layout : pixel (y, x) of the padded, scaled, flipped image, straight from the frame the caller holds: x.flip(f) -> F.interpolate(size = (hs, ws),
//                    mode = 'bilinear', align_corners = False) -> F.pad(right, bottom, 0.447).  The flip is applied to the source INDEX, before the resample.
//   de-scale/flip  : y[..., :4] /= s; y[..., 0] = W - y[..., 0] (flip 3) or y[..., 1] = H - y[..., 1] (flip 2) on a decoded xywh row.
// THE ORDER, all float32, two roundings per multiply-add (`#pragma clang fp contract(off)` in every body, whatever the including file is built with):
//   scale = (float)in / (float)out;  src = scale * ((float)dst + 0.5f) - 0.5f, clamped at 0;  i0 = (int)src;  i1 = min(i0 + 1, in - 1);  l1 = src - (float)i0;  l0 = 1 - l1
//   out = lh0 * (lw0 * p00 + lw1 * p01) + lh1 * (lw0 * p10 + lw1 * p11)
// which is the geometry and the weights of torch's upsample_bilinear2d; bit equality with torch's own kernel is not claimed (its association and contraction belong to
// the torch build).  hs == H (or ws == W) needs no special case: scale = 1, src = dst, l1 = 0, and 1 * p + 0 * q is p.
// A uint8 BGR frame is first converted exactly as k_input_layout<true> (y7t_post.hip) converts it -- (float)u8 / 255.0f, channel 2 - ch -- and then treated as the float image.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define Y7T_TTA_HD __host__ __device__ inline
#else
#define Y7T_TTA_HD inline
#endif

#define Y7T_TTA_PAD 0.447f      // utils/torch_utils.py:257 ("imagenet mean")
enum { Y7T_TTA_FLIP_NONE = 0, Y7T_TTA_FLIP_UD = 2, Y7T_TTA_FLIP_LR = 3 };      // the reference's dims: x.flip(2) / x.flip(3) of (B, 3, H, W)

// what one launch resamples: the source frame (H x W), the flip, the resampled size (hs x ws) inside the padded image (Hp x Wp)
struct Y7TTtaGeom { int H, W, flip, hs, ws, Hp, Wp; };

struct Y7TTtaTap { int i0, i1; float l0, l1; };
// output index `dst` of `out` samples -> the two source taps among `in` and their weights
Y7T_TTA_HD Y7TTtaTap y7t_tta_tap(int dst, int in, int out) {
#pragma clang fp contract(off)
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    Y7TTtaTap t;
    t.i0 = (int)src;
    if (t.i0 > in - 1) t.i0 = in - 1;      // (never taken for dst < out: src < in - 0.5; it keeps every read inside the frame whatever the caller passes)
    t.i1 = t.i0 + 1 < in - 1 ? t.i0 + 1 : in - 1;
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

// channel ch (RGB order) of source pixel (y, x) of image b as the float image holds it
Y7T_TTA_HD float y7t_tta_src(const void* img, int is_u8, int b, int ch, int H, int W, int y, int x) {
#pragma clang fp contract(off)
    if (is_u8) return (float)((const uint8_t*)img)[(((size_t)b * H + y) * W + x) * 3 + (2 - ch)] / 255.0f;      // BGR -> RGB, /255
    return ((const float*)img)[(((size_t)b * 3 + ch) * H + y) * W + x];
}

// the three channels of pixel (y, x) of the padded image of frame b: the pad value right of ws and below hs, the bilinear sample of the flipped frame elsewhere
Y7T_TTA_HD void y7t_tta_rgb(const void* img, int is_u8, int b, const Y7TTtaGeom& g, int y, int x, float* rgb) {
#pragma clang fp contract(off)
    if (y >= g.hs || x >= g.ws) { rgb[0] = rgb[1] = rgb[2] = Y7T_TTA_PAD; return; }
    const Y7TTtaTap ty = y7t_tta_tap(y, g.H, g.hs), tx = y7t_tta_tap(x, g.W, g.ws);
    // x.flip(f) first: tap i of the flipped frame is pixel (extent - 1 - i) of the frame
    const int y0 = g.flip == Y7T_TTA_FLIP_UD ? g.H - 1 - ty.i0 : ty.i0, y1 = g.flip == Y7T_TTA_FLIP_UD ? g.H - 1 - ty.i1 : ty.i1;
    const int x0 = g.flip == Y7T_TTA_FLIP_LR ? g.W - 1 - tx.i0 : tx.i0, x1 = g.flip == Y7T_TTA_FLIP_LR ? g.W - 1 - tx.i1 : tx.i1;
    for (int ch = 0; ch < 3; ++ch) {
        const float p00 = y7t_tta_src(img, is_u8, b, ch, g.H, g.W, y0, x0), p01 = y7t_tta_src(img, is_u8, b, ch, g.H, g.W, y0, x1);
        const float p10 = y7t_tta_src(img, is_u8, b, ch, g.H, g.W, y1, x0), p11 = y7t_tta_src(img, is_u8, b, ch, g.H, g.W, y1, x1);
        rgb[ch] = ty.l0 * (tx.l0 * p00 + tx.l1 * p01) + ty.l1 * (tx.l0 * p10 + tx.l1 * p11);
    }
}

// the `ldout` (8 or 16) channels of output pixel (yo, xo) of the network's NHWC input, as floats (the kernel rounds each once to fp16): with ReOrg (models/common.py:48-53)
// c = g * 3 + ch, g = (row parity) + 2 * (column parity) of the 2 x 2 block, 12 + 4 zeros; without, 3 + 5 zeros.  The layout of k_input_layout (y7t_post.hip).
Y7T_TTA_HD void y7t_tta_layout_px(const void* img, int is_u8, int b, const Y7TTtaGeom& g, int reorg, int yo, int xo, float* v /*[16]*/) {
    for (int c = 0; c < 16; ++c) v[c] = 0.f;
    const int ng = reorg ? 4 : 1;
#if defined(__clang__)
#pragma unroll      // (constant trip count, the tail guarded: every index into v is a constant and v stays in registers)
#endif
    for (int q = 0; q < 4; ++q) {
        if (q >= ng) break;
        const int y = reorg ? 2 * yo + (q & 1) : yo, x = reorg ? 2 * xo + (q >> 1) : xo;
        y7t_tta_rgb(img, is_u8, b, g, y, x, v + q * 3);
    }
}

// one pass's transform of a decoded row: its scale, its flip, the FIRST pass's extent along the flipped axis, and where its rows start in the concatenation
struct Y7TTtaPass { float scale; int flip; float flip_extent; int row_base; };

// yi[..., :4] /= si, then the de-flip (models/yolo.py:311-315), on c = {x, y, w, h}: a true float32 division by (float)si, as the reference's CPU path computes it
Y7T_TTA_HD void y7t_tta_descale_deflip(float* c, const Y7TTtaPass& p) {
#pragma clang fp contract(off)
    for (int k = 0; k < 4; ++k) c[k] = c[k] / p.scale;
    if (p.flip == Y7T_TTA_FLIP_LR) c[0] = p.flip_extent - c[0];
    else if (p.flip == Y7T_TTA_FLIP_UD) c[1] = p.flip_extent - c[1];
}

// a row of this pass in the concatenation torch.cat(y, 1): the rows of the passes before it come first (what cidx holds for an augmented candidate)
Y7T_TTA_HD int y7t_tta_row(const Y7TTtaPass& p, int row_in_pass) { return p.row_base + row_in_pass; }
