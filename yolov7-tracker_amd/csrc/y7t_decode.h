// y7t_decode.h -- the Detect decode of ONE anchor row (models/yolo.py:49-56) and the candidate tests of non_max_suppression (utils/general.py:629-662), stated once
// for the three kernels that run it: k_decode_filter and k_decode_filter_ml (y7t_post.hip) and the EPI == 1 epilogue of k_conv_igemm (y7t_conv.hip).  Their candidates
// are compared bit for bit (tests/test_conv_forms_gpu.py), so every body carries `#pragma clang fp contract(off)`: two roundings per multiply-add, whatever
// -ffp-contract the including file is built with (y7t_conv.hip: fast-honor-pragmas).  What the kernels keep to themselves is how they reserve candidate slots.
// `v`: the row's `no` fp32 logits -- x, y, w, h, objectness, classes.
#pragma once
#include "y7t_det.h"
#include "y7t_tta.h"

__device__ __forceinline__ float y7t_sigmoid(float x) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-x));
}

// xc = prediction[..., 4] > conf_thres, and the same test on a class confidence: strictly above (a NaN does not pass)
__device__ __forceinline__ bool y7t_conf_passes(float conf, float conf_thres) {
#pragma clang fp contract(off)
    return conf > conf_thres;
}

// x[:, 5:] *= x[:, 4:5], one class of it
__device__ __forceinline__ float y7t_class_conf(const float* v, int c, float obj) {
#pragma clang fp contract(off)
    return y7t_sigmoid(v[5 + c]) * obj;
}

// conf, j = x[:, 5:].max(1): the first class of the largest confidence
struct Y7TBest { float conf; int cls; };
__device__ __forceinline__ Y7TBest y7t_best_class(const float* v, int nc, float obj) {
#pragma clang fp contract(off)
    Y7TBest best = {-1.f, 0};
    for (int c = 0; c < nc; ++c) {
        const float s = y7t_class_conf(v, c, obj);
        if (s > best.conf) { best.conf = s; best.cls = c; }
    }
    return best;
}

// the row's box at cell (x, y), anchor `an` of level L: centre and size (what Detect returns) ...
__device__ __forceinline__ void y7t_decode_xywh(const float* v, int x, int y, int an, const Y7TLevel& L, float* c) {
#pragma clang fp contract(off)
    const float sx = y7t_sigmoid(v[0]), sy = y7t_sigmoid(v[1]), sw = y7t_sigmoid(v[2]), sh = y7t_sigmoid(v[3]);
    c[0] = (sx * 2.f - 0.5f + (float)x) * L.stride; c[1] = (sy * 2.f - 0.5f + (float)y) * L.stride;
    c[2] = (sw * 2.f) * (sw * 2.f) * L.aw[an]; c[3] = (sh * 2.f) * (sh * 2.f) * L.ah[an];
}
// ... and the corners non_max_suppression works on (xywh2xyxy).  Two steps, so that a kernel may reserve the slot between them and write the corners in place.
__device__ __forceinline__ void y7t_xywh2xyxy(const float* c, float* box) {
#pragma clang fp contract(off)
    box[0] = c[0] - c[2] / 2; box[1] = c[1] - c[3] / 2; box[2] = c[0] + c[2] / 2; box[3] = c[1] + c[3] / 2;
}
__device__ __forceinline__ void y7t_decode_box(const float* v, int x, int y, int an, const Y7TLevel& L, float* box) {
    float c[4];
    y7t_decode_xywh(v, x, y, an, L, c);
    y7t_xywh2xyxy(c, box);
}
// ... of one pass of augmented inference (models/yolo.py:311-315): the row's xywh brought back to the first pass's coordinates (y7t_tta.h) before the corners
__device__ __forceinline__ void y7t_decode_box_tta(const float* v, int x, int y, int an, const Y7TLevel& L, const Y7TTtaPass& pass, float* box) {
    float c[4];
    y7t_decode_xywh(v, x, y, an, L, c);
    y7t_tta_descale_deflip(c, pass);
    y7t_xywh2xyxy(c, box);
}

// the row's index in the reference's (B, A, no) ordering: what cidx holds
__device__ __forceinline__ int y7t_anchor_row(const Y7TLevel& L, int an, int y, int x) { return L.row0 + (an * L.ny + y) * L.nx + x; }
