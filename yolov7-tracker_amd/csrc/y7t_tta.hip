// y7t_tta.hip -- test-time augmentation around the plain forward (models/yolo.py:301-317): the two kernels a pass needs beside the launch list
//   * k_tta_scale_layout: x.flip + scale_img (utils/torch_utils.py:247-257) + the NHWC fp16 input layout (ReOrg where the plan has it) in one launch, straight into
//     buffer 0 of the pass plan's arena -- no intermediate float image
//   * k_decode_append: k_decode_filter (y7t_post.hip) with the pass's de-scale / de-flip between the decode and the corners, appending to the candidate arrays the
//     passes before it filled (row index = row_base + the row inside the pass)
// The per-element arithmetic is y7t_tta.h / y7t_decode.h, shared with the CPU build the tests compare these kernels with; this file is the walk over the pixels, the rows and the slots.
#include "y7t_common.h"
#include <string.h>
#include "y7t_decode.h"

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(8))) _Float16 half8;

static_assert(sizeof(y7t_tta_pass) == sizeof(Y7TTtaPass) && sizeof(y7t_tta_pass) == 16, "y7t_tta_pass (include/y7t.h) is Y7TTtaPass (y7t_tta.h), member for member");

// One thread per output pixel of the network's input (a 2 x 2 block of the padded image with ReOrg), x fastest: the lanes of a wave write consecutive 16- or 32-byte
// pieces (one contiguous run) and read source pixels whose x grows with the lane by in / out (times two with ReOrg) -- under 3.1 for every ratio >= 0.65 -- so the
// wave's four taps of a channel fall into the same few consecutive cache lines of one or two source rows.  The flip mirrors the index (the lanes then walk the row
// downwards: the same lines).  A bandwidth kernel: at most four source pixels per output element and no reuse beyond what the caches give for nothing.
__global__ void __launch_bounds__(256) k_tta_scale_layout(const void* __restrict__ img, int is_u8, int B, const Y7TTtaGeom g, int reorg, half_t* __restrict__ out,
                                                          int ldout) {
    const int Ho = reorg ? g.Hp / 2 : g.Hp, Wo = reorg ? g.Wp / 2 : g.Wp;
    const long long tot = (long long)B * Ho * Wo;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < tot; p += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(p / ((long long)Ho * Wo));
        const int rem = (int)(p - (long long)b * Ho * Wo);
        const int yo = rem / Wo, xo = rem - yo * Wo;
        float f[16];
        y7t_tta_layout_px(img, is_u8, b, g, reorg, yo, xo, f);
        half_t v[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] = (half_t)f[c];
        half_t* o = out + (size_t)p * ldout;
        for (int c = 0; c < ldout; c += 8) *(half8*)(o + c) = *(half8*)(v + c);
    }
}

extern "C" int y7t_tta_scale_layout(const void* img, int is_u8, int B, int H, int W, int flip, int hs, int ws, int Hp, int Wp, int reorg, void* out_f16,
                                    int ldout, y7t_stream stream) {
    Y7T_ARG_CHECK(img && out_f16 && B > 0 && H > 0 && W > 0);
    Y7T_ARG_CHECK(flip == Y7T_TTA_FLIP_NONE || flip == Y7T_TTA_FLIP_UD || flip == Y7T_TTA_FLIP_LR);
    Y7T_ARG_CHECK(hs > 0 && ws > 0 && hs <= Hp && ws <= Wp);
    Y7T_ARG_CHECK(ldout == 8 || ldout == 16);
    Y7T_ARG_CHECK(reorg ? (ldout == 16 && Hp % 2 == 0 && Wp % 2 == 0) : 1);
    Y7T_ARG_CHECK((long long)B * Hp * Wp * ldout * 2 < (1ll << 31));      // (one launch: the layout tensor stays below 2 GiB, like every single-launch op of a plan)
    const Y7TTtaGeom g = {H, W, flip, hs, ws, Hp, Wp};
    const long long tot = (long long)B * (reorg ? Hp / 2 : Hp) * (reorg ? Wp / 2 : Wp);
    int blocks = (int)((tot + 255) / 256); if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_tta_scale_layout, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, is_u8 != 0, B, g, reorg != 0, (half_t*)out_f16, ldout);
    Y7T_LAUNCH_CHECK();
    y7t_note_kernel("tta_scale_layout<%s>", is_u8 ? "u8" : "f32");
    return 0;
}

// ------------------------------------------------------------------------------------------------ decode + filter, appending
struct AppendArgs {
    const float* p;       // head conv output of this level, NHWC fp32: [B][ny][nx][na*no]
    Y7TLevel g;
    int na, no, B;
    Y7TCand c;
    Y7TTtaPass pass;
};

// k_decode_filter's walk and slot reservation (past cap the count grows and nothing is written); the box goes through the pass's transform and the row index starts at
// the pass's row_base.  The counters are whatever the passes before left: the launcher zeroes them for the first pass only.
__global__ void __launch_bounds__(256) k_decode_append(const AppendArgs a) {
    const Y7TLevel& L = a.g;
    const int per_img = a.na * L.ny * L.nx;
    const long long tot = (long long)a.B * per_img;
    const int nc = a.no - 5;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < tot; t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / per_img), r = (int)(t - (long long)b * per_img);
        const int x = r % L.nx, an = (r / L.nx) % a.na, y = r / (L.nx * a.na);      // x fastest, then anchor, then y: neighbouring threads read neighbouring NHWC rows
        const float* p = a.p + ((((size_t)b * L.ny + y) * L.nx + x) * a.na + an) * a.no;
        const float obj = y7t_sigmoid(p[4]);
        if (!y7t_conf_passes(obj, a.c.conf_thres)) continue;
        const Y7TBest best = y7t_best_class(p, nc, obj);
        if (!y7t_conf_passes(best.conf, a.c.conf_thres)) continue;
        const int slot = atomicAdd(a.c.count + b, 1);
        if (slot >= a.c.cap) continue;
        y7t_decode_box_tta(p, x, y, an, L, a.pass, a.c.cbox + ((size_t)b * a.c.cap + slot) * 4);
        a.c.cscore[(size_t)b * a.c.cap + slot] = best.conf;
        a.c.ccls[(size_t)b * a.c.cap + slot] = (float)best.cls;
        a.c.cidx[(size_t)b * a.c.cap + slot] = y7t_tta_row(a.pass, y7t_anchor_row(L, an, y, x));
    }
}

extern "C" int y7t_det_decode_append(const float* const* head, const int* ny, const int* nx, const float* strides, const float* anchors, int nl, int na, int no,
                                     int B, float conf_thres, int cap, int max_nms, int multi_label, const y7t_tta_pass* pass, int first_pass, void* workspace,
                                     size_t workspace_bytes, y7t_stream stream) {
    Y7T_ARG_CHECK(head && ny && nx && strides && anchors && pass && workspace);
    Y7T_ARG_CHECK(nl >= 1 && nl <= 4 && na >= 1 && na <= 3 && no >= 6 && B >= 1 && cap >= 64 && max_nms >= 1);
    Y7T_ARG_CHECK(conf_thres >= 0.0f);      // (every candidate score is positive, which the rank sort's bit-pattern keys rely on)
    Y7T_ARG_CHECK(pass->scale > 0.0f && pass->row_base >= 0);
    Y7T_ARG_CHECK(pass->flip == Y7T_TTA_FLIP_NONE || pass->flip == Y7T_TTA_FLIP_UD || pass->flip == Y7T_TTA_FLIP_LR);
    for (int l = 0; l < nl; ++l) Y7T_ARG_CHECK(head[l] && ny[l] > 0 && nx[l] > 0);
    if (multi_label && no > 6) {
        y7t_set_error("decode_append: the multi_label form of the appending decode is not built (one candidate per row, its best class)");
        return Y7T_E_STATE;
    }
    const hipStream_t s = (hipStream_t)stream;
    const Y7TPostWs w = y7t_post_ws(workspace, B, cap, max_nms);
    if (w.total > workspace_bytes) { y7t_set_error("decode_append: workspace too small (%zu < %zu)", workspace_bytes, w.total); return Y7T_E_ARG; }
    if (first_pass) { if (int rc = y7t_zero_counters(w.cand.count, B, s)) return rc; }
    AppendArgs a;
    memset(&a, 0, sizeof(a));
    a.na = na; a.no = no; a.B = B; a.c = w.cand; a.c.conf_thres = conf_thres;
    a.pass.scale = pass->scale; a.pass.flip = pass->flip; a.pass.flip_extent = pass->flip_extent; a.pass.row_base = pass->row_base;
    for (int l = 0; l < nl; ++l) {
        a.p = head[l];
        a.g = y7t_level(l, na, ny, nx, strides, anchors);
        const long long tot = (long long)B * na * ny[l] * nx[l];
        int blocks = (int)((tot + 255) / 256); if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_decode_append, dim3(blocks), dim3(256), 0, s, a);
        Y7T_LAUNCH_CHECK();
    }
    y7t_note_kernel("decode_append");
    return 0;
}
