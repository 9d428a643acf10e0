// y7t_det.h -- internal types shared by the detector translation units (conv, pooling, post-process, plan executor)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { Y7T_ACT_NONE = 0, Y7T_ACT_SILU = 1, Y7T_ACT_LEAKY = 2 };

// One Detect level's geometry (the arithmetic on it: y7t_decode.h; y7t_level fills it)
struct Y7TLevel {
    float stride, aw[3], ah[3];   // models/yolo.py:52-53: xy = (s*2 - 0.5 + grid) * stride; wh = (s*2)^2 * anchor_grid
    int ny, nx, row0;             // row0: first row of this level in the reference's (B, A, no) ordering
};
// level l of a head with `na` anchors per cell: row0 is the sum over the finer levels (models/yolo.py:57 cat order); anchors: [nl][na][2] in pixels
Y7TLevel y7t_level(int l, int na, const int* ny, const int* nx, const float* stride, const float* anchors);

// The candidate arrays: the head of a postprocess workspace (y7t_post_ws), written by the decode pass or by the fused Detect epilogues.  (Member order, here and in
// Y7TLevel: the bytes of Y7TDecode inside Y7TConvArgs stay where the measured conv kernels' argument loads expect them, profiles/post_decode_refactor_isa.txt.)
struct Y7TCand {
    float conf_thres;             // what a decode pass admits (y7t_post_ws leaves it 0: the pass's caller sets it)
    int cap;                      // candidate capacity per image
    float *cbox, *cscore, *ccls;  // [B][cap][4] xyxy, [B][cap], [B][cap]
    int *cidx, *count;            // [B][cap] row index (tie-break / parity checks), [B] candidates found (may exceed cap -> overflow)
};

// Detect decode fused into the 1x1 conv's epilogue (y7t_det_forward_fused): the level + where the candidates go
struct Y7TDecode {
    Y7TLevel lv;
    int na, no;
    Y7TCand c;
};

struct Y7TConvArgs {
    const _Float16* in;  // NHWC fp16 buffer holding the input slice
    int ldin, cin_off;   // channels of that buffer, first channel of the slice
    int B, H, W, Cin;    // input batch / spatial size / channels of the slice (multiple of 8)
    const _Float16* w;   // packed weights [Cout_pad][K_pad], k = (kh*KW + kw)*Cin + ci
    const float* bias;   // [Cout_pad]
    void* out;           // NHWC buffer (fp16, or fp32 when out_f32)
    int ldout, cout_off, out_f32;
    int Ho, Wo, Cout, Cout_pad;
    int KH, KW, stride, pad;
    int K, K_pad;        // K = KH*KW*Cin, K_pad = round_up(K, 64)
    int M;               // B*Ho*Wo
    int act;
    const _Float16* zeros;  // unused (kept for ABI stability of y7t_conv2d_nhwc_f16)
    unsigned in_bytes, w_bytes;
    int xcd_swizzle, tile_order;
    int splitk, ksteps, allow_splitk;   // split-K: workgroups per output tile, K-steps per split
    float* partial;                     // fp32 slabs [splitk][M][Cout_pad]
    float* splitk_ws;                   // caller's split-K workspace of Y7T_SPLITK_WS_BYTES (a detector owns one, so detectors on different streams
                                        // never share slabs), or null: one process-wide workspace (the single-layer entry point; one stream at a time)
    int korder;        // a y7t_weight_layout (include/y7t.h); conv_dispatch turns the two _N64 layouts into their 128-row siblings + panel64
    int panel64;       // 64-row weight panels although Cout_pad % 128 == 0 (small maps, where 128-row panels would leave most CUs without a workgroup)
    int force_patch;   // tests: run an eligible 3x3/s1 layer on k_conv3x3_patch whatever its tile efficiency
    int no_patch;      // host-side: keep this launch on the generic implicit-GEMM kernel
    int ablate;   // debug: bit0 skip DMA loads, bit1 skip MFMAs, bit2 skip the whole compute phase  // extents for the buffer descriptors (filled by y7t_conv_launch)
    int epi;      // 1: Detect decode + candidate filter instead of the output store (1x1 convs, dec below)
    Y7TDecode dec;
    // upsample-on-read (1x1 convs): channels [up_c0, up_c0 + up_C) of the input come from `in2` (H/2 x W/2, ldin2 channels, slice at cin2_off)
    const _Float16* in2;
    int ldin2, cin2_off, up_c0, up_C;
    unsigned in2_bytes;
    // dynamic tile scheduling of the persistent kernels (y7t_conv_ws.hip, y7t_conv_ws128.hip): Y7T_TILE_CTR_INTS ints, zero between launches -- [0 .. 3] chunks handed
    // out (one counter per output-channel tile of the launch), [Y7T_TILE_CTR_DONE] workgroups that have left (the last one resets them all).  One set per op of a
    // detector's plan (y7t_detector.hip); null = static partition (the single-layer entry point).
    int* tile_ctr;
};
#define Y7T_TILE_CTR_DONE 4
#define Y7T_TILE_CTR_INTS 8

#define Y7T_SPLITK_WS_BYTES (128ull << 20)
int y7t_conv_launch(const Y7TConvArgs& a, hipStream_t s);

// fused uint8 frame -> (letterbox) -> layout -> stem conv (y7t_stem.hip)
int y7t_stem_u8_launch(const void* frames_u8, int B, int H0, int W0, int H, int W, int new_h, int new_w, int top, int left, const _Float16* w, int K_pad,
                       const float* bias, _Float16* out, int ldout, int cout_off, int act, hipStream_t s);

int y7t_upsample_launch(const _Float16* in, int ldin, int cin_off, int B, int H, int W, int C, _Float16* out, int ldout, int cout_off, hipStream_t s);
int y7t_add_launch(const _Float16* a, int lda, int a_off, const _Float16* b, int ldb, int b_off, int B, int H, int W, int C, _Float16* out, int ldout, int cout_off,
                   hipStream_t s);   // a, b, out: buffer bases
int y7t_spp3_try(const _Float16* in, int ldin, int cin_off, int B, int H, int W, int C, _Float16* out, int ldout, int cout_off, hipStream_t s);   // 0 done, 1 not applicable
int y7t_maxpool_launch(const _Float16* in, int ldin, int cin_off, int B, int H, int W, int C, int k, int st, int pd, _Float16* out, int ldout,
                       int cout_off, hipStream_t s);

// decode + NMS chain (y7t_post.hip)
struct Y7TPostArgs {
    const float* head[4];   // per level NHWC fp32 [B][ny][nx][na*no]
    int predecoded;         // 1: the candidate arrays of `ws` are already filled (fused Detect epilogue): skip the decode pass
    int ny[4], nx[4];
    float stride[4];
    float anchors[24];      // [nl][na][2] in pixels
    int nl, na, no, B;
    float conf_thres, iou_thres;
    int max_det, max_nms, cap;
    const float* letterbox_dev;  // [B][5] gain, padw, padh, H0, W0 (device)
    float* dets;            // [B][max_det][6]
    int* ndets;             // [B]
    int* keep_idx;          // [B][max_det] candidate slot of each kept detection
    int* count_out;         // [B] number of candidates found (> cap means overflow) or null
    void* ws; size_t ws_bytes;
    // y7t_nms_opts (include/y7t.h); all zero: the tracking path's chain, launch for launch
    int agnostic;           // class offset 0 (general.py:677)
    int multi_label;        // one candidate per (row, class) above conf_thres (general.py:654-656); decode pass only, no > 6
    int filter_classes;     // keep the candidates whose class has its bit in class_mask (general.py:662-663)
    uint32_t class_mask[8]; // Y7T_NMS_MASK_WORDS: bit c % 32 of word c / 32 = class c
};
// THE layout of a postprocess workspace: every array 256-byte aligned, in this order.  `total` is what a workspace needs (also on a null base: nothing is
// dereferenced); the candidate arrays come first (the fused Detect epilogues fill them; Detector.candidate_arrays of detector/model.py restates their offsets)
struct Y7TPostWs {
    Y7TCand cand;
    int* nsorted;           // [B]
    float* sbox;            // [B][mcap][4] class-offset boxes in rank order; mcap = min(cap, max_nms): NMS runs on the top max_nms candidates only (general.py:664-665)
    int* sorder;            // [B][mcap] candidate slot of each rank
    float* lb;              // [B][5] letterbox parameters
    int mcap;
    size_t total;
};
Y7TPostWs y7t_post_ws(void* base, int B, int cap, int max_nms);
// Zero the B candidate counters of a workspace on `s`: a KERNEL, not hipMemsetAsync.  Every chain that fills the candidate arrays starts with this, and the chains are
// captured into hipGraphs (Detector.capture).  As a memset node the zeroing did not survive replays: the second replay of a two-node graph (memset, Detect conv) wrote a
// repeating 16-byte pattern of stale words over the counters instead of zeros (tests/graph_replay_gpu_cases.py::test_fused_detect_epilogue_replayed; negative counters
// then index the candidate arrays out of bounds).  A kernel node carries its arguments by value and replays as recorded.
int y7t_zero_counters(int* count, int B, hipStream_t s);
int y7t_post_run(const Y7TPostArgs& a, hipStream_t s);
