// y7t_reid_osnet.h -- the arithmetic of the general OSNet path (csrc/y7t_reid_osnet.hip; DESIGN.md section 4 "OSNet family"), stated once: the strip rule of the
// LightConv3x3 level kernel, the slot layout of the branch buffer, the instance-norm normaliser, the gate's sigmoid and the four-branch sum.  Plain C++ that the
// host launcher and the kernels share; tests/osnet_f16_ref.py restates it in numpy.
//
// Storage: activations fp16 NHWC with the channel count padded to a multiple of 16; every pad channel is exactly zero after every op (zero weights, zero bias,
// zero gamma / beta).  Every dense product is v_mfma_f32_16x16x16_f16 with A = weights in tracker/reid.py::_frags order, B = 16 pixels x 16 channels, fp32 accumulate
// starting from the bias.
#ifndef Y7T_REID_OSNET_H
#define Y7T_REID_OSNET_H
#include <stdint.h>
#include <math.h>

#ifdef __HIPCC__
#define Y7T_OSNET_HD __host__ __device__ inline
#else
#define Y7T_OSNET_HD inline
#endif

// LDS of the level kernel: (S + 2) rows x (W + 2) pixels x midp halves for the 1x1's output, + Y7T_OSNET_LDS_STATIC bytes of reduction scratch; 64 KiB per workgroup
#define Y7T_OSNET_LDS_BUDGET 61440
#define Y7T_OSNET_LDS_STATIC 4096
#define Y7T_OSNET_IN_EPS 1e-5f

// rows of a strip: the most whose haloed 1x1 output fits the LDS budget, at most H; override > 0 (tests) forces it.  0: not even one row fits
Y7T_OSNET_HD int y7t_osnet_strip_rows(int H, int W, int midp, int override_rows) {
    const long long row_bytes = (long long)(W + 2) * midp * 2;
    long long s = Y7T_OSNET_LDS_BUDGET / row_bytes - 2;
    if (s < 1) return 0;
    if (override_rows > 0 && override_rows < s) s = override_rows;
    return (int)(s < H ? s : H);
}
Y7T_OSNET_HD int y7t_osnet_strips(int H, int S) { return (H + S - 1) / S; }

// the branch buffer of an OSBlock, per crop: level 0 holds branches a b c d (4 slots), level 1 b c d, level 2 c d, level 3 d -- 10 slots of H W midp halves.
// Level j, slot s is branch j + s after its (j + 1)-th LightConv3x3; it reads level j - 1, slot s + 1.  Branch b is finished in slot 0 of level b
#define Y7T_OSNET_SLOTS 10
Y7T_OSNET_HD int y7t_osnet_level_slot(int level) { return level * 4 - level * (level - 1) / 2; }       // 0, 4, 7, 9

// InstanceNorm2d(affine=True, eps=1e-5): biased variance, a true division and square root
Y7T_OSNET_HD float y7t_osnet_in_scale(float var) { return 1.0f / sqrtf(var + Y7T_OSNET_IN_EPS); }
Y7T_OSNET_HD float y7t_osnet_in_apply(float x, float mean, float inv, float gamma, float beta, int relu) {
    const float y = (x - mean) * inv * gamma + beta;
    return relu ? fmaxf(y, 0.f) : y;
}

Y7T_OSNET_HD float y7t_osnet_sigmoid(float a) { return 1.0f / (1.0f + expf(-a)); }
// x2 = sum_b gate_b * x2_b, in branch order
Y7T_OSNET_HD float y7t_osnet_gate_sum(const float g[4], const float x[4]) { return ((g[0] * x[0] + g[1] * x[1]) + g[2] * x[2]) + g[3] * x[3]; }

// pw epilogue: `relu` field bit 0 = ReLU, `k` field = residual mode
enum { Y7T_OSNET_RES_NONE = 0, Y7T_OSNET_RES_ADD = 1 /* + aux (identity) */, Y7T_OSNET_RES_GEMM = 2 /* second GEMM over aux with the weights at w2_off */ };

#ifdef __HIPCC__
struct y7t_reid_op;
// one op of the Y7T_REID_H_OS_* / Y7T_REID_INSTNORM types; pointers already resolved.  0 or a Y7T_E_* code
int y7t_reid_osnet_check(const y7t_reid_op& op);
int y7t_reid_osnet_launch(const y7t_reid_op& op, const float* in, float* out, float* aux, const float* wblob, int N, int max_n, hipStream_t s);
#endif
#endif
