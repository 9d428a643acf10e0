// y7t_reid_osnet.hip -- the general OSNet path: every width (x0_25 .. x1_0), the IBN variant, any crop size with H and W multiples of 16, layer by layer with
// fp16 NHWC activations in HBM, fp32 accumulation and every dense product on v_mfma_f32_16x16x16_f16 (DESIGN.md section 4 "OSNet family").
//
// Restates tracker/reid_models/OSNet.py:28-157 (ConvLayer, Conv1x1, Conv1x1Linear, LightConv3x3), :162-220 (ChannelGate), :223-276 (OSBlock, with IN) and :413-431
// (forward in eval mode) with BatchNorm folded on the host (tracker/reid.py::lower_osnet_f16).  Opt-in (ReIDExtractor(half=True)): the one-workgroup-per-crop kernel of
// y7t_reid_fused.hip stays the default for x0_25 at 128 x 64, the fp32 op list of y7t_reid.hip the default elsewhere and the exact path.
//
// MFMA operand roles (the fused kernel's): A = 16 output channels x 16 k of the weights, packed on the host in lane order (reid.py::_frags), B = 16 pixels x 16
// channels -- lane l holds pixel l % 16, channels 4 (l / 16) .. + 3, one 8-byte load --, D = lane l holds pixel l % 16, output channels 4 (l / 16) .. + 3: one
// 8-byte fp16 store into the NHWC map.  No atomics; every reduction is a fixed tree or a fixed serial order, so bits repeat from call to call and a crop's result
// depends on nothing but the crop.
#include "y7t_common.h"
#include "y7t_conv_common.h"
#include "y7t_reid_osnet.h"

typedef __attribute__((ext_vector_type(4))) float floatx4;

enum { R_H_OS_STEM = 15, R_H_OS_PW = 16, R_H_OS_LIGHT = 17, R_H_OS_GATESUM = 18, R_H_OS_INSTNORM = 19, R_H_OS_AVGPOOL = 20, R_H_OS_GAPFC = 21, R_INSTNORM = 22 };

namespace {

__device__ __forceinline__ floatx4 mfma16(half4 a, half4 b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ half4 to_half4(floatx4 v) {
    half4 h; h[0] = (_Float16)v[0]; h[1] = (_Float16)v[1]; h[2] = (_Float16)v[2]; h[3] = (_Float16)v[3];
    return h;
}

// ---- stem: 7x7 / stride 2 / pad 3 over the fp32 crop k_reid_crop sampled (each pixel rounded to fp16 once, here), 3 -> C0p, + bias, raw fp16 out.
// K-step (kh, half) of k_osnet_x025's stem: k = 4 q + c is input pixel kw = 4 half + q, channel c (c == 3 and kw == 7: zero).  One wave: 16 output pixels x C0p
template <int G>
__global__ void __launch_bounds__(256) k_osnet_stem(const float* __restrict__ in, int H, int W, int Ho, int Wo, long long M, const half4* __restrict__ wfr,
                                                    const float* __restrict__ bias, half_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, p = lane & 15, q = lane >> 4;
    const long long m0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (m0 >= M) return;
    const long long m = m0 + p < M ? m0 + p : M - 1;
    const int xo = (int)(m % Wo), yo = (int)((m / Wo) % Ho);
    const float* img = in + (size_t)(m / ((long long)Wo * Ho)) * H * W * 3;
    floatx4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = *(const floatx4*)(bias + g * 16 + q * 4);
    for (int kh = 0; kh < 7; ++kh) {
        const int iy = yo * 2 - 3 + kh;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kw = 4 * h + q, ix = xo * 2 - 3 + kw;
            half4 b = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
            if (kw < 7 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                const float* px = img + ((size_t)iy * W + ix) * 3;
                b[0] = (half_t)px[0]; b[1] = (half_t)px[1]; b[2] = (half_t)px[2];
            }
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = mfma16(wfr[(g * 14 + kh * 2 + h) * 64 + lane], b, acc[g]);
        }
    }
    if (m0 + p < M) {
#pragma unroll
        for (int g = 0; g < G; ++g) *(half4*)(out + (size_t)m * (G * 16) + g * 16 + q * 4) = to_half4(acc[g]);
    }
}

// ---- pointwise 1x1: out[m][co] = act(bias[co] + sum_k in[m][k] W[co][k] (+ sum_k in2[m][k] W2[co][k]) (+ res[m][co])).  One wave: 16 pixels x 64 output channels
// (blockIdx.y picks the 64); fp16 out, or fp32 (the fc of the tail)
__global__ void __launch_bounds__(256) k_osnet_pw(const half_t* __restrict__ in, int K1, const half_t* __restrict__ in2, int K2, const half4* __restrict__ wfr,
                                                  const half4* __restrict__ wfr2, const float* __restrict__ bias, const half_t* __restrict__ res, long long M, int Cout,
                                                  int relu, half_t* __restrict__ out, float* __restrict__ outf) {
    const int lane = threadIdx.x & 63, p = lane & 15, q = lane >> 4;
    const long long m0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (m0 >= M) return;
    const long long m = m0 + p < M ? m0 + p : M - 1;
    const int G = Cout / 16, g0 = blockIdx.y * 4, NK1 = K1 / 16, NK2 = K2 / 16;
    floatx4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = g0 + j < G ? *(const floatx4*)(bias + (g0 + j) * 16 + q * 4) : floatx4{0.f, 0.f, 0.f, 0.f};
    const half_t* row = in + (size_t)m * K1 + q * 4;
    for (int k = 0; k < NK1; ++k) {
        const half4 b = *(const half4*)(row + k * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g0 + j < G) acc[j] = mfma16(wfr[((size_t)(g0 + j) * NK1 + k) * 64 + lane], b, acc[j]);
    }
    if (in2) {
        const half_t* row2 = in2 + (size_t)m * K2 + q * 4;
        for (int k = 0; k < NK2; ++k) {
            const half4 b = *(const half4*)(row2 + k * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (g0 + j < G) acc[j] = mfma16(wfr2[((size_t)(g0 + j) * NK2 + k) * 64 + lane], b, acc[j]);
        }
    }
    if (m0 + p >= M) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (g0 + j >= G) continue;
        const size_t o = (size_t)m * Cout + (g0 + j) * 16 + q * 4;
        floatx4 v = acc[j];
        if (res) {
            const half4 r = *(const half4*)(res + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (float)r[e];
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (outf) *(floatx4*)(outf + o) = v;
        else *(half4*)(out + o) = to_half4(v);
    }
}

// ---- one LightConv3x3 of every branch that has one at this level.  grid (crop * strips, slot).  The workgroup computes the linear 1x1 of its strip + one halo row
// on each side on MFMA into a zero-haloed fp16 LDS image [(S + 2)][(W + 2)][midp] -- rows and columns outside the map stay zero: the depthwise conv pads the 1x1's
// OUTPUT --, then the depthwise 3x3 + bias + ReLU on the VALU out of LDS (4 channels per thread, 8-byte reads of whole consecutive pixels), fp16 to HBM.  Slot 0 is
// the last LightConv3x3 of its branch: it also writes the strip's per-channel sums of the stored values to part[crop][level][strip][midp]
// per slot parameters at wlev: A fragments (midp^2 halves) | depthwise taps fp32 [9][midp] | bias fp32 [midp]
__global__ void __launch_bounds__(256) k_osnet_light(const half_t* __restrict__ in, long long in_crop_stride, long long in_slot_stride, half_t* __restrict__ out,
                                                     long long out_crop_stride, const float* __restrict__ wlev, int H, int W, int midp, int S, int strips, int level,
                                                     float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    __shared__ float red[Y7T_OSNET_LDS_STATIC / 4];
    half_t* img = (half_t*)lds_raw;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, q = lane >> 4;
    const int n = blockIdx.x / strips, strip = blockIdx.x % strips, slot = blockIdx.y;
    const int r0 = strip * S, rows = min(S, H - r0);                 // output rows r0 .. r0 + rows - 1; LDS row i is map row r0 - 1 + i
    const int HW = H * W, NK = midp / 16, W2 = W + 2;
    const size_t slot_floats = (size_t)midp * midp / 2 + 10 * (size_t)midp;
    const half4* wfr = (const half4*)(wlev + slot * slot_floats);
    const float* dw = wlev + slot * slot_floats + (size_t)midp * midp / 2;
    const float* bias = dw + 9 * midp;
    const half_t* src = in + (size_t)n * in_crop_stride + (size_t)slot * in_slot_stride;
    half_t* dst = out + (size_t)n * out_crop_stride + (size_t)slot * HW * midp;

    const int img_vec = (rows + 2) * W2 * midp / 8;                  // midp % 16 == 0
    for (int i = tid; i < img_vec; i += 256) ((floatx4*)img)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const int ya = max(r0 - 1, 0), yb = min(r0 + rows, H - 1);       // map rows the 1x1 is computed for
    const int npx = (yb - ya + 1) * W, ntile = (npx + 15) / 16;
    for (int t = wave; t < ntile * NK; t += 4) {                     // task: 16 pixels x 16 output channels
        const int tile = t / NK, g = t % NK;
        const int px = min(tile * 16 + p, npx - 1), y = ya + px / W, x = px % W;
        const half_t* row = src + ((size_t)y * W + x) * midp + q * 4;
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < NK; ++k) acc = mfma16(wfr[(g * NK + k) * 64 + lane], *(const half4*)(row + k * 16), acc);
        if (tile * 16 + p < npx) *(half4*)(img + ((size_t)(y - r0 + 1) * W2 + x + 1) * midp + g * 16 + q * 4) = to_half4(acc);
    }
    __syncthreads();
    const int CG = midp / 4, P = 256 / CG, cg = tid % CG, ps = tid / CG;      // thread: channels 4 cg .. + 3 of pixels ps, ps + P, ...
    floatx4 sum = {0.f, 0.f, 0.f, 0.f};
    if (ps < P) {
        floatx4 wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = *(const floatx4*)(dw + k * midp + cg * 4);
        const floatx4 b4 = *(const floatx4*)(bias + cg * 4);
        for (int px = ps; px < rows * W; px += P) {
            const int y = px / W, x = px % W;
            floatx4 acc = b4;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const half4 v = *(const half4*)(img + ((size_t)(y + kh) * W2 + x + kw) * midp + cg * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += (float)v[e] * wt[kh * 3 + kw][e];
                }
            half4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[e] = (half_t)fmaxf(acc[e], 0.f); sum[e] += (float)o[e]; }
            *(half4*)(dst + ((size_t)(r0 + y) * W + x) * midp + cg * 4) = o;
        }
    }
    if (slot != 0) return;                                           // uniform over the workgroup
    if (ps < P) *(floatx4*)(red + (ps * CG + cg) * 4) = sum;         // P * CG <= 256 entries of 4 floats
    __syncthreads();
    if (tid < midp) {
        float s = 0.f;
        for (int k = 0; k < P; ++k) s += red[(k * CG + tid / 4) * 4 + tid % 4];
        part[(((size_t)n * 4 + level) * strips + strip) * midp + tid] = s;
    }
}

// ---- gates and the gated sum: per crop, pooled_b = (sum over strips, in strip order, of branch b's partials) / HW, gate_b = sigmoid(fc2(relu(fc1(pooled_b)))) in
// fp32 (one ChannelGate for the four branches), x2 = sum_b gate_b * x2_b -> fp16.  grid (crop, pixel chunk): every workgroup of a crop recomputes the crop's gates
// (4 (2 midp R) multiply-adds) instead of a launch of their own.  w1 [R][midp], w2 [midp][R]; midp <= 128, R <= 8
__global__ void __launch_bounds__(256) k_osnet_gatesum(const half_t* __restrict__ T, const float* __restrict__ part, int strips, int HW, int midp, int R,
                                                       const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, int chunk_px, half_t* __restrict__ out) {
    __shared__ float pooled[4 * 128];
    __shared__ float hid[4 * 8];
    __shared__ float gate[4 * 128];
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < 4 * midp; i += 256) {
        const int b = i / midp, c = i % midp;
        const float* pp = part + ((size_t)n * 4 + b) * strips * midp + c;
        float s = 0.f;
        for (int k = 0; k < strips; ++k) s += pp[(size_t)k * midp];
        pooled[i] = s / (float)HW;
    }
    __syncthreads();
    if (tid < 4 * R) {
        const int b = tid / R, r = tid % R;
        float a = b1[r];
        for (int c = 0; c < midp; ++c) a += w1[r * midp + c] * pooled[b * midp + c];
        hid[tid] = fmaxf(a, 0.f);
    }
    __syncthreads();
    for (int i = tid; i < 4 * midp; i += 256) {
        const int b = i / midp, c = i % midp;
        float a = b2[c];
        for (int r = 0; r < R; ++r) a += w2[c * R + r] * hid[b * R + r];
        gate[i] = y7t_osnet_sigmoid(a);
    }
    __syncthreads();
    const int CG = midp / 4;
    const size_t crop = (size_t)n * Y7T_OSNET_SLOTS * HW * midp;
    const int px0 = blockIdx.y * chunk_px, px1 = min(px0 + chunk_px, HW);
    for (int i = px0 * CG + tid; i < px1 * CG; i += 256) {
        const int c = (i % CG) * 4;
        half4 v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) v[b] = *(const half4*)(T + crop + ((size_t)y7t_osnet_level_slot(b) * HW) * midp + (size_t)i * 4);
        half4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g[4] = {gate[c + e], gate[midp + c + e], gate[2 * midp + c + e], gate[3 * midp + c + e]};
            const float x[4] = {(float)v[0][e], (float)v[1][e], (float)v[2][e], (float)v[3][e]};
            o[e] = (half_t)y7t_osnet_gate_sum(g, x);
        }
        *(half4*)(out + (size_t)n * HW * midp + (size_t)i * 4) = o;
    }
}

// ---- InstanceNorm2d(affine, eps 1e-5) (+ ReLU) per (crop, channel) over the map: two passes over the STORED tensor in fp32 -- mean, then centred squares (biased
// variance) --, each a per-thread serial sum over pixels tid, tid + 256, ... and a fixed 256-leaf tree.  grid (crop, C / 8).  T = _Float16 (fp16 path) or float
// (the exact op list)
template <typename T> struct alignas(8 * sizeof(T)) Vec8 { T v[8]; };
template <typename T>
__global__ void __launch_bounds__(256) k_osnet_instnorm(const T* __restrict__ in, const T* __restrict__ add, int HW, int C, const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                        T* __restrict__ out) {
    __shared__ float red[256 * 8];
    const int tid = threadIdx.x, c0 = blockIdx.y * 8;
    const T* x = in + (size_t)blockIdx.x * HW * C + c0;
    const T* xa = add ? add + (size_t)blockIdx.x * HW * C + c0 : nullptr;      // the norm of in + add (the exact list's x3 + identity), summed once per read
    T* y = out + (size_t)blockIdx.x * HW * C + c0;
    float mean[8], inv[8], acc[8];
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int i = tid; i < HW; i += 256) {
            Vec8<T> v = *(const Vec8<T>*)(x + (size_t)i * C);
            if (xa) {
                const Vec8<T> a = *(const Vec8<T>*)(xa + (size_t)i * C);
#pragma unroll
                for (int e = 0; e < 8; ++e) v.v[e] = (T)((float)v.v[e] + (float)a.v[e]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (float)v.v[e];
                acc[e] += pass ? (f - mean[e]) * (f - mean[e]) : f;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[tid * 8 + e] = acc[e];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) {
#pragma unroll
                for (int e = 0; e < 8; ++e) red[tid * 8 + e] += red[(tid + w) * 8 + e];
            }
            __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float r = red[e] / (float)HW;
            if (pass) inv[e] = y7t_osnet_in_scale(r); else mean[e] = r;
        }
        __syncthreads();
    }
    float ga[8], be[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ga[e] = gamma[c0 + e]; be[e] = beta[c0 + e]; }
    for (int i = tid; i < HW; i += 256) {
        Vec8<T> v = *(const Vec8<T>*)(x + (size_t)i * C);
        if (xa) {
            const Vec8<T> a = *(const Vec8<T>*)(xa + (size_t)i * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) v.v[e] = (T)((float)v.v[e] + (float)a.v[e]);
        }
        Vec8<T> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[e] = (T)y7t_osnet_in_apply((float)v.v[e], mean[e], inv[e], ga[e], be[e], relu);
        *(Vec8<T>*)(y + (size_t)i * C) = o;
    }
}

// ---- AvgPool2d(2) on fp16 maps: ((a + b) + c) + d in fp32, * 0.25, one rounding
__global__ void __launch_bounds__(256) k_osnet_avgpool2(const half_t* __restrict__ in, int N, int H, int W, int C, half_t* __restrict__ out) {
    const int C8 = C / 8, Ho = H / 2, Wo = W / 2;
    const long long tot = (long long)N * Ho * Wo * C8;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < tot; t += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(t % C8);
        const long long px = t / C8;
        const int xo = (int)(px % Wo), yo = (int)((px / Wo) % Ho), n = (int)(px / ((long long)Wo * Ho));
        const half_t* b = in + (((size_t)n * H + yo * 2) * W + xo * 2) * C + c8 * 8;
        const half8 v00 = *(const half8*)b, v01 = *(const half8*)(b + C), v10 = *(const half8*)(b + (size_t)W * C), v11 = *(const half8*)(b + (size_t)W * C + C);
        half8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)(((((float)v00[e] + (float)v01[e]) + (float)v10[e]) + (float)v11[e]) * 0.25f);
        *(half8*)(out + (size_t)px * C + c8 * 8) = o;
    }
}

// ---- global average pool of an fp16 map -> fp16 (N, C): thread (slot, 8-channel group) sums pixels slot, slot + P, ... serially, the P slots are added in order
__global__ void __launch_bounds__(256) k_osnet_gap(const half_t* __restrict__ in, int HW, int C, half_t* __restrict__ out) {
    __shared__ float red[256 * 8];
    const int tid = threadIdx.x, CG = C / 8, P = 256 / CG, cg = tid % CG, ps = tid / CG;      // C <= 2048
    const half_t* x = in + (size_t)blockIdx.x * HW * C;
    if (ps < P) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int i = ps; i < HW; i += P) {
            const half8 v = *(const half8*)(x + (size_t)i * C + cg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(ps * CG + cg) * 8 + e] = acc[e];
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float s = 0.f;
        for (int k = 0; k < P; ++k) s += red[(k * CG + c / 8) * 8 + c % 8];
        out[(size_t)blockIdx.x * C + c] = (half_t)(s / (float)HW);
    }
}

int blocks_for(long long tot) { long long b = (tot + 255) / 256; return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b)); }

}  // namespace

int y7t_reid_osnet_check(const y7t_reid_op& op) {
    switch (op.type) {
    case R_H_OS_STEM:
        Y7T_ARG_CHECK(op.C == 3 && op.Co % 16 == 0 && op.Co >= 16 && op.Co <= 64 && op.b_off >= 0 && op.w_off % 4 == 0 && op.b_off % 4 == 0);
        Y7T_ARG_CHECK(op.Ho == (op.H + 6 - 7) / 2 + 1 && op.Wo == (op.W + 6 - 7) / 2 + 1 && op.H > 0 && op.W > 0);
        break;
    case R_H_OS_PW: case R_H_OS_GAPFC:
        Y7T_ARG_CHECK(op.C % 16 == 0 && op.C >= 16 && op.Co % 16 == 0 && op.Co >= 16 && op.b_off >= 0 && op.w_off % 4 == 0 && op.b_off % 4 == 0 && op.H > 0 && op.W > 0);
        if (op.type == R_H_OS_GAPFC) { Y7T_ARG_CHECK(op.aux_buf >= 0 && op.C <= 2048); break; }
        Y7T_ARG_CHECK(op.k >= Y7T_OSNET_RES_NONE && op.k <= Y7T_OSNET_RES_GEMM);
        if (op.k != Y7T_OSNET_RES_NONE) Y7T_ARG_CHECK(op.aux_buf >= 0);
        if (op.k == Y7T_OSNET_RES_GEMM) Y7T_ARG_CHECK(op.s % 16 == 0 && op.s >= 16 && op.w2_off >= 0 && op.w2_off % 4 == 0);
        break;
    case R_H_OS_LIGHT:
        Y7T_ARG_CHECK(op.C % 16 == 0 && op.C >= 16 && op.C <= 128 && op.k >= 0 && op.k <= 3 && op.s >= 1 && op.s <= 4 - op.k && op.p >= 0 && op.aux_buf >= 0);
        Y7T_ARG_CHECK(op.H > 0 && op.W > 0 && op.w_off % 4 == 0);
        if (y7t_osnet_strip_rows(op.H, op.W, op.C, op.p) < 1) { y7t_set_error("reid: a %d-wide map with %d channels does not fit the level kernel's LDS", op.W, op.C); return Y7T_E_ARG; }
        break;
    case R_H_OS_GATESUM:
        Y7T_ARG_CHECK(op.C % 16 == 0 && op.C >= 16 && op.C <= 128 && op.R >= 1 && op.R <= 8 && op.p >= 0 && op.aux_buf >= 0 && op.b_off >= 0 && op.H > 0 && op.W > 0);
        Y7T_ARG_CHECK(y7t_osnet_strip_rows(op.H, op.W, op.C, op.p) >= 1);
        break;
    case R_H_OS_INSTNORM: case R_INSTNORM:
        Y7T_ARG_CHECK(op.C % 8 == 0 && op.C >= 8 && op.b_off >= 0 && op.H > 0 && op.W > 0);
        break;
    case R_H_OS_AVGPOOL:
        Y7T_ARG_CHECK(op.C % 8 == 0 && op.C >= 8 && op.H >= 2 && op.W >= 2 && op.Ho == op.H / 2 && op.Wo == op.W / 2);
        break;
    default:
        Y7T_ARG_CHECK(false);
    }
    return 0;
}

static void launch_pw(const half_t* in, int K1, const half_t* in2, int K2, const float* wfr, const float* wfr2, const float* bias, const half_t* res, long long M, int Cout,
                      int relu, half_t* out, float* outf, hipStream_t s) {
    hipLaunchKernelGGL(k_osnet_pw, dim3((unsigned)((M + 63) / 64), (Cout / 16 + 3) / 4), dim3(256), 0, s, in, K1, in2, K2, (const half4*)wfr, (const half4*)wfr2, bias, res, M,
                       Cout, relu, out, outf);
}

int y7t_reid_osnet_launch(const y7t_reid_op& op, const float* in, float* out, float* aux, const float* wblob, int N, int max_n, hipStream_t s) {
    (void)max_n;
    const float* w = wblob + op.w_off;
    const float* bias = op.b_off >= 0 ? wblob + op.b_off : nullptr;
    switch (op.type) {
    case R_H_OS_STEM: {
        const long long M = (long long)N * op.Ho * op.Wo;
        const dim3 grid((unsigned)((M + 63) / 64));
#define Y7T_STEM(G) hipLaunchKernelGGL(k_osnet_stem<G>, grid, dim3(256), 0, s, in, op.H, op.W, op.Ho, op.Wo, M, (const half4*)w, bias, (half_t*)out)
        switch (op.Co / 16) { case 1: Y7T_STEM(1); break; case 2: Y7T_STEM(2); break; case 3: Y7T_STEM(3); break; default: Y7T_STEM(4); break; }
#undef Y7T_STEM
        break;
    }
    case R_H_OS_PW: {
        const long long M = (long long)N * op.H * op.W;
        const bool gemm2 = op.k == Y7T_OSNET_RES_GEMM;
        launch_pw((const half_t*)in, op.C, gemm2 ? (const half_t*)aux : nullptr, gemm2 ? op.s : 0, w, gemm2 ? wblob + op.w2_off : nullptr, bias,
                  op.k == Y7T_OSNET_RES_ADD ? (const half_t*)aux : nullptr, M, op.Co, op.relu & 1, (half_t*)out, nullptr, s);
        break;
    }
    case R_H_OS_LIGHT: {
        const int S = y7t_osnet_strip_rows(op.H, op.W, op.C, op.p), strips = y7t_osnet_strips(op.H, S);
        const long long HWC = (long long)op.H * op.W * op.C;
        const half_t* src = (const half_t*)in;
        long long in_crop = HWC, in_slot = 0;                        // level 0: every branch reads conv1's output
        if (op.k > 0) { src += (long long)(y7t_osnet_level_slot(op.k - 1) + 1) * HWC; in_crop = Y7T_OSNET_SLOTS * HWC; in_slot = HWC; }
        const size_t lds = (size_t)(S + 2) * (op.W + 2) * op.C * 2;
        hipLaunchKernelGGL(k_osnet_light, dim3((unsigned)N * strips, op.s), dim3(256), lds, s, src, in_crop, in_slot, (half_t*)out + (long long)y7t_osnet_level_slot(op.k) * HWC,
                           Y7T_OSNET_SLOTS * HWC, w, op.H, op.W, op.C, S, strips, op.k, aux);
        break;
    }
    case R_H_OS_GATESUM: {
        const int S = y7t_osnet_strip_rows(op.H, op.W, op.C, op.p), strips = y7t_osnet_strips(op.H, S), HW = op.H * op.W;
        const int chunk = 1024;
        hipLaunchKernelGGL(k_osnet_gatesum, dim3(N, (HW + chunk - 1) / chunk), dim3(256), 0, s, (const half_t*)in, (const float*)aux, strips, HW, op.C, op.R, w, bias,
                           wblob + op.w2_off, wblob + op.b2_off, chunk, (half_t*)out);
        break;
    }
    case R_H_OS_INSTNORM:
        hipLaunchKernelGGL(k_osnet_instnorm<half_t>, dim3(N, op.C / 8), dim3(256), 0, s, (const half_t*)in, (const half_t*)aux, op.H * op.W, op.C, w, bias, op.relu, (half_t*)out);
        break;
    case R_INSTNORM:
        hipLaunchKernelGGL(k_osnet_instnorm<float>, dim3(N, op.C / 8), dim3(256), 0, s, in, (const float*)aux, op.H * op.W, op.C, w, bias, op.relu, out);
        break;
    case R_H_OS_AVGPOOL:
        hipLaunchKernelGGL(k_osnet_avgpool2, dim3(blocks_for((long long)N * op.Ho * op.Wo * (op.C / 8))), dim3(256), 0, s, (const half_t*)in, N, op.H, op.W, op.C, (half_t*)out);
        break;
    case R_H_OS_GAPFC:
        hipLaunchKernelGGL(k_osnet_gap, dim3(N), dim3(256), 0, s, (const half_t*)in, op.H * op.W, op.C, (half_t*)aux);
        Y7T_LAUNCH_CHECK();
        launch_pw((const half_t*)aux, op.C, nullptr, 0, w, nullptr, bias, nullptr, N, op.Co, op.relu & 1, nullptr, out, s);
        break;
    default:
        Y7T_ARG_CHECK(false);
    }
    Y7T_LAUNCH_CHECK();
    return 0;
}
