// y7t_aflink.hip -- AFLink, the appearance-free link model of StrongSORT++ (the reference's tracker/reid_models/AFLink.py: PostLinker, eval mode) as gfx950 kernels,
// fp32 throughout, batched over candidate pairs of tracklets; and the candidate gate, the compaction into a pair list and the pair transform in front of it
// (csrc/y7t_aflink.h; DESIGN.md section 4 "AFLink").
//
// The network normalises every pair jointly, so nothing is shared between pairs: it runs once per pair, 16.4 M multiply-adds.  Pairs are processed in CHUNKS of at
// most Y7T_AFL_CHUNK, layer by layer, both branches in one launch (blockIdx.z); activations are [pair][row][column][channel] in two ping-pong buffers:
//   k_afl_block1        Cin = 1: seven taps per output, plain vector code                                       (P, 30, 3)      -> [P][24][3][32]
//   k_afl_gemm<32,7>    blocks 2-4 as implicit GEMMs on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32): M = P x rows x 3, N = Cout, K = 7 x Cin.  With the channel
//   k_afl_gemm<64,7>    innermost, tap t of output position m is the input position m + 3 t: the seven taps are seven row-shifted K-slabs of the SAME buffer, no
//   k_afl_gemm<128,7>   im2col.  The three BatchNorms of a block (one per column) stay an epilogue scale and shift per (column, channel); ReLU.
//   k_afl_gemm<768,1>   the fusion block: the (1,3) convolution collapses the three columns, which are contiguous: a plain GEMM with K = 3 x 256
//   k_afl_head          mean over the six rows, concatenation, Linear(512,128), ReLU, Linear(128,2), softmax -> score = P(link)
// A wave owns a 64 x 64 output tile (2 x 2 MFMA tiles, 64 accumulator registers) and reads both operands straight from memory as float4 along K (the four workgroup
// waves share the weight rows through L1; a chunk's activations stay cache-resident); there is no LDS, no barrier and no atomic in the network, every sum has one
// fixed order, so scores are bit-identical from call to call.  Nothing is read back between launches: in y7t_aflink_candidates the number of pairs stays on the device
// and every kernel derives its extent from it.
#include "y7t_aflink.h"
#include "y7t_common.h"
#include <string.h>
#include <mutex>
#include <unordered_map>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t al64f(size_t x) { return (x + 63) & ~(size_t)63; }

// ---- the packed state dict (offsets in floats; INTEGRATION.md lists them) ----
static const int kCin[4] = {1, 32, 64, 128}, kCout[4] = {32, 64, 128, 256};
static const size_t kRawBranch = 307040, kRawFusion = 197632, kRawFusion0 = 2 * kRawBranch, kRawCls = kRawFusion0 + 2 * kRawFusion;

// ---- the derived weights inside the object (floats, per branch region) ----
struct Derived { size_t w[4], s[4], wf, sf, branch, fc1t, b1, fc2, b2, total; };
static Derived derived_layout() {
    Derived d;
    size_t o = 0;
    for (int k = 0; k < 4; ++k) {
        d.w[k] = o; o = al64f(o + (size_t)kCout[k] * kCin[k] * 7);
        d.s[k] = o; o = al64f(o + (size_t)6 * kCout[k]);      // scale[3][Cout], shift[3][Cout]
    }
    d.wf = o; o = al64f(o + (size_t)256 * 768);
    d.sf = o; o = al64f(o + 512);
    d.branch = o;
    o = 2 * d.branch;
    d.fc1t = o; o = al64f(o + 512 * 128);
    d.b1 = o; o = al64f(o + 128);
    d.fc2 = o; o = al64f(o + 256);
    d.b2 = o; o = al64f(o + 2);
    d.total = o;
    return d;
}
static const size_t kOffW = 256;      // (the first 256 bytes of the object are a header nothing polls)
static size_t weight_bytes() { return kOffW + al256(derived_layout().total * 4); }

enum { kActFloats = 4608 };           // floats per pair and branch of an activation buffer: the largest layer output (12 x 3 x 128 = 6 x 3 x 256)
struct WsLayout { size_t bufA, bufB, x, rowcnt, rowoff, total; int ch; };
static WsLayout ws_layout(int max_tracklets, int max_pairs) {
    WsLayout L;
    L.ch = max_pairs < Y7T_AFL_CHUNK ? max_pairs : Y7T_AFL_CHUNK;
    size_t o = 0;
    L.bufA = o; o = al256(o + (size_t)2 * L.ch * kActFloats * 4);
    L.bufB = o; o = al256(o + (size_t)2 * L.ch * kActFloats * 4);
    L.x = o; o = al256(o + (size_t)2 * L.ch * Y7T_AFL_BLOCK * 4);
    L.rowcnt = o; o = al256(o + (size_t)max_tracklets * 4);
    L.rowoff = o; o = al256(o + (size_t)max_tracklets * 4);
    L.total = o;
    return L;
}

// pairs of this chunk: all of pmax when the count is the host's, else what the device-side count leaves of [p0, p0 + pmax)
__device__ __forceinline__ int afl_chunk_pairs(const int* cnt, int cap, int p0, int pmax) {
    if (!cnt) return pmax;
    int c = *cnt;
    if (c > cap) c = cap;
    c -= p0;
    return c < 0 ? 0 : (c > pmax ? pmax : c);
}

// ---- block 1: out[b][p][r][c][co] = relu(scale[c][co] * sum_t x[b][p][r + t][c] * w[co][t] + shift[c][co]), r < 24 ----
__global__ void __launch_bounds__(256) k_afl_block1(const float* __restrict__ x1, const float* __restrict__ x2, float* __restrict__ out, const float* __restrict__ wts,
                                                    size_t w_off, size_t s_off, size_t w_branch, size_t out_branch, const int* __restrict__ cnt, int cap, int p0, int pmax) {
    const int b = blockIdx.z, P = afl_chunk_pairs(cnt, cap, p0, pmax);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * 72 * 32) return;
    const int co = idx & 31, m = idx >> 5, p = m / 72, rc = m % 72, c = rc % 3;
    const float* x = (b ? x2 : x1) + (size_t)p * Y7T_AFL_BLOCK + rc;
    const float* w = wts + b * w_branch + w_off + co * 7;
    const float* ss = wts + b * w_branch + s_off;
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 7; ++t) acc = __builtin_fmaf(x[3 * t], w[t], acc);
    const float v = __builtin_fmaf(acc, ss[c * 32 + co], ss[96 + c * 32 + co]);
    out[b * out_branch + (size_t)m * 32 + co] = v > 0.f ? v : 0.f;
}

// ---- blocks 2-4 and the fusion convolution ----
// out[b][m][n] = relu(scale[m % ncol][n] * sum_{t < TAPS} sum_{ci < CIN} in[b][row(m) + 3 t][ci] * W[b][n][t][ci] + shift[m % ncol][n])
// row(m) = (m / RO3) * RI3 + m % RO3: output position m = (pair, row, column) among RO3 a pair, input positions RI3 a pair.  M = P * RO3 rows, COUT % 64 == 0.
// grid (ceil(M / 256), COUT / 64, 2 branches), 256 threads: wave w takes rows [(4 blockIdx.x + w) 64, + 64).  Lane (r = l & 31, h = l >> 5) loads four consecutive
// k of row r of each operand at k0 + 4 h and feeds MFMA j with element j: A[i = r][k = h] and B[k = h][j = r] then carry the same k = k0 + 4 h + j on both sides.
// Rows past M read row M - 1 (in bounds) and are not stored.
template <int CIN, int TAPS>
__global__ void __launch_bounds__(256) k_afl_gemm(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ wts, size_t w_off, size_t s_off,
                                                  size_t w_branch, size_t in_branch, size_t out_branch, const int* __restrict__ cnt, int cap, int p0, int pmax, int RI3,
                                                  int RO3, int COUT, int ncol) {
    const int b = blockIdx.z, P = afl_chunk_pairs(cnt, cap, p0, pmax), M = P * RO3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int m0 = (blockIdx.x * 4 + wave) * 64, n0 = blockIdx.y * 64;
    if (m0 >= M) return;
    constexpr int K = TAPS * CIN;
    const float* arow[2];
    const float* brow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = m0 + 32 * i + r;
        if (m > M - 1) m = M - 1;
        arow[i] = in + b * in_branch + (size_t)((m / RO3) * RI3 + m % RO3) * CIN + 4 * h;
        brow[i] = wts + b * w_branch + w_off + (size_t)(n0 + 32 * i + r) * K + 4 * h;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    for (int t = 0; t < TAPS; ++t) {
        const float* a0 = arow[0] + (size_t)t * 3 * CIN;
        const float* a1 = arow[1] + (size_t)t * 3 * CIN;
        const float* b0 = brow[0] + t * CIN;
        const float* b1 = brow[1] + t * CIN;
#pragma unroll 2
        for (int c0 = 0; c0 < CIN; c0 += 8) {
            const float4 av0 = *(const float4*)(a0 + c0), av1 = *(const float4*)(a1 + c0);
            const float4 bv0 = *(const float4*)(b0 + c0), bv1 = *(const float4*)(b1 + c0);
            const float aa[2][4] = {{av0.x, av0.y, av0.z, av0.w}, {av1.x, av1.y, av1.z, av1.w}};
            const float bb[2][4] = {{bv0.x, bv0.y, bv0.z, bv0.w}, {bv1.x, bv1.y, bv1.z, bv1.w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[0][j], bb[0][j], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[0][j], bb[1][j], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[1][j], bb[0][j], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[1][j], bb[1][j], acc[1][1], 0, 0, 0);
            }
        }
    }
    // C / D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const float* scale = wts + b * w_branch + s_off;
    const float* shift = scale + (size_t)ncol * COUT;
    float* o = out + b * out_branch;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = m0 + 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h;
            if (m >= M) continue;
            const int c = m % ncol;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + 32 * j + r;
                const float v = __builtin_fmaf(acc[i][j][q], scale[c * COUT + n], shift[c * COUT + n]);
                o[(size_t)m * COUT + n] = v > 0.f ? v : 0.f;
            }
        }
}

// ---- pooling and classifier: Y7T_AFL_HEAD_PAIRS pairs a workgroup share every read of fc1 (stored transposed: [k][unit]) ----
__global__ void __launch_bounds__(256) k_afl_head(const float* __restrict__ f, size_t f_branch, const float* __restrict__ wts, size_t o_fc1t, size_t o_b1, size_t o_fc2,
                                                  size_t o_b2, float* __restrict__ scores, const int* __restrict__ cnt, int cap, int p0, int pmax) {
    constexpr int PP = Y7T_AFL_HEAD_PAIRS;
    __shared__ float v[PP][512], hb[PP][128], lg[PP][2];
    const int P = afl_chunk_pairs(cnt, cap, p0, pmax), tid = threadIdx.x, pbase = blockIdx.x * PP;
    if (pbase >= P) return;      // (the whole workgroup)
    for (int e = tid; e < PP * 512; e += 256) {
        const int pp = e >> 9, k = e & 511, br = k >> 8, c = k & 255, p = pbase + pp;
        float s = 0.f;
        if (p < P) {
            const float* src = f + br * f_branch + (size_t)p * 1536 + c;
            for (int r = 0; r < 6; ++r) s += src[r * 256];
            s = s / 6.0f;
        }
        v[pp][k] = s;
    }
    __syncthreads();
    {
        const int j = tid & 127, g = tid >> 7;
        const float* w = wts + o_fc1t + j;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 512; ++k) {
            const float wk = w[(size_t)k * 128];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_fmaf(wk, v[g * 4 + q][k], acc[q]);
        }
        const float bias = wts[o_b1 + j];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const float t = acc[q] + bias; hb[g * 4 + q][j] = t > 0.f ? t : 0.f; }
    }
    __syncthreads();
    if (tid < 2 * PP) {
        const int pp = tid >> 1, o = tid & 1;
        const float* w = wts + o_fc2 + o * 128;
        float acc = 0.f;
        for (int j = 0; j < 128; ++j) acc = __builtin_fmaf(w[j], hb[pp][j], acc);
        lg[pp][o] = acc + wts[o_b2 + o];
    }
    __syncthreads();
    if (tid < PP && pbase + tid < P) {
        const float l0 = lg[tid][0], l1 = lg[tid][1], mx = l0 > l1 ? l0 : l1;
        const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
        scores[(size_t)p0 + pbase + tid] = e1 / (e0 + e1);
    }
}

// ---- candidates: gate, deterministic compaction (no atomics: counts per row, a scan, an ordered emit), transform ----
__global__ void __launch_bounds__(256) k_afl_gate_count(const double* __restrict__ rows, const int* __restrict__ off, int N, double t0, double t1, double s,
                                                        int* __restrict__ rowcnt) {
    __shared__ int red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    int c = 0;
    for (int j = tid; j < N; j += 256) c += y7t_afl_gate(rows, off, i, j, t0, t1, s) ? 1 : 0;
    red[tid] = c;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) rowcnt[i] = red[0];
}

__global__ void __launch_bounds__(256) k_afl_scan(const int* __restrict__ rowcnt, int N, int max_pairs, int* __restrict__ rowoff, int* __restrict__ count_out,
                                                  int* __restrict__ status_out) {
    __shared__ int part[256];
    const int tid = threadIdx.x, seg = (N + 255) / 256, lo = tid * seg, hi = lo + seg < N ? lo + seg : N;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += rowcnt[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        count_out[0] = run;
        status_out[0] = run > max_pairs ? Y7T_AFL_OVERFLOW : 0;
    }
    __syncthreads();
    int run = part[tid];
    for (int i = lo; i < hi; ++i) { rowoff[i] = run; run += rowcnt[i]; }
}

__global__ void __launch_bounds__(256) k_afl_emit(const double* __restrict__ rows, const int* __restrict__ off, int N, double t0, double t1, double s,
                                                  const int* __restrict__ rowoff, int max_pairs, int* __restrict__ pairs) {
    __shared__ int wt[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run = rowoff[i];
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int j = j0 + tid;
        const bool f = j < N && y7t_afl_gate(rows, off, i, j, t0, t1, s);
        const unsigned long long mask = __ballot(f);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wt[wave] = __popcll(mask);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 4; ++w) { if (w < wave) woff += wt[w]; tot += wt[w]; }
        const int pos = run + woff + before;
        if (f && pos < max_pairs) { pairs[2 * (size_t)pos] = i; pairs[2 * (size_t)pos + 1] = j; }
        run += tot;
        __syncthreads();
    }
}

// a wave per pair: lane l < 60 owns row l of the 60 (former 0..29, latter 30..59); lanes 60..63 repeat rows 0..3, which changes no minimum or maximum
__global__ void __launch_bounds__(256) k_afl_transform(const double* __restrict__ rows, const int* __restrict__ off, const int* __restrict__ pairs,
                                                       const int* __restrict__ cnt, int cap, int p0, int pmax, float* __restrict__ xbuf, size_t x_branch,
                                                       float* __restrict__ x1_out, float* __restrict__ x2_out) {
    const int P = afl_chunk_pairs(cnt, cap, p0, pmax), lane = threadIdx.x & 63, lp = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (lp >= P) return;
    const size_t p = (size_t)p0 + lp;
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    const int row = lane < 60 ? lane : lane - 60, latter = row >= Y7T_AFL_LEN ? 1 : 0, r = row - latter * Y7T_AFL_LEN;
    double v[3], mn[3], mx[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = y7t_afl_block_at(rows, off, latter ? j : i, latter, r, c);
        mn[c] = v[c]; mx[c] = v[c];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double a = __shfl_xor(mn[c], m, 64), b = __shfl_xor(mx[c], m, 64);
            mn[c] = a < mn[c] ? a : mn[c];
            mx[c] = b > mx[c] ? b : mx[c];
        }
    }
    if (lane >= 60) return;
    float* dst = xbuf + latter * x_branch + (size_t)lp * Y7T_AFL_BLOCK + r * 3;
    float* ext = latter ? x2_out : x1_out;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double sub, div;
        y7t_afl_norm(mn[c], mx[c], &sub, &div);
        const float o = y7t_afl_apply(v[c], sub, div);
        dst[c] = o;
        if (ext) ext[p * Y7T_AFL_BLOCK + r * 3 + c] = o;
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct AflInfo { int max_tracklets, max_rows, max_pairs; };
static std::mutex g_afl_mu;
static std::unordered_map<const void*, AflInfo> g_afls;

extern "C" size_t y7t_aflink_num_weights(void) { return Y7T_AFL_NUM_WEIGHTS; }
extern "C" size_t y7t_aflink_weight_bytes(void) { return weight_bytes(); }

static bool caps_ok(int max_tracklets, int max_rows, int max_pairs) {
    return max_tracklets >= 1 && max_tracklets <= Y7T_AFL_MAX_TRACKLETS && max_rows >= 1 && max_pairs >= 1 && max_pairs <= (1 << 24);
}

extern "C" size_t y7t_aflink_workspace_bytes(int max_tracklets, int max_rows, int max_pairs) {
    if (!caps_ok(max_tracklets, max_rows, max_pairs)) return 0;
    return ws_layout(max_tracklets, max_pairs).total;
}

extern "C" int y7t_aflink_release(void* obj) {
    std::lock_guard<std::mutex> l(g_afl_mu);
    g_afls.erase(obj);
    return 0;
}

// eval-mode BatchNorm as y = x * scale + shift, folded in float64: raw = {weight, bias, running_mean, running_var} of n channels each
static void bn_fold(const float* raw, int n, float* scale, float* shift) {
    for (int c = 0; c < n; ++c) {
        const double g = raw[c], b = raw[n + c], mu = raw[2 * n + c], var = raw[3 * n + c];
        const double s = g / sqrt(var + 1e-5);
        scale[c] = (float)s;
        shift[c] = (float)(b - mu * s);
    }
}

extern "C" int y7t_aflink_init(void* obj, size_t bytes, const float* weights, int max_tracklets, int max_rows, int max_pairs, y7t_stream stream) {
    Y7T_ARG_CHECK(obj && weights);
    Y7T_ARG_CHECK(caps_ok(max_tracklets, max_rows, max_pairs));
    Y7T_ARG_CHECK(((uintptr_t)obj & 255) == 0);
    Y7T_ARG_CHECK(bytes >= weight_bytes() + ws_layout(max_tracklets, max_pairs).total);
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> raw(Y7T_AFL_NUM_WEIGHTS);
    Y7T_HIP_CHECK(hipMemcpyAsync(raw.data(), weights, raw.size() * 4, hipMemcpyDefault, st));
    Y7T_HIP_CHECK(hipStreamSynchronize(st));
    const Derived d = derived_layout();
    std::vector<float> dv(d.total, 0.f);
    for (int b = 0; b < 2; ++b) {
        const float* src = raw.data() + b * kRawBranch;
        float* dst = dv.data() + b * d.branch;
        for (int k = 0; k < 4; ++k) {
            const int ci = kCin[k], co = kCout[k];
            // conv.weight [co][ci][7][1] -> [co][tap][ci]
            for (int o = 0; o < co; ++o)
                for (int c = 0; c < ci; ++c)
                    for (int t = 0; t < 7; ++t) dst[d.w[k] + ((size_t)o * 7 + t) * ci + c] = src[((size_t)o * ci + c) * 7 + t];
            src += (size_t)co * ci * 7;
            for (int col = 0; col < 3; ++col) {      // bnf, bnx, bny
                bn_fold(src, co, dst + d.s[k] + col * co, dst + d.s[k] + (3 + col) * co);
                src += 4 * co;
            }
        }
        const float* fs = raw.data() + kRawFusion0 + b * kRawFusion;
        // conv.weight [co][ci][1][3] -> [co][column][ci]
        for (int o = 0; o < 256; ++o)
            for (int c = 0; c < 256; ++c)
                for (int t = 0; t < 3; ++t) dst[d.wf + ((size_t)o * 3 + t) * 256 + c] = fs[((size_t)o * 256 + c) * 3 + t];
        bn_fold(fs + 256 * 256 * 3, 256, dst + d.sf, dst + d.sf + 256);
    }
    const float* cs = raw.data() + kRawCls;      // fc1.weight [128][512], fc1.bias, fc2.weight [2][128], fc2.bias
    for (int j = 0; j < 128; ++j)
        for (int k = 0; k < 512; ++k) dv[d.fc1t + (size_t)k * 128 + j] = cs[(size_t)j * 512 + k];
    memcpy(dv.data() + d.b1, cs + 128 * 512, 128 * 4);
    memcpy(dv.data() + d.fc2, cs + 128 * 512 + 128, 256 * 4);
    memcpy(dv.data() + d.b2, cs + 128 * 512 + 128 + 256, 2 * 4);
    char* b = (char*)obj;
    Y7T_HIP_CHECK(hipMemsetAsync(b, 0, kOffW, st));
    Y7T_HIP_CHECK(hipMemcpyAsync(b + kOffW, dv.data(), dv.size() * 4, hipMemcpyHostToDevice, st));
    Y7T_HIP_CHECK(hipStreamSynchronize(st));      // (`dv` is this call's)
    std::lock_guard<std::mutex> l(g_afl_mu);
    g_afls[obj] = AflInfo{max_tracklets, max_rows, max_pairs};
    return 0;
}

static int afl_info(const void* obj, AflInfo* info) {
    std::lock_guard<std::mutex> l(g_afl_mu);
    auto it = g_afls.find(obj);
    if (it == g_afls.end()) { y7t_set_error("this address holds no AFLink object (y7t_aflink_init)"); return Y7T_E_STATE; }
    *info = it->second;
    return 0;
}

// the network over one chunk: x1 / x2 point at the chunk's first pair; scores at pair 0 of the call
static int afl_enqueue_chunk(char* obj, const WsLayout& L, const float* x1, const float* x2, float* scores, const int* cnt, int cap, int p0, int pmax, hipStream_t st) {
    const Derived d = derived_layout();
    const float* wts = (const float*)(obj + kOffW);
    char* ws = obj + weight_bytes();
    float *A = (float*)(ws + L.bufA), *B = (float*)(ws + L.bufB);
    const size_t ab = (size_t)L.ch * kActFloats;
    hipLaunchKernelGGL(k_afl_block1, dim3((pmax * 72 * 32 + 255) / 256, 1, 2), dim3(256), 0, st, x1, x2, A, wts, d.w[0], d.s[0], d.branch, ab, cnt, cap, p0, pmax);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_afl_gemm<32, 7>), dim3((pmax * 54 + 255) / 256, 1, 2), dim3(256), 0, st, A, B, wts, d.w[1], d.s[1], d.branch, ab, ab, cnt, cap, p0, pmax, 72, 54, 64, 3);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_afl_gemm<64, 7>), dim3((pmax * 36 + 255) / 256, 2, 2), dim3(256), 0, st, B, A, wts, d.w[2], d.s[2], d.branch, ab, ab, cnt, cap, p0, pmax, 54, 36, 128, 3);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_afl_gemm<128, 7>), dim3((pmax * 18 + 255) / 256, 4, 2), dim3(256), 0, st, A, B, wts, d.w[3], d.s[3], d.branch, ab, ab, cnt, cap, p0, pmax, 36, 18, 256, 3);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_afl_gemm<768, 1>), dim3((pmax * 6 + 255) / 256, 4, 2), dim3(256), 0, st, B, A, wts, d.wf, d.sf, d.branch, ab, ab, cnt, cap, p0, pmax, 6, 6, 256, 1);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afl_head, dim3((pmax + Y7T_AFL_HEAD_PAIRS - 1) / Y7T_AFL_HEAD_PAIRS), dim3(256), 0, st, A, ab, wts, d.fc1t, d.b1, d.fc2, d.b2, scores, cnt, cap, p0, pmax);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_aflink_score_pairs_f32(void* obj, const float* x1, const float* x2, int P, float* scores, y7t_stream stream) {
    AflInfo info;
    if (int e = afl_info(obj, &info)) return e;
    Y7T_ARG_CHECK(P >= 0 && (P == 0 || (x1 && x2 && scores)));
    const WsLayout L = ws_layout(info.max_tracklets, info.max_pairs);
    for (int p0 = 0; p0 < P; p0 += L.ch) {
        const int n = P - p0 < L.ch ? P - p0 : L.ch;
        if (int e = afl_enqueue_chunk((char*)obj, L, x1 + (size_t)p0 * Y7T_AFL_BLOCK, x2 + (size_t)p0 * Y7T_AFL_BLOCK, scores, nullptr, 0, p0, n, (hipStream_t)stream)) return e;
    }
    return 0;
}

extern "C" int y7t_aflink_candidates(void* obj, const double* rows, const int* row_offsets, int n_tracklets, double thrT0, double thrT1, double thrS, int* pairs_out,
                                     float* x1_out, float* x2_out, float* scores_out, int* count_out, int* status_out, y7t_stream stream) {
    AflInfo info;
    if (int e = afl_info(obj, &info)) return e;
    Y7T_ARG_CHECK(n_tracklets >= 0 && row_offsets && pairs_out && scores_out && count_out && status_out && (n_tracklets == 0 || rows));
    if (n_tracklets > info.max_tracklets) {
        y7t_set_error("y7t_aflink_candidates: %d tracklets exceed this object's capacity (%d)", n_tracklets, info.max_tracklets);
        return Y7T_E_CAPACITY;
    }
    hipStream_t st = (hipStream_t)stream;
    const int N = n_tracklets;
    if (N == 0) {
        Y7T_HIP_CHECK(hipMemsetAsync(count_out, 0, 4, st));
        Y7T_HIP_CHECK(hipMemsetAsync(status_out, 0, 4, st));
        return 0;
    }
    const WsLayout L = ws_layout(info.max_tracklets, info.max_pairs);
    char* ws = (char*)obj + weight_bytes();
    int *rowcnt = (int*)(ws + L.rowcnt), *rowoff = (int*)(ws + L.rowoff);
    float* xbuf = (float*)(ws + L.x);
    const size_t xb = (size_t)L.ch * Y7T_AFL_BLOCK;
    hipLaunchKernelGGL(k_afl_gate_count, dim3(N), dim3(256), 0, st, rows, row_offsets, N, thrT0, thrT1, thrS, rowcnt);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afl_scan, dim3(1), dim3(256), 0, st, rowcnt, N, info.max_pairs, rowoff, count_out, status_out);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afl_emit, dim3(N), dim3(256), 0, st, rows, row_offsets, N, thrT0, thrT1, thrS, rowoff, info.max_pairs, pairs_out);
    Y7T_LAUNCH_CHECK();
    // the count stays on the device: chunks are enqueued up to the most this table can yield, and every kernel leaves at once where the list has ended
    const long long most = (long long)N * (N - 1);
    const int bound = most < info.max_pairs ? (int)most : info.max_pairs;
    for (int p0 = 0; p0 < bound; p0 += L.ch) {
        const int n = bound - p0 < L.ch ? bound - p0 : L.ch;
        hipLaunchKernelGGL(k_afl_transform, dim3((n + 3) / 4), dim3(256), 0, st, rows, row_offsets, pairs_out, count_out, info.max_pairs, p0, n, xbuf, xb, x1_out, x2_out);
        Y7T_LAUNCH_CHECK();
        if (int e = afl_enqueue_chunk((char*)obj, L, xbuf, xbuf + xb, scores_out, count_out, info.max_pairs, p0, n, st)) return e;
    }
    return 0;
}
