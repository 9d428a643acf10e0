// y7t_dhn.hip -- the Deep Hungarian Net of DeepMOT (/root/reference/tracker/deepmot.py:10-140, class Munkrs) as gfx950 kernels, fp32 throughout, eval() mode
// (no dropout between the stacked GRU layers: DESIGN.md, DeepMOT).
//
// The network: D (h x w) flattened row-major to T = h * w scalars -> a bidirectional 2-layer GRU (hidden 256) over that sequence -> its T x 512 output re-ordered
// column-major -> a second bidirectional 2-layer GRU -> re-ordered back -> Linear(512,256), Linear(256,64), Linear(64,1) with nothing between them -> sigmoid.
// That is four PASSES (row layer 0, row layer 1, column layer 0, column layer 1) of T strictly sequential steps each; a pass runs its two directions concurrently.
//
// A pass, per chunk of at most Y7T_DHN_CHUNK steps:
//   k_dhn_proj1 / k_dhn_proj   the input projections W_ih x + b_ih of the chunk's positions, both directions (K = 1: an outer product; K = 512: a tiled fp32 FMA GEMM)
//   k_dhn_recur<S>             the recurrence.  One direction's W_hh (768 x 256 fp32 = 768 KiB) does not fit one CU, so a direction is split by hidden units over
//                              G = 256 / S workgroups, each keeping its 3 S x 256 slice of W_hh in registers for the whole launch; 2 G workgroups in all, launched
//                              with hipLaunchCooperativeKernel, which checks that they are co-resident.  Every step the 256-float h goes round as 8-byte
//                              {epoch, value} granules (relaxed agent-scope atomic stores and loads: the data is the flag, no fence): a thread stores the unit it
//                              computed and polls one granule.  EVERY SPIN IS BOUNDED: a thread that gives up makes its workgroup set the status word and leave; the
//                              others see the word (or run into their own bound) and leave too; y7t_dhn_forward_f32 then returns Y7T_E_STATE.
//   The granules carry epoch = pass * T + step + 1, which no other step of the call uses; the block of polled words is zeroed at the head of every call.
// k_dhn_head: the three linears folded into one 512-vector and a constant at load time (in float64), the sigmoid.
#include "y7t_dhn.h"
#include <math.h>
#include <string.h>
#include <mutex>
#include <unordered_map>
#include <vector>

#define Y7T_DHN_CHUNK 2048           // positions per chunk: the projections of a chunk take 2 x 2048 x 768 x 4 = 12 MiB whatever T is
#define Y7T_DHN_H 256                // hidden size
#define Y7T_DHN_SPIN_LIMIT (1u << 20)      // polls of one granule before a thread gives up (a poll is an L2 round trip: ~1 s; a step takes microseconds)

// the packed weights: the 38 tensors of Munkrs.state_dict() in its order, float32 (offsets in floats; INTEGRATION.md lists them)
static const size_t kGruSmall = 768 + 768 * 256 + 768 + 768;            // weight_ih (768 x 1), weight_hh (768 x 256), bias_ih, bias_hh
static const size_t kGruBig = 768 * 512 + 768 * 256 + 768 + 768;        // weight_ih (768 x 512), ...
static const size_t kOffHead = 2 * kGruSmall + 6 * kGruBig;             // 3945984
static const size_t kNumWeights = kOffHead + 512 * 256 + 256 + 256 * 64 + 64 + 64 + 1;      // 4093825
static size_t gru_off(int pass, int dir) {      // pass 0: lstm_row l0, 1: lstm_row l1, 2: lstm_col l0, 3: lstm_col l1
    size_t o = 0;
    for (int p = 0; p < pass; ++p) o += 2 * (p == 0 ? kGruSmall : kGruBig);
    return o + dir * (pass == 0 ? kGruSmall : kGruBig);
}

// the object's layout (bytes)
static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static const size_t kSyncBytes = 16 + 2 * 2 * 256 * 8;      // status word (padded to 16) + granules [parity][direction][unit]: the block zeroed per call, at the object's start
static const size_t kOffHw = al256(kSyncBytes);
static const size_t kOffW = kOffHw + 256;
static const size_t kOffFold = kOffW + al256(kNumWeights * 4);      // 512 floats + the constant
static const size_t kWeightBytes = kOffFold + al256(513 * 4);
struct WsLayout { size_t xp, y0, y1, D, out, total; };
static WsLayout ws_layout(size_t T) {
    WsLayout L;
    size_t o = 0;
    const size_t ch = T < Y7T_DHN_CHUNK ? T : Y7T_DHN_CHUNK;
    L.xp = o; o = al256(o + 2 * ch * 768 * 4);
    L.y0 = o; o = al256(o + T * 512 * 4);
    L.y1 = o; o = al256(o + T * 512 * 4);
    L.D = o; o = al256(o + T * 4);
    L.out = o; o = al256(o + T * 4);
    L.total = o;
    return L;
}

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned gu32;
#define Y7T_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- input projections ----
// row layer 0 (K = 1): xp[d][ls][g] = W_ih[g] * D[q] + b_ih[g]
__global__ void __launch_bounds__(256) k_dhn_proj1(const float* __restrict__ D, const float* __restrict__ w0, const float* __restrict__ w1, const float* __restrict__ b0,
                                                   const float* __restrict__ b1, float* __restrict__ xp, int s0, int ns, int T, int ch) {
    const long long tot = 2ll * ns * 768;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < tot; e += gridDim.x * 256ll) {
        const int g = (int)(e % 768), ls = (int)((e / 768) % ns), d = (int)(e / (768ll * ns));
        const int s = s0 + ls, q = d ? T - 1 - s : s;
        xp[((size_t)d * ch + ls) * 768 + g] = __builtin_fmaf((d ? w1 : w0)[g], D[q], (d ? b1 : b0)[g]);
    }
}

// K = 512: xp[d][ls][g] = sum_k X[row(ls)][k] * W_ih[g][k] + b_ih[g].  64 x 64 tile, 16-deep k chunks of both operands in LDS, 4 x 4 products per thread.
// perm: the sequence is column-major over the h x w matrix and X is in row-major order (column layer 0 reads row layer 1's output): position q = j * h + i reads row i * w + j.
__global__ void __launch_bounds__(256) k_dhn_proj(const float* __restrict__ X, const float* __restrict__ w0, const float* __restrict__ w1, const float* __restrict__ b0,
                                                  const float* __restrict__ b1, float* __restrict__ xp, int s0, int ns, int T, int ch, int perm, int hh, int ww) {
    __shared__ __attribute__((aligned(16))) float sA[16][68], sB[16][68];
    const int d = blockIdx.z, tid = threadIdx.x, m0 = blockIdx.x * 64, g0 = blockIdx.y * 64;
    const float* W = d ? w1 : w0;
    const float* bias = d ? b1 : b0;
    const int lr = tid >> 2, kq = (tid & 3) * 4, ty = tid >> 4, tx = tid & 15;
    const int ls = m0 + lr;
    const float* pa = nullptr;
    if (ls < ns) {
        const int s = s0 + ls, q = d ? T - 1 - s : s;
        const int r = perm ? (q % hh) * ww + q / hh : q;
        pa = X + (size_t)r * 512 + kq;
    }
    const float* pb = W + (size_t)(g0 + lr) * 512 + kq;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < 512; k0 += 16) {
        const float4 a = pa ? *(const float4*)(pa + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 b = *(const float4*)(pb + k0);
        __syncthreads();
        sA[kq][lr] = a.x; sA[kq + 1][lr] = a.y; sA[kq + 2][lr] = a.z; sA[kq + 3][lr] = a.w;
        sB[kq][lr] = b.x; sB[kq + 1][lr] = b.y; sB[kq + 2][lr] = b.z; sB[kq + 3][lr] = b.w;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4 av = *(const float4*)&sA[k][ty * 4], bv = *(const float4*)&sB[k][tx * 4];
            const float aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(aa[i], bb[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l = m0 + ty * 4 + i;
        if (l >= ns) continue;
        float4 o;
        o.x = acc[i][0] + bias[g0 + tx * 4]; o.y = acc[i][1] + bias[g0 + tx * 4 + 1]; o.z = acc[i][2] + bias[g0 + tx * 4 + 2]; o.w = acc[i][3] + bias[g0 + tx * 4 + 3];
        *(float4*)(xp + ((size_t)d * ch + l) * 768 + g0 + tx * 4) = o;
    }
}

// ---- the recurrence ----
struct Y7TDhnRecur {
    const float* whh[2];      // [768][256] per direction, gate rows r, z, n
    const float* bhh[2];
    const float* xp;          // [2][ch][768]  W_ih x + b_ih of the chunk's steps
    float* Y;                 // [T][512]      the layer's output in sequence order: [q][direction * 256 + unit]
    unsigned long long* exch; // [2][2][256]   granules {epoch, h bits}: [step parity][direction][unit]
    unsigned* status;
    unsigned epoch0;          // pass * T
    int s0, ns, T, ch;
};

// wait until the granule carries `epoch` -> its value; false: gave up (the bound, or another workgroup has set the status word)
__device__ __forceinline__ bool dhn_poll(gu64* g, unsigned epoch, gu32* status, unsigned& value) {
    for (unsigned spins = 0;; ++spins) {
        const unsigned long long x = __hip_atomic_load(g, Y7T_RLX_AGENT);
        if ((unsigned)(x >> 32) == epoch) { value = (unsigned)x; return true; }
        if (spins >= Y7T_DHN_SPIN_LIMIT) return false;
        if ((spins & 255u) == 255u && __hip_atomic_load(status, Y7T_RLX_AGENT) != 0u) return false;
        __builtin_amdgcn_s_sleep(1);
    }
}

__device__ __forceinline__ float dhn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// S hidden units per workgroup; L = 256 / S lanes share a unit's three 256-long dot products (lane p takes the float4 groups p, p + L, ...: the lanes of a unit read
// consecutive 16-byte slots of h in LDS) and L workgroups share a direction.  grid = 2 L workgroups of 256 threads.
template <int S>
__global__ void __launch_bounds__(256) k_dhn_recur(Y7TDhnRecur a) {
    constexpr int L = 256 / S, NV = S / 4;
    __shared__ __attribute__((aligned(16))) float hbuf[2][256];
    const int d = blockIdx.x / L, g = blockIdx.x % L;
    const int tid = threadIdx.x, u = tid / L, p = tid % L, j = g * S + u;
    float4 wr[NV], wz[NV], wn[NV];
    {
        const float* W = a.whh[d];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            wr[i] = *(const float4*)(W + (size_t)j * 256 + 4 * (p + L * i));
            wz[i] = *(const float4*)(W + (size_t)(256 + j) * 256 + 4 * (p + L * i));
            wn[i] = *(const float4*)(W + (size_t)(512 + j) * 256 + 4 * (p + L * i));
        }
    }
    const float bhr = a.bhh[d][j], bhz = a.bhh[d][256 + j], bhn = a.bhh[d][512 + j];
    gu64* ex = (gu64*)a.exch + d * 256;
    gu32* status = (gu32*)a.status;
    for (int ls = 0; ls < a.ns; ++ls) {
        const int s = a.s0 + ls, par = s & 1;
        float gr = 0.f, gz = 0.f, gn = 0.f;
        if (p == 0) {      // (issued before the wait)
            const float* x = a.xp + ((size_t)d * a.ch + ls) * 768 + j;
            gr = x[0]; gz = x[256]; gn = x[512];
        }
        // h of the previous step: thread t takes unit t's granule (written by the workgroup that owns it, this one included); step 0 starts from zero
        bool fail = false;
        float hv = 0.f;
        if (s > 0) {
            unsigned bits = 0;
            fail = !dhn_poll(ex + (par ^ 1) * 512 + tid, a.epoch0 + (unsigned)s, status, bits);
            hv = __uint_as_float(bits);
        }
        hbuf[par][tid] = hv;
        if (__syncthreads_or(fail ? 1 : 0)) {      // a stalled peer: say so and leave, all of this workgroup; the others follow
            if (tid == 0) __hip_atomic_store(status, 1u, Y7T_RLX_AGENT);
            return;
        }
        float ar = 0.f, az = 0.f, an = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float4 h4 = *(const float4*)&hbuf[par][4 * (p + L * i)];
            ar = __builtin_fmaf(wr[i].x, h4.x, ar); ar = __builtin_fmaf(wr[i].y, h4.y, ar); ar = __builtin_fmaf(wr[i].z, h4.z, ar); ar = __builtin_fmaf(wr[i].w, h4.w, ar);
            az = __builtin_fmaf(wz[i].x, h4.x, az); az = __builtin_fmaf(wz[i].y, h4.y, az); az = __builtin_fmaf(wz[i].z, h4.z, az); az = __builtin_fmaf(wz[i].w, h4.w, az);
            an = __builtin_fmaf(wn[i].x, h4.x, an); an = __builtin_fmaf(wn[i].y, h4.y, an); an = __builtin_fmaf(wn[i].z, h4.z, an); an = __builtin_fmaf(wn[i].w, h4.w, an);
        }
#pragma unroll
        for (int m = 1; m < L; m <<= 1) { ar += __shfl_xor(ar, m, 64); az += __shfl_xor(az, m, 64); an += __shfl_xor(an, m, 64); }
        if (p == 0) {      // the GRU cell: gates r, z, n; h' = (1 - z) n + z h
            const float r = dhn_sigmoid(gr + (ar + bhr)), z = dhn_sigmoid(gz + (az + bhz));
            const float n = tanhf(__builtin_fmaf(r, an + bhn, gn));
            const float hold = hbuf[par][j];
            const float hn = __builtin_fmaf(z, hold - n, n);
            const int q = d ? a.T - 1 - s : s;
            a.Y[(size_t)q * 512 + d * 256 + j] = hn;
            __hip_atomic_store(ex + par * 512 + j, ((unsigned long long)(a.epoch0 + (unsigned)s + 1u) << 32) | (unsigned long long)__float_as_uint(hn), Y7T_RLX_AGENT);
        }
    }
}

// ---- the head: out[p] = sigmoid(v . Y[q(p)] + c), a wave per position; q(p) = j * h + i for p = i * w + j (the column layers' order back to row-major) ----
__global__ void __launch_bounds__(256) k_dhn_head(const float* __restrict__ Y, const float* __restrict__ fold, float* __restrict__ out, int T, int hh, int ww) {
    const int lane = threadIdx.x & 63;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = fold[lane + 64 * c];
    const float cst = fold[512];
    for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < T; p += gridDim.x * 4) {
        const int q = (p % ww) * hh + p / ww;
        const float* y = Y + (size_t)q * 512;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc = __builtin_fmaf(v[c], y[lane + 64 * c], acc);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == 0) out[p] = dhn_sigmoid(acc + cst);
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct DhnInfo { int max_h, max_w; };
static std::mutex g_dhn_mu;
static std::unordered_map<const void*, DhnInfo> g_dhns;

extern "C" size_t y7t_dhn_weight_bytes(void) { return kWeightBytes; }
extern "C" size_t y7t_dhn_num_weights(void) { return kNumWeights; }

extern "C" size_t y7t_dhn_workspace_bytes(int max_h, int max_w) {
    if (max_h <= 0 || max_w <= 0 || (long long)max_h * max_w > Y7T_DHN_MAX_T) return 0;
    return ws_layout((size_t)max_h * max_w).total;
}

extern "C" int y7t_dhn_release(void* dhn) {
    std::lock_guard<std::mutex> l(g_dhn_mu);
    g_dhns.erase(dhn);
    return 0;
}

extern "C" int y7t_dhn_init(void* dhn, size_t bytes, const float* weights, int max_h, int max_w, y7t_stream stream) {
    Y7T_ARG_CHECK(dhn && weights && max_h > 0 && max_w > 0);
    Y7T_ARG_CHECK((long long)max_h * max_w <= Y7T_DHN_MAX_T);
    Y7T_ARG_CHECK(((uintptr_t)dhn & 255) == 0);
    Y7T_ARG_CHECK(bytes >= kWeightBytes + ws_layout((size_t)max_h * max_w).total);
    hipStream_t st = (hipStream_t)stream;
    char* b = (char*)dhn;
    // the head folded in float64: out = W3 (W2 (W1 y + b1) + b2) + b3 = v . y + c.  The three tensors come down (from the host or the device) for that
    std::vector<float> head(kNumWeights - kOffHead);
    Y7T_HIP_CHECK(hipMemcpyAsync(head.data(), weights + kOffHead, head.size() * 4, hipMemcpyDefault, st));
    Y7T_HIP_CHECK(hipMemcpyAsync(b + kOffW, weights, kNumWeights * 4, hipMemcpyDefault, st));
    Y7T_HIP_CHECK(hipStreamSynchronize(st));
    const float *W1 = head.data(), *b1 = W1 + 512 * 256, *W2 = b1 + 256, *b2 = W2 + 256 * 64, *W3 = b2 + 64, *b3 = W3 + 64;
    std::vector<double> u(256, 0.0);      // W3 W2: 1 x 256
    for (int m = 0; m < 64; ++m) for (int k = 0; k < 256; ++k) u[k] += (double)W3[m] * (double)W2[(size_t)m * 256 + k];
    std::vector<float> fold(513);
    for (int c = 0; c < 512; ++c) {
        double s = 0.0;
        for (int k = 0; k < 256; ++k) s += u[k] * (double)W1[(size_t)k * 512 + c];
        fold[c] = (float)s;
    }
    double cst = (double)b3[0];
    for (int m = 0; m < 64; ++m) cst += (double)W3[m] * (double)b2[m];
    for (int k = 0; k < 256; ++k) cst += u[k] * (double)b1[k];
    fold[512] = (float)cst;
    Y7T_HIP_CHECK(hipMemcpyAsync(b + kOffFold, fold.data(), 513 * 4, hipMemcpyHostToDevice, st));
    Y7T_HIP_CHECK(hipMemsetAsync(b, 0, kOffW, st));
    Y7T_HIP_CHECK(hipStreamSynchronize(st));      // (`fold` and `head` are this call's)
    std::lock_guard<std::mutex> l(g_dhn_mu);
    g_dhns[dhn] = DhnInfo{max_h, max_w};
    return 0;
}

int y7t_dhn_view(const void* dhn, Y7TDhnView* v) {
    DhnInfo info;
    {
        std::lock_guard<std::mutex> l(g_dhn_mu);
        auto it = g_dhns.find(dhn);
        if (it == g_dhns.end()) { y7t_set_error("this address holds no Deep Hungarian Net (y7t_dhn_init)"); return Y7T_E_STATE; }
        info = it->second;
    }
    char* b = (char*)dhn;
    const WsLayout L = ws_layout((size_t)info.max_h * info.max_w);
    v->max_h = info.max_h; v->max_w = info.max_w;
    v->D = (float*)(b + kWeightBytes + L.D); v->out = (float*)(b + kWeightBytes + L.out);
    v->hw = (int*)(b + kOffHw); v->status = (unsigned*)b;
    return 0;
}

// workgroups per direction (2, 4, 8 or 16): 4 by default (profiles/deepmot_dhn.txt); the measuring build reads Y7T_DHN_GROUPS at every call (scripts/time_deepmot.py sweeps it)
static int dhn_groups() {
    const int g = y7t_exp_switch("Y7T_DHN_GROUPS", 4);
    return (g == 2 || g == 4 || g == 8 || g == 16) ? g : 4;
}

static int launch_recur(int G, Y7TDhnRecur& a, hipStream_t st) {
    void* args[] = {&a};
    const void* k = G == 2 ? (const void*)k_dhn_recur<128> : G == 8 ? (const void*)k_dhn_recur<32> : G == 16 ? (const void*)k_dhn_recur<16> : (const void*)k_dhn_recur<64>;
    Y7T_HIP_CHECK(hipLaunchCooperativeKernel(k, dim3(2 * G), dim3(256), args, 0, st));      // (refuses a grid that is not co-resident)
    return 0;
}

int y7t_dhn_enqueue(void* dhn, const float* D, int h, int w, float* out, hipStream_t st) {
    Y7TDhnView v;
    if (int e = y7t_dhn_view(dhn, &v)) return e;
    Y7T_ARG_CHECK(D && out && h >= 1 && w >= 1);
    if ((long long)h * w > (long long)v.max_h * v.max_w) {
        y7t_set_error("y7t_dhn: a %d x %d matrix exceeds the workspace of this object (%d x %d)", h, w, v.max_h, v.max_w);
        return Y7T_E_CAPACITY;
    }
    const int T = h * w, G = dhn_groups();
    char* b = (char*)dhn;
    const WsLayout L = ws_layout((size_t)v.max_h * v.max_w);
    const int ch = (size_t)v.max_h * v.max_w < Y7T_DHN_CHUNK ? v.max_h * v.max_w : Y7T_DHN_CHUNK;
    const float* Wt = (const float*)(b + kOffW);
    float* xp = (float*)(b + kWeightBytes + L.xp);
    float* Y[2] = {(float*)(b + kWeightBytes + L.y0), (float*)(b + kWeightBytes + L.y1)};
    Y7T_HIP_CHECK(hipMemsetAsync(b, 0, kSyncBytes, st));      // every polled word, every call
    for (int pass = 0; pass < 4; ++pass) {
        const size_t in_w = pass == 0 ? 768 : (size_t)768 * 512;
        const float* blk[2] = {Wt + gru_off(pass, 0), Wt + gru_off(pass, 1)};
        const float* X = pass == 0 ? D : Y[(pass - 1) & 1];
        Y7TDhnRecur a;
        for (int d = 0; d < 2; ++d) { a.whh[d] = blk[d] + in_w; a.bhh[d] = blk[d] + in_w + 768 * 256 + 768; }
        a.xp = xp; a.Y = Y[pass & 1]; a.exch = (unsigned long long*)(b + 16); a.status = (unsigned*)b;
        a.epoch0 = (unsigned)pass * (unsigned)T; a.T = T; a.ch = ch;
        for (int s0 = 0; s0 < T; s0 += ch) {
            const int ns = T - s0 < ch ? T - s0 : ch;
            if (pass == 0) {
                int blocks = (int)((2ll * ns * 768 + 255) / 256);
                if (blocks > 2048) blocks = 2048;
                hipLaunchKernelGGL(k_dhn_proj1, dim3(blocks), dim3(256), 0, st, X, blk[0], blk[1], blk[0] + in_w + 768 * 256, blk[1] + in_w + 768 * 256, xp, s0, ns, T, ch);
            } else {
                hipLaunchKernelGGL(k_dhn_proj, dim3((ns + 63) / 64, 12, 2), dim3(256), 0, st, X, blk[0], blk[1], blk[0] + in_w + 768 * 256, blk[1] + in_w + 768 * 256, xp, s0, ns, T,
                                   ch, pass == 2 ? 1 : 0, h, w);
            }
            Y7T_LAUNCH_CHECK();
            a.s0 = s0; a.ns = ns;
            if (int e = launch_recur(G, a, st)) return e;
        }
    }
    int blocks = (T + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_dhn_head, dim3(blocks), dim3(256), 0, st, Y[1], (const float*)(b + kOffFold), out, T, h, w);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_dhn_forward_f32(void* dhn, const float* D, int h, int w, float* out, y7t_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = y7t_dhn_enqueue(dhn, D, h, w, out, st)) return e;
    unsigned status = 0;
    Y7T_HIP_CHECK(hipMemcpyAsync(&status, dhn, 4, hipMemcpyDeviceToHost, st));
    Y7T_HIP_CHECK(hipStreamSynchronize(st));
    if (status) {
        y7t_set_error("y7t_dhn_forward_f32: a workgroup of the recurrence waited for a peer's hidden state past its bound and gave up (status %u); the output is not valid", status);
        return Y7T_E_STATE;
    }
    return 0;
}
