// y7t_tracker.hip -- gfx950 kernels + C ABI for the tracker half of the hot path
// (Kalman predict/update, IoU cost, linear assignment, fused ByteTrack/SORT frame step).
// The arithmetic lives in y7t_track_core.h / y7t_track_step.h (reference citations there).
//
// Roofline notes: all of these are HBM/latency bound, none is a
// contraction -> no MFMA.  Kalman predict moves 1152 B/track, IoU 32(N+M) B in + 8NM B out,
// the fused step keeps the LAP work arrays and (when it fits) the cost matrix in LDS.
#include "y7t_common.h"
#include "y7t_track_step.h"
#include "y7t_track_deepsort.h"
#include "y7t_track_strongsort.h"
#include "y7t_track_botsort_reid.h"
#include "y7t_track_deepmot.h"
#include "y7t_dhn.h"
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <unordered_map>

static thread_local char g_err[512] = "";
void y7t_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* y7t_last_error(void) { return g_err; }
// diagnostics: name of the kernel the last launch helper of this thread chose (conv dispatch rules live on the host side of the
// library, so "which kernel runs this layer at this batch" is a property tests and bench.py can read back)
static thread_local char g_kernel[128] = "";
void y7t_note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
}
extern "C" const char* y7t_last_kernel(void) { return g_kernel; }
extern "C" int y7t_version(void) { return 100; }
extern "C" int y7t_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

// ---------------------------------------------------------------------------------------------
// per-op kernels
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_iou_cost(const double* __restrict__ a, int n, const double* __restrict__ b, int m,
                                                  double* __restrict__ cost) {
    // one thread per (i, j); j fastest -> coalesced 8-byte stores, box rows broadcast through L1
    const long long tot = (long long)n * m;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < tot; k += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(k / m), j = (int)(k - (long long)i * m);
        double bi[4], bj[4];
        for (int c = 0; c < 4; ++c) { bi[c] = a[4 * (size_t)i + c]; bj[c] = b[4 * (size_t)j + c]; }
        cost[k] = y7t_iou_dist(bi, bj);
    }
}

__global__ void __launch_bounds__(64) k_kf_initiate(int kind, const double* __restrict__ z, double* mean, double* cov, int K,
                                                    int flags) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    double zz[4], m[8], P[64];
    for (int c = 0; c < 4; ++c) zz[c] = z[4 * (size_t)k + c];
    y7t_kf_initiate(kind, zz, flags & 1, m, P);
    for (int c = 0; c < 8; ++c) mean[8 * (size_t)k + c] = m[c];
    for (int c = 0; c < 64; ++c) cov[64 * (size_t)k + c] = P[c];
}

__global__ void __launch_bounds__(64) k_kf_predict(int kind, double* mean, double* cov, const uint8_t* __restrict__ mask, int N) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    double m[8], P[64];
    for (int c = 0; c < 8; ++c) m[c] = mean[8 * (size_t)k + c];
    for (int c = 0; c < 64; ++c) P[c] = cov[64 * (size_t)k + c];
    if (mask && mask[k]) m[7] = 0.0;
    y7t_kf_predict(kind, m, P);
    for (int c = 0; c < 8; ++c) mean[8 * (size_t)k + c] = m[c];
    for (int c = 0; c < 64; ++c) cov[64 * (size_t)k + c] = P[c];
}

__global__ void __launch_bounds__(64) k_kf_project(int kind, const double* __restrict__ mean, const double* __restrict__ cov,
                                                   const double* __restrict__ conf, double* pm, double* pc, int N) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    double m[8], P[64], a[4], S[16];
    for (int c = 0; c < 8; ++c) m[c] = mean[8 * (size_t)k + c];
    for (int c = 0; c < 64; ++c) P[c] = cov[64 * (size_t)k + c];
    y7t_kf_project(kind, m, P, conf ? conf[k] : 0.0, a, S);
    for (int c = 0; c < 4; ++c) pm[4 * (size_t)k + c] = a[c];
    for (int c = 0; c < 16; ++c) pc[16 * (size_t)k + c] = S[c];
}

__global__ void __launch_bounds__(64) k_kf_update(int kind, double* mean, double* cov, const double* __restrict__ z,
                                                  const int* __restrict__ idx, const double* __restrict__ conf, int K) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int t = idx ? idx[k] : k;
    double m[8], P[64], zz[4];
    for (int c = 0; c < 8; ++c) m[c] = mean[8 * (size_t)t + c];
    for (int c = 0; c < 64; ++c) P[c] = cov[64 * (size_t)t + c];
    for (int c = 0; c < 4; ++c) zz[c] = z[4 * (size_t)k + c];
    y7t_kf_update(kind, m, P, zz, conf ? conf[k] : 0.0);
    for (int c = 0; c < 8; ++c) mean[8 * (size_t)t + c] = m[c];
    for (int c = 0; c < 64; ++c) cov[64 * (size_t)t + c] = P[c];
}

__global__ void __launch_bounds__(64) k_kf_gating(int kind, const double* __restrict__ mean, const double* __restrict__ cov,
                                                  const double* __restrict__ z, int N, int M, int only_pos, double* out) {
    const long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (k >= (long long)N * M) return;
    const int i = (int)(k / M), j = (int)(k - (long long)i * M);
    double m[8], P[64], zz[4];
    for (int c = 0; c < 8; ++c) m[c] = mean[8 * (size_t)i + c];
    for (int c = 0; c < 64; ++c) P[c] = cov[64 * (size_t)i + c];
    for (int c = 0; c < 4; ++c) zz[c] = z[4 * (size_t)j + c];
    out[k] = y7t_kf_gating(kind, m, P, zz, only_pos);
}

// ---------------------------------------------------------------------------------------------
// single-workgroup programs: LAPJV and the fused tracker step.  Dynamic LDS layout:
//   [0, 512)  rv  (64 doubles)   [512, 768) ri (64 ints)   [1024, ...) fast scratch
// ---------------------------------------------------------------------------------------------
#define Y7T_LDS_HDR 1024
extern __shared__ __attribute__((aligned(16))) char y7t_smem[];

__device__ __forceinline__ Y7TExec make_exec(unsigned fast_bytes) {
    Y7TExec ex;
    ex.tid = threadIdx.x; ex.nt = blockDim.x;
    ex.rv = (double*)y7t_smem; ex.ri = (int*)(y7t_smem + 512);
    ex.fast = fast_bytes ? y7t_smem + Y7T_LDS_HDR : nullptr;
    ex.fast_bytes = fast_bytes;
    ex.arena = nullptr; ex.arena_bytes = 0;
    return ex;
}
// its sibling for the programs that use no LDS: this thread of that many
__device__ __forceinline__ Y7TExec make_exec_flat(int tid, int nt) {
    Y7TExec ex;
    ex.tid = tid; ex.nt = nt;
    ex.rv = nullptr; ex.ri = nullptr; ex.fast = nullptr; ex.fast_bytes = 0;
    ex.arena = nullptr; ex.arena_bytes = 0;
    return ex;
}

__global__ void k_lapjv(const double* __restrict__ cost, int nr, int nc, double limit, int* x, int* y, double* opt, void* ws_g,
                        unsigned fast_bytes, int jv_extended) {
    const Y7TExec ex = make_exec(fast_bytes);
    Y7TLap L;
    L.nr = nr; L.nc = nc; L.ld = nc; L.n = nr + nc; L.half = limit / 2.0; L.prof = nullptr;
    const size_t ws = y7t_al(y7t_lap_ws_bytes(L.n)), cb = (size_t)nr * nc * sizeof(double);
    void* lapws = ws_g;
    size_t off = 0;
    if (ws <= fast_bytes) { lapws = ex.fast; off = ws; }
    const double* c = cost;
    if (ex.fast && off + cb <= fast_bytes) {  // stage the cost matrix in LDS
        double* cl = (double*)(ex.fast + off);
        for (int k = ex.tid; k < nr * nc; k += ex.nt) cl[k] = cost[k];
        c = cl;
    }
    __syncthreads();
    L.c = c;
    y7t_lap_bind(L, lapws, L.n);
    if (jv_extended) y7t_lap_solve(ex, L);
    else if (y7t_lap_solve_sap(ex, L)) y7t_lap_solve_literal(ex, L);      // ties: lapjv's own order decides
    for (int i = ex.tid; i < nr; i += ex.nt) x[i] = (L.x[i] >= nc) ? -1 : L.x[i];
    for (int j = ex.tid; j < nc; j += ex.nt) y[j] = (L.y[j] >= nr) ? -1 : L.y[j];
    if (opt && ex.tid == 0) {
        double s = 0.0;
        for (int i = 0; i < nr; ++i) if (L.x[i] < nc) s += cost[(size_t)i * nc + L.x[i]];
        *opt = s;
    }
}

__global__ void k_tracker_init(void* blob, Y7TTrkCfg cfg, unsigned long long idc) {
    const Y7TExec ex = make_exec_flat(threadIdx.x, blockDim.x);
    y7t_tracker_init(ex, blob, cfg, idc);
}

// ---- the frame-step kernels: three launch forms x the step programs of y7t_track_step.h (y7t_step_one: which body a program runs and why the instances are separate).
// MAXT is the launch's thread bound and the instance's register budget: the host runs a launch of nt threads on the smallest MAXT >= nt (launch_step).
// Only the instances the entry points name exist.  `warp` is the ByteTrack family's camera-motion matrix; the C-BIoU and UAVMOT programs ignore it. ----
template <int PROG, int MAXT>      // one frame of one pool
__global__ void __launch_bounds__(MAXT) k_tracker_step(void* state, const float* dets, int n, double* out_rows, int out_cap, int* out_count, unsigned fast_bytes,
                                                        const double* warp) {
    const Y7TExec ex = make_exec(fast_bytes);
    y7t_step_one<PROG, y7t_step_inlined(PROG, MAXT)>(ex, state, dets, n, out_rows, out_cap, out_count, warp);
}

// n_frames consecutive frames of ONE tracker in one launch: the same frame step, frame after frame, by the same workgroup (the state stays hot in
// this CU's caches and nothing is launched between frames).  For pipelines that have a whole batch's detections before the tracker runs.
template <int PROG, int MAXT>
__global__ void __launch_bounds__(MAXT) k_tracker_step_frames(void* state, const float* const* dets, const int* n_dets, double* const* out_rows, int* const* out_count, int out_cap,
                                                               int n_frames, unsigned fast_bytes, unsigned arena_bytes, const double* const* warps) {
    Y7TExec ex = make_exec(fast_bytes);
    if (arena_bytes) { ex.arena = y7t_smem + Y7T_LDS_HDR + fast_bytes; ex.arena_bytes = arena_bytes; }      // the index lists live in LDS for the whole launch
    y7t_arena_load(ex, state);
    for (int f = 0; f < n_frames; ++f) {
        y7t_step_one<PROG, y7t_step_inlined(PROG, MAXT)>(ex, state, dets[f], n_dets[f], out_rows[f], out_cap, out_count[f], warps ? warps[f] : nullptr);
        y7t_sync(ex);
    }
    y7t_arena_store(ex, state);
}

// one workgroup per pool of a batch.  PLAIN: while no C-BIoU / UAVMOT pool exists in the process (its 1024-thread instance runs the called copy, which serves C-BIoU
// too); ANY: a launch cannot see its pools' kinds, so this one branches on every workgroup's pool
template <int PROG, int MAXT>
__global__ void __launch_bounds__(MAXT) k_tracker_step_batch(void* const* states, const float* const* dets, const int* n_dets, double* const* out_rows,
                                                              int* out_count, int out_cap, unsigned fast_bytes, const double* const* warps) {
    const int b = blockIdx.x;
    const Y7TExec ex = make_exec(fast_bytes);
    y7t_step_one<PROG, y7t_step_inlined(PROG, MAXT)>(ex, states[b], dets[b], n_dets[b], out_rows[b], out_cap, out_count + b, warps ? warps[b] : nullptr);
}

// matching.structure_similarity_distance: one workgroup, the n + m structure vectors in LDS (a lane per element), then the n x m cosine distances
__global__ void __launch_bounds__(256) k_structure_distance(const double* __restrict__ txy, int n, const double* __restrict__ dxy, int m, double* __restrict__ out) {
    double* sv = (double*)y7t_smem;
    for (int k = threadIdx.x; k < n + m; k += blockDim.x) {
        if (k < n) y7t_amf_vec<double>(n, k, [&](int b, int c) { return txy[2 * b + c]; }, sv + 3 * k);
        else y7t_amf_vec<float>(m, k - n, [&](int b, int c) { return (float)dxy[2 * b + c]; }, sv + 3 * k);
    }
    __syncthreads();
    const long long tot = (long long)n * m;
    for (long long e = threadIdx.x; e < tot; e += blockDim.x) {
        const int i = (int)(e / m), j = (int)(e - (long long)i * m);
        out[e] = y7t_amf_cos_dist(sv + 3 * i, sv + 3 * (n + j));
    }
}

// a step the library refuses on the device side: the pool's status word says why (Y7T_ERR_KIND), no row is returned
__global__ void k_tracker_refuse(void* state, int* out_count) {
    if (threadIdx.x == 0) {
        ((Y7TTrkHdr*)state)->status |= Y7T_ERR_KIND;
        if (out_count) *out_count = 0;
    }
}

// ---- DeepSORT (y7t_track_deepsort.h) ----
__global__ void k_feat_init(void* fblob, int cap_t, int cap_d, int dim, int budget) {
    const Y7TExec ex = make_exec_flat(threadIdx.x, blockDim.x);
    y7t_feat_init(ex, fblob, cap_t, cap_d, dim, budget);
}

// detection features of the frame -> normalised rows (a wave per detection)
__global__ void __launch_bounds__(256) k_ds_normalize(void* fblob, const float* __restrict__ det_feats, int n) {
    const Y7TFeat f = y7t_feat_bind(fblob);
    const Y7TExec ex = make_exec_flat(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    if (n > f.h->cap_d) n = f.h->cap_d;      // (the step reports Y7T_ERR_CAP_D; nothing is written past the state)
    y7t_feat_normalize_dets(ex, f, det_feats, n);
}

// nearest-embedding distances, tiled: a workgroup takes (slot, 64 detections), the slot's stored rows 32 at a time, 32-deep k chunks of both operands in LDS,
// 2 x 4 products per thread.  Every product is the sequential FMA chain over k = 0 .. dim-1 of y7t_embed_slot (= numpy's sgemm), so the costs -- and
// the assignment that follows them -- are bit-identical; only the order in which DIFFERENT products advance changes.
// Round 6: the grid is (Y7T_EMBED_WORKERS, detection tiles) instead of (cap_tracks, detection tiles).  Every workgroup walks the state column once, ranks the live
// slots (Tracked / Lost) in slot order and takes those whose rank is its blockIdx.x modulo the worker count: a frame with 64 live tracks of a 512-slot pool launched
// 1024 workgroups of which ~900 found nothing to do -- beside the detector each of them queued for a CU slot first (the kernel ran 128 us per frame in the cfg4
// pipeline against 38 us alone, profiles/r06_batch_80.txt section 4).
#define Y7T_EMBED_WORKERS 128
__global__ void __launch_bounds__(256) k_embed_dist(void* blob, void* fblob, int n) {
    const Y7TTrkHdr* h = (const Y7TTrkHdr*)blob;
    const Y7TTrk s = y7t_trk_bind(blob, h->cfg.cap_t, h->cfg.cap_d);
    const int j0 = blockIdx.y * 64, cap_t = h->cfg.cap_t;
    if (n > h->cfg.cap_d) n = h->cfg.cap_d;
    const Y7TFeat f = y7t_feat_bind(fblob);
    const int dim = f.h->dim, tid = threadIdx.x;
    __shared__ float sA[32][33], sB[64][33], smin[16][64];
    __shared__ int s_cnt[4], s_own[64], s_nown;
    // ---- the live slots of rank = blockIdx.x (mod gridDim.x), in slot order ----
    if (tid == 0) s_nown = 0;
    int seen = 0;      // live slots below `base` (uniform)
    for (int base = 0; base < cap_t; base += 256) {
        const int sl = base + tid;
        bool live = false;
        if (sl < cap_t) { const int st = s.state[sl]; live = st == Y7T_TRACKED || st == Y7T_LOST; }
        const unsigned long long bal = __ballot(live);
        __syncthreads();                                   // (s_cnt of the previous round has been read; s_nown's initial store is visible)
        if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(bal);
        __syncthreads();
        int before = seen;
        for (int w = 0; w < (tid >> 6); ++w) before += s_cnt[w];
        const int rank = before + __popcll(bal & ((1ull << (tid & 63)) - 1ull));
        if (live && rank % (int)gridDim.x == (int)blockIdx.x) { const int k = rank / (int)gridDim.x; if (k < 64) s_own[k] = sl; atomicMax(&s_nown, k + 1); }
        seen += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
    __syncthreads();
    const int n_own = s_nown < 64 ? s_nown : 64;      // (64 x the worker count live tracks: more than any pool this library is given; the launcher checks cap_tracks)
    for (int oi = 0; oi < n_own; ++oi) {
        const int slot = s_own[oi];
        const int nf = f.nfeat[slot];
        if (dim & 31) {      // feature dimensions that are not a multiple of the k chunk: the plain form, one workgroup per slot
            if (blockIdx.y == 0) {
                const Y7TExec ex = make_exec_flat(threadIdx.x, blockDim.x);
                y7t_embed_slot(ex, f, slot, n, s.tsu[slot]);
            }
            continue;
        }
        if (nf <= 0 || j0 >= n) continue;
        const int ty = tid >> 4, tx = tid & 15, lrow = tid >> 3, kq = (tid & 7) * 4;
        const float* hist = f.ring + (size_t)slot * f.h->budget * dim;
        float best[4] = {3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f};
        // (round 6: the NEXT k chunk's global loads are issued before the current chunk's products -- beside the detector a load takes several times what it takes alone,
        //  and the loop used to wait for every chunk with nothing else to do)
        auto fetch = [&](int h0, int k0, float4& va, float4& vb0, float4& vb1) {
            va = make_float4(0.f, 0.f, 0.f, 0.f); vb0 = va; vb1 = va;
            if (h0 + lrow < nf) va = *(const float4*)(hist + (size_t)(h0 + lrow) * dim + k0 + kq);
            if (j0 + lrow < n) vb0 = *(const float4*)(f.detn + (size_t)(j0 + lrow) * dim + k0 + kq);
            if (j0 + 32 + lrow < n) vb1 = *(const float4*)(f.detn + (size_t)(j0 + 32 + lrow) * dim + k0 + kq);
        };
        float4 va, vb0, vb1;
        fetch(0, 0, va, vb0, vb1);
        for (int h0 = 0; h0 < nf; h0 += 32) {
            float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            for (int k0 = 0; k0 < dim; k0 += 32) {
                __syncthreads();
                sA[lrow][kq] = va.x; sA[lrow][kq + 1] = va.y; sA[lrow][kq + 2] = va.z; sA[lrow][kq + 3] = va.w;
                sB[lrow][kq] = vb0.x; sB[lrow][kq + 1] = vb0.y; sB[lrow][kq + 2] = vb0.z; sB[lrow][kq + 3] = vb0.w;
                sB[32 + lrow][kq] = vb1.x; sB[32 + lrow][kq + 1] = vb1.y; sB[32 + lrow][kq + 2] = vb1.z; sB[32 + lrow][kq + 3] = vb1.w;
                __syncthreads();
                if (k0 + 32 < dim) fetch(h0, k0 + 32, va, vb0, vb1);
                else if (h0 + 32 < nf) fetch(h0 + 32, 0, va, vb0, vb1);
#pragma unroll 8
                for (int k = 0; k < 32; ++k) {
                    const float a0 = sA[2 * ty][k], a1 = sA[2 * ty + 1][k];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float b = sB[tx + 16 * c][k];
                        acc[0][c] = __builtin_fmaf(a0, b, acc[0][c]);
                        acc[1][c] = __builtin_fmaf(a1, b, acc[1][c]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if (h0 + 2 * ty + r < nf)
#pragma unroll
                    for (int c = 0; c < 4; ++c) { const float d = 1.0f - acc[r][c]; best[c] = d < best[c] ? d : best[c]; }
        }
        __syncthreads();                                   // (the previous slot's reduction has read smin)
#pragma unroll
        for (int c = 0; c < 4; ++c) smin[ty][tx + 16 * c] = best[c];
        __syncthreads();
        if (tid < 64 && j0 + tid < n) {
            float m = smin[0][tid];
            for (int q = 1; q < 16; ++q) m = smin[q][tid] < m ? smin[q][tid] : m;
            f.app[(size_t)slot * f.h->cap_d + j0 + tid] = m;
            if ((double)m <= 0.15) { const int a = s.tsu[slot]; atomicMin(f.cmin + j0 + tid, a); atomicMax(f.cmax + j0 + tid, a); }
        }
    }
}

// the appearance vectors the step queued -> the rings (a wave per vector, across the grid)
__global__ void __launch_bounds__(256) k_ds_store(void* fblob, const float* __restrict__ det_feats) {
    const Y7TFeat f = y7t_feat_bind(fblob);
    const Y7TExec ex = make_exec_flat(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    y7t_feat_store_pending(ex, f, det_feats);
}

template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_tracker_step_deepsort(void* state, void* fblob, const float* dets, int n, const float* det_feats, double* out_rows,
                                                                 int out_cap, int* out_count, unsigned fast_bytes) {
    const Y7TExec ex = make_exec(fast_bytes);
    y7t_tracker_step_deepsort(ex, state, fblob, dets, n, det_feats, out_rows, out_cap, out_count);
}

// ---- StrongSORT (y7t_track_strongsort.h): three launches per frame -- k_ss_appearance, k_tracker_step_strongsort, k_ss_store ----
__global__ void k_ss_init(void* fblob, int cap_t, int cap_d, int dim, double gamma) {
    const Y7TExec ex = make_exec_flat(threadIdx.x, blockDim.x);
    y7t_ss_init(ex, fblob, cap_t, cap_d, dim, gamma);
}

// matching.embedding_distance(tracks, detections, 'euclidean') for every slot of the tracked / lost lists (confirmed and unconfirmed alike: the unconfirmed association
// reads the same matrix) against every detection row above det_thresh, tiled like k_embed_dist: a workgroup takes 32 list entries x 64 detections, 32-deep k chunks of
// both operands in LDS, 2 x 4 pairs per thread, the next chunk's global loads issued before the current chunk's arithmetic.  Every pair's sum is the sequential float64
// chain over k = 0 .. dim-1 of y7t_scipy_euclidean (= scipy's cdist, y7t_np_arith.h), so the distances -- and the assignments that follow them -- are bit-identical to the plain form; only the
// order in which DIFFERENT pairs advance changes.  The grid is (workers, detection tiles): a worker walks the groups of 32 list entries whose number is its blockIdx.x
// modulo the worker count (the lists' lengths are only known on the device).  The rows are the LISTS, not the state column: a lost track that aged out last frame is
// Removed but still in the lost list for this frame's association (basetrack's sub_stracks runs before removed_stracks.extend), and its row takes part in the solve.
// vec_ok: both operands are 16-byte aligned (float4 loads); otherwise, and for dimensions that are not a multiple of the k chunk, the plain lane-per-pair form.
#define Y7T_SS_WORKERS 64
__global__ void __launch_bounds__(256) k_ss_appearance(void* blob, void* fblob, const float* __restrict__ dets, const float* __restrict__ det_feats, int n, int vec_ok) {
    const Y7TTrkHdr* h = (const Y7TTrkHdr*)blob;
    const int cap_t = h->cfg.cap_t;
    const Y7TTrk s = y7t_trk_bind(blob, cap_t, h->cfg.cap_d);
    const Y7TSs f = y7t_ss_bind(fblob);
    if (h->cfg.tracker != Y7T_STRONGSORT || f.h->cap_t < cap_t || f.h->cap_d < h->cfg.cap_d) return;      // (the step reports it; nothing is read or written past either state)
    if (n > h->cfg.cap_d) n = h->cfg.cap_d;
    const int j0 = blockIdx.y * 64;
    if (j0 >= n) return;
    const int dim = f.h->dim, ld = f.h->cap_d, tid = threadIdx.x;
    const int nt0 = h->n_tracked < cap_t ? h->n_tracked : cap_t, nl0 = h->n_lost < cap_t ? h->n_lost : cap_t, n_live = nt0 + nl0;
    const float det_t = (float)h->cfg.det_thresh;
    __shared__ float sA[32][33], sB[64][33];
    __shared__ int s_slot[32], s_use[64];
    if (tid < 64) s_use[tid] = (j0 + tid < n && y7t_ss_row_used(dets, j0 + tid, det_t)) ? 1 : 0;
    const int ty = tid >> 4, tx = tid & 15, lrow = tid >> 3, kq = (tid & 7) * 4;
    for (int g = blockIdx.x; g * 32 < n_live; g += gridDim.x) {
        __syncthreads();                                   // (the previous group's pairs have read s_slot)
        if (tid < 32) {
            const int r = g * 32 + tid;
            int sl = r < n_live ? y7t_ss_live_slot(s, nt0, r) : -1;
            if (sl < 0 || sl >= cap_t) sl = -1;
            s_slot[tid] = sl;
        }
        __syncthreads();
        if ((dim & 31) || !vec_ok) {                       // the plain form: the group's 32 x 64 pairs, a lane per pair
            for (int e = tid; e < 32 * 64; e += 256) {
                const int sl = s_slot[e >> 6], c = e & 63;
                if (sl < 0 || !s_use[c]) continue;
                f.app[(size_t)sl * ld + j0 + c] = y7t_ss_dist(f.vec + (size_t)sl * dim, det_feats + (size_t)(j0 + c) * dim, dim);
            }
            continue;
        }
        const int sla = s_slot[lrow];
        const float* pa = sla >= 0 ? f.vec + (size_t)sla * dim + kq : nullptr;
        const float* pb0 = s_use[lrow] ? det_feats + (size_t)(j0 + lrow) * dim + kq : nullptr;
        const float* pb1 = s_use[32 + lrow] ? det_feats + (size_t)(j0 + 32 + lrow) * dim + kq : nullptr;
        auto fetch = [&](int k0, float4& va, float4& vb0, float4& vb1) {
            va = make_float4(0.f, 0.f, 0.f, 0.f); vb0 = va; vb1 = va;
            if (pa) va = *(const float4*)(pa + k0);
            if (pb0) vb0 = *(const float4*)(pb0 + k0);
            if (pb1) vb1 = *(const float4*)(pb1 + k0);
        };
        double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        float4 va, vb0, vb1;
        fetch(0, va, vb0, vb1);
        for (int k0 = 0; k0 < dim; k0 += 32) {
            __syncthreads();
            sA[lrow][kq] = va.x; sA[lrow][kq + 1] = va.y; sA[lrow][kq + 2] = va.z; sA[lrow][kq + 3] = va.w;
            sB[lrow][kq] = vb0.x; sB[lrow][kq + 1] = vb0.y; sB[lrow][kq + 2] = vb0.z; sB[lrow][kq + 3] = vb0.w;
            sB[32 + lrow][kq] = vb1.x; sB[32 + lrow][kq + 1] = vb1.y; sB[32 + lrow][kq + 2] = vb1.z; sB[32 + lrow][kq + 3] = vb1.w;
            __syncthreads();
            if (k0 + 32 < dim) fetch(k0 + 32, va, vb0, vb1);
#pragma unroll 8
            for (int k = 0; k < 32; ++k) {
                const float a0 = sA[2 * ty][k], a1 = sA[2 * ty + 1][k];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float b = sB[tx + 16 * c][k];
                    acc[0][c] = y7t_scipy_sqstep(acc[0][c], a0, b);
                    acc[1][c] = y7t_scipy_sqstep(acc[1][c], a1, b);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int sl = s_slot[2 * ty + r];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (sl >= 0 && s_use[tx + 16 * c]) f.app[(size_t)sl * ld + j0 + tx + 16 * c] = y7t_scipy_root(acc[r][c]);
        }
    }
}

// the appearance vectors the step queued -> the slots' vectors: the float32 moving average of STrack.update or the raw copy of a new track (a wave per vector, across the grid)
__global__ void __launch_bounds__(256) k_ss_store(void* fblob, const float* __restrict__ det_feats) {
    const Y7TSs f = y7t_ss_bind(fblob);
    const Y7TExec ex = make_exec_flat(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    y7t_ss_store_pending(ex, f, det_feats);
}

template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_tracker_step_strongsort(void* state, void* fblob, const float* dets, int n, const float* det_feats, double* out_rows,
                                                                   int out_cap, int* out_count, unsigned fast_bytes, const double* warp) {
    const Y7TExec ex = make_exec(fast_bytes);
    y7t_tracker_step_strongsort(ex, state, fblob, dets, n, det_feats, out_rows, out_cap, out_count, warp);
}

// ---- BoT-SORT with its appearance branch (y7t_track_botsort_reid.h): three launches per frame -- k_br_prepare, k_tracker_step_botsort_reid, k_br_store ----
__global__ void k_br_init(void* fblob, int cap_t, int cap_d, int dim, double theta_iou, double theta_emb) {
    const Y7TExec ex = make_exec_flat(threadIdx.x, blockDim.x);
    y7t_br_init(ex, fblob, cap_t, cap_d, dim, theta_iou, theta_emb);
}

// the frame's normalised float64 rows -- the vectors of the slots of the tracked / lost lists and the detection rows at or above det_thresh -- a wave per row, across
// the grid (numpy's pairwise sum of squares by the wave's first eight lanes, the divisions a lane per element).  A row that cannot be normalised sets status bit 4
__global__ void __launch_bounds__(256) k_br_prepare(void* blob, void* fblob, const float* __restrict__ dets, const float* __restrict__ det_feats, int n) {
    const Y7TTrkHdr* h = (const Y7TTrkHdr*)blob;
    const Y7TTrk s = y7t_trk_bind(blob, h->cfg.cap_t, h->cfg.cap_d);
    const Y7TBr f = y7t_br_bind(fblob);
    if (h->cfg.tracker != Y7T_BOTSORT_REID || f.h->ss.cap_t < h->cfg.cap_t || f.h->ss.cap_d < h->cfg.cap_d) return;      // (the step reports it; nothing is read or written past either state)
    const Y7TExec ex = make_exec_flat(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    y7t_br_prepare(ex, s, f, dets, det_feats, n);
}

// the appearance vectors the step queued -> the slots' vectors: StrongSORT's store (y7t_ss_store_pending) on this feature state's queue of two entries per detection
__global__ void __launch_bounds__(256) k_br_store(void* fblob, const float* __restrict__ det_feats) {
    const Y7TBr f = y7t_br_bind(fblob);
    const Y7TExec ex = make_exec_flat(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    y7t_ss_store_pending<Y7T_BR_PPD>(ex, f.ss, det_feats);
}

template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_tracker_step_botsort_reid(void* state, void* fblob, const float* dets, int n, const float* det_feats, double* out_rows,
                                                                     int out_cap, int* out_count, unsigned fast_bytes, const double* warp) {
    const Y7TExec ex = make_exec(fast_bytes);
    y7t_tracker_step_botsort_reid(ex, state, fblob, dets, n, det_feats, out_rows, out_cap, out_count, warp);
}

// ---- DeepMOT (y7t_track_deepmot.h): the two programs of a frame, on either side of the Deep Hungarian Net's launches (y7t_dhn.hip) ----
template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_deepmot_front(void* state, const float* dets, int n, int img_h, int img_w, float* D, long long d_cap, int* hw, unsigned fast_bytes) {
    const Y7TExec ex = make_exec(fast_bytes);
    y7t_deepmot_front(ex, state, dets, n, img_h, img_w, D, d_cap, hw);
}
template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_deepmot_back(void* state, const float* dets, const float* net_out, const unsigned* net_status, double* out_rows, int out_cap,
                                                        int* out_count, unsigned fast_bytes) {
    const Y7TExec ex = make_exec(fast_bytes);
    y7t_deepmot_back(ex, state, dets, net_out, net_status, out_rows, out_cap, out_count);
}

__global__ void __launch_bounds__(64) k_kf_gmc(double* mean, double* cov, const double* __restrict__ warp, int N) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    double m[8], P[64], H[6];
    for (int c = 0; c < 6; ++c) H[c] = warp[c];
    for (int c = 0; c < 8; ++c) m[c] = mean[8 * (size_t)k + c];
    for (int c = 0; c < 64; ++c) P[c] = cov[64 * (size_t)k + c];
    y7t_kf_gmc(y7t_warp_load(H), m, P);
    for (int c = 0; c < 8; ++c) mean[8 * (size_t)k + c] = m[c];
    for (int c = 0; c < 64; ++c) cov[64 * (size_t)k + c] = P[c];
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static inline hipStream_t S(y7t_stream s) { return (hipStream_t)s; }
static const unsigned kFastBytes = 128 * 1024;  // fast scratch per workgroup (of the CU's 160 KiB LDS)
// Fast scratch of a frame step.  Asking for less than the maximum on small frames (so that the step's workgroup can share a CU with the detector's
// workgroups instead of waiting for one to drain) was measured: no gain in the step's start latency, and the association's cost matrix / candidate
// lists falling back to the state blob made the in-pipeline chain 12 % slower (14.1 -> 15.8 ms per 32 frames).  Y7T_TRACKER_FAST_KB overrides.
static unsigned step_fast_bytes(int n_dets) {
    static int forced = -1;
    if (forced < 0) forced = y7t_exp_switch("Y7T_TRACKER_FAST_KB", 0) * 1024;
    if (forced > 0) return (unsigned)(forced < (int)kFastBytes ? forced : (int)kFastBytes);
    (void)n_dets;
    return kFastBytes;
}

// (Round 6 measured the step kernels asking for the CU's WHOLE 160 KiB so that no convolution workgroup shares their CU: cfg3 chain 26.95 / 26.91 ms with, 27.01 without;
// cfg4 35.02 / 35.01 vs 35.17; cfg2 11.21 / 11.27 vs 11.33 -- nothing, removed (profiles/r06_small_experiments.txt).  What slows the step beside a running detector is
// not a neighbour on its CU.)
template <class K>
static int ensure_lds(K kernel, unsigned bytes) {
    Y7T_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
// the attribute is per device and the callers may be threads of several trackers: done-bits per device, set after the call succeeded.  The done-word is a
// static of this function, which is instantiated once per kernel instance: no launch can pair a kernel with another kernel's word
template <auto KERNEL>
static int ensure_lds_once(unsigned bytes) {
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    Y7T_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    if (int e = ensure_lds(KERNEL, bytes)) return e;
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

// A frame-step launch: FAMILY::k<MAXT> is a kernel template's instance for MAXT threads, FAMILY::kMinT the smallest one that exists.  This is the one place that maps a
// launch's thread count to an instance: the smallest MAXT >= nt of 256 / 512 / 1024 (register budgets: y7t_step_one, y7t_track_step.h; thread counts: step_threads).
// lds_max: what the instance is allowed once per device; lds: what this launch asks for
template <auto KERNEL, class... A>
static int launch_instance(int blocks, int nt, unsigned lds_max, unsigned lds, y7t_stream stream, A... args) {
    if (int e = ensure_lds_once<KERNEL>(lds_max)) return e;
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(nt), lds, S(stream), args...);
    Y7T_LAUNCH_CHECK();
    return 0;
}
template <class FAMILY, class... A>
static int launch_step(int blocks, int nt, unsigned lds_max, unsigned lds, y7t_stream stream, A... args) {
    if constexpr (FAMILY::kMinT <= 256) if (nt <= 256) return launch_instance<FAMILY::template k<256>>(blocks, nt, lds_max, lds, stream, args...);
    if (nt <= 512) return launch_instance<FAMILY::template k<512>>(blocks, nt, lds_max, lds, stream, args...);
    return launch_instance<FAMILY::template k<1024>>(blocks, nt, lds_max, lds, stream, args...);
}
template <int PROG> struct StepSingle { static const int kMinT = 256; template <int MAXT> static constexpr auto k = &k_tracker_step<PROG, MAXT>; };
template <int PROG> struct StepFrames { static const int kMinT = 256; template <int MAXT> static constexpr auto k = &k_tracker_step_frames<PROG, MAXT>; };
template <int PROG> struct StepBatch { static const int kMinT = 512; template <int MAXT> static constexpr auto k = &k_tracker_step_batch<PROG, MAXT>; };      // (launches of <= 256 threads take the 512 instance)
struct StepDeepsort { static const int kMinT = 256; template <int MAXT> static constexpr auto k = &k_tracker_step_deepsort<MAXT>; };
struct StepStrongsort { static const int kMinT = 256; template <int MAXT> static constexpr auto k = &k_tracker_step_strongsort<MAXT>; };
struct StepBotsortReid { static const int kMinT = 256; template <int MAXT> static constexpr auto k = &k_tracker_step_botsort_reid<MAXT>; };
struct StepDeepmotFront { static const int kMinT = 256; template <int MAXT> static constexpr auto k = &k_deepmot_front<MAXT>; };
struct StepDeepmotBack { static const int kMinT = 256; template <int MAXT> static constexpr auto k = &k_deepmot_back<MAXT>; };

extern "C" int y7t_iou_cost_f64(const double* a, int n, const double* b, int m, double* cost, y7t_stream stream) {
    Y7T_ARG_CHECK(n >= 0 && m >= 0);
    if (n == 0 || m == 0) return 0;
    Y7T_ARG_CHECK(a && b && cost);
    const long long tot = (long long)n * m;
    int blocks = (int)((tot + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_iou_cost, dim3(blocks), dim3(256), 0, S(stream), a, n, b, m, cost);
    Y7T_LAUNCH_CHECK();
    return 0;
}

static int kind_ok(int kind) { return kind == Y7T_KF_XYAH || kind == Y7T_KF_XYWH || kind == Y7T_KF_NSA; }

extern "C" int y7t_structure_distance_f64(const double* track_xy, int n, const double* det_xy, int m, double* out, y7t_stream stream) {
    Y7T_ARG_CHECK(n >= 0 && m >= 0 && n + m <= 2048);      // (the vectors of both lists in one workgroup's LDS: 48 KiB)
    if (n == 0 || m == 0) return 0;
    Y7T_ARG_CHECK(track_xy && det_xy && out);
    hipLaunchKernelGGL(k_structure_distance, dim3(1), dim3(256), (size_t)(n + m) * 3 * sizeof(double), S(stream), track_xy, n, det_xy, m, out);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_kf_initiate_f64(int kind, const double* z, double* mean, double* cov, int K, int flags, y7t_stream stream) {
    Y7T_ARG_CHECK(K >= 0);
    if (!kind_ok(kind)) { y7t_set_error("kalman kind %d is not implemented on the device (default/botsort/strongsort are)", kind); return Y7T_E_ARG; }
    if (K == 0) return 0;
    Y7T_ARG_CHECK(z && mean && cov);
    hipLaunchKernelGGL(k_kf_initiate, dim3((K + 63) / 64), dim3(64), 0, S(stream), kind, z, mean, cov, K, flags);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_kf_multi_predict_f64(int kind, double* mean, double* cov, const uint8_t* mask, int N, y7t_stream stream) {
    Y7T_ARG_CHECK(N >= 0);
    if (!kind_ok(kind)) { y7t_set_error("kalman kind %d is not implemented on the device", kind); return Y7T_E_ARG; }
    if (N == 0) return 0;
    Y7T_ARG_CHECK(mean && cov);
    hipLaunchKernelGGL(k_kf_predict, dim3((N + 63) / 64), dim3(64), 0, S(stream), kind, mean, cov, mask, N);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_kf_project_f64(int kind, const double* mean, const double* cov, const double* conf, double* pmean,
                                  double* pcov, int N, y7t_stream stream) {
    Y7T_ARG_CHECK(N >= 0);
    if (!kind_ok(kind)) { y7t_set_error("kalman kind %d is not implemented on the device", kind); return Y7T_E_ARG; }
    if (N == 0) return 0;
    Y7T_ARG_CHECK(mean && cov && pmean && pcov);
    hipLaunchKernelGGL(k_kf_project, dim3((N + 63) / 64), dim3(64), 0, S(stream), kind, mean, cov, conf, pmean, pcov, N);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_kf_update_batch_f64(int kind, double* mean, double* cov, const double* z, const int* track_idx,
                                       const double* conf, int K, y7t_stream stream) {
    Y7T_ARG_CHECK(K >= 0);
    if (!kind_ok(kind)) { y7t_set_error("kalman kind %d is not implemented on the device", kind); return Y7T_E_ARG; }
    if (K == 0) return 0;
    Y7T_ARG_CHECK(mean && cov && z);
    hipLaunchKernelGGL(k_kf_update, dim3((K + 63) / 64), dim3(64), 0, S(stream), kind, mean, cov, z, track_idx, conf, K);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_kf_gating_f64(int kind, const double* mean, const double* cov, const double* z, int N, int M,
                                 int only_position, double* out, y7t_stream stream) {
    Y7T_ARG_CHECK(N >= 0 && M >= 0);
    if (!kind_ok(kind)) { y7t_set_error("kalman kind %d is not implemented on the device", kind); return Y7T_E_ARG; }
    if (N == 0 || M == 0) return 0;
    Y7T_ARG_CHECK(mean && cov && z && out);
    const long long tot = (long long)N * M;
    hipLaunchKernelGGL(k_kf_gating, dim3((unsigned)((tot + 63) / 64)), dim3(64), 0, S(stream), kind, mean, cov, z, N, M,
                       only_position, out);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_lap_literal_calls(void) {
    int v = -1;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(y7t_g_literal_calls), sizeof(int)) != hipSuccess) return -1;
    return v;
}

extern "C" size_t y7t_lapjv_workspace_bytes(int n, int m) {
    if (n < 0 || m < 0) return 0;
    return y7t_al(y7t_lap_ws_bytes(n + m)) + 64;
}

extern "C" int y7t_lapjv_f64(const double* cost, int n, int m, double cost_limit, int* x, int* y, double* opt, void* workspace,
                             y7t_stream stream) {
    Y7T_ARG_CHECK(n >= 0 && m >= 0);
    if (n == 0 || m == 0) {
        // matching.py:31-32: an empty cost matrix leaves everything unmatched
        if (n) Y7T_HIP_CHECK(hipMemsetAsync(x, 0xff, sizeof(int) * (size_t)n, S(stream)));
        if (m) Y7T_HIP_CHECK(hipMemsetAsync(y, 0xff, sizeof(int) * (size_t)m, S(stream)));
        if (opt) Y7T_HIP_CHECK(hipMemsetAsync(opt, 0, sizeof(double), S(stream)));
        return 0;
    }
    Y7T_ARG_CHECK(cost && x && y && workspace);
    if (int e = ensure_lds_once<&k_lapjv>(kFastBytes + Y7T_LDS_HDR)) return e;
    const int nn = n + m;
    const int threads = nn <= 128 ? 64 : (nn <= 512 ? 256 : 1024);
    static int jv = -1;
    if (jv < 0) jv = y7t_exp_switch("Y7T_LAP_JV_EXTENDED", 0);
    hipLaunchKernelGGL(k_lapjv, dim3(1), dim3(threads), kFastBytes + Y7T_LDS_HDR, S(stream), cost, n, m, cost_limit, x, y, opt,
                       workspace, kFastBytes, jv);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_lapjv_f64_host(const double* cost_host, int n, int m, double cost_limit, int* x_host, int* y_host, double* opt_host, y7t_stream stream) {
    Y7T_ARG_CHECK(n >= 0 && m >= 0 && (n == 0 || x_host) && (m == 0 || y_host));
    if (n == 0 || m == 0) {
        for (int i = 0; i < n; ++i) x_host[i] = -1;
        for (int j = 0; j < m; ++j) y_host[j] = -1;
        if (opt_host) *opt_host = 0.0;
        return 0;
    }
    Y7T_ARG_CHECK(cost_host);
    static char* buf = nullptr;            // one staging allocation per process, grown on demand: cost | x | y | opt | solver workspace
    static size_t cap = 0;
    static std::mutex mu;                  // matching.linear_assignment routes every numpy call through here: one caller at a time owns the buffer
    std::lock_guard<std::mutex> lock(mu);  // (the call synchronises its stream before returning, so nothing of it is in flight when the lock drops)
    const size_t cb = y7t_al(sizeof(double) * (size_t)n * m), xb = y7t_al(sizeof(int) * (size_t)n), yb = y7t_al(sizeof(int) * (size_t)m), ob = y7t_al(sizeof(double));
    const size_t need = cb + xb + yb + ob + y7t_lapjv_workspace_bytes(n, m);
    if (need > cap) {
        if (buf) Y7T_HIP_CHECK(hipFree(buf));
        buf = nullptr; cap = 0;
        Y7T_HIP_CHECK(hipMalloc((void**)&buf, need));
        cap = need;
    }
    double* dc = (double*)buf; int* dx = (int*)(buf + cb); int* dy = (int*)(buf + cb + xb); double* dopt = (double*)(buf + cb + xb + yb);
    Y7T_HIP_CHECK(hipMemcpyAsync(dc, cost_host, sizeof(double) * (size_t)n * m, hipMemcpyHostToDevice, S(stream)));
    if (int e = y7t_lapjv_f64(dc, n, m, cost_limit, dx, dy, dopt, buf + cb + xb + yb + ob, stream)) return e;
    Y7T_HIP_CHECK(hipMemcpyAsync(x_host, dx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, S(stream)));
    Y7T_HIP_CHECK(hipMemcpyAsync(y_host, dy, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, S(stream)));
    if (opt_host) Y7T_HIP_CHECK(hipMemcpyAsync(opt_host, dopt, sizeof(double), hipMemcpyDeviceToHost, S(stream)));
    Y7T_HIP_CHECK(hipStreamSynchronize(S(stream)));
    return 0;
}

// what the host side knows of every initialised state blob (the header itself lives in device memory): its tracker kind and the bytes of LDS its index lists take
// (y7t_arena_bytes of its capacities).  The plain frame step refuses a DeepSORT pool with detections -- it would create / update tracks without the appearance-ring
// bookkeeping, and a reused slot would keep its previous occupant's vectors.  Only the predict-only form (n < 0) is shared between the trackers.
struct PoolInfo { int kind; size_t arena_bytes; int cap_t; };
static std::mutex g_pool_mu;
static std::unordered_map<const void*, PoolInfo> g_pools;
static std::atomic<int> g_n_cbiou{0}, g_n_uavmot{0}, g_n_strongsort{0}, g_n_deepmot{0}, g_n_botsort_reid{0};      // noted pools of the kinds a batch launch must branch for (written under g_pool_mu)
static void count_kind(int kind, int d) {
    if (kind == Y7T_C_BIOU) g_n_cbiou += d;
    else if (kind == Y7T_UAVMOT) g_n_uavmot += d;
    else if (kind == Y7T_STRONGSORT) g_n_strongsort += d;
    else if (kind == Y7T_DEEPMOT) g_n_deepmot += d;
    else if (kind == Y7T_BOTSORT_REID) g_n_botsort_reid += d;
}
static void forget_pool(const void* state) {      // (g_pool_mu held; an address that was never noted changes nothing)
    auto it = g_pools.find(state);
    if (it == g_pools.end()) return;
    count_kind(it->second.kind, -1);
    g_pools.erase(it);
}
static void note_pool(const void* state, int kind, int cap_t, int cap_d) {
    std::lock_guard<std::mutex> l(g_pool_mu);
    forget_pool(state);      // (a pool re-initialised at the same address, maybe with another kind)
    g_pools[state] = PoolInfo{kind, y7t_arena_bytes(cap_t, cap_d), cap_t};
    count_kind(kind, +1);
}
static PoolInfo pool_info(const void* state) {
    std::lock_guard<std::mutex> l(g_pool_mu);
    auto it = g_pools.find(state);
    return it == g_pools.end() ? PoolInfo{-1, 0, 0} : it->second;
}

// the caller is about to free / reuse `state`: forget what the host side knows about it, so that a later blob at the same address is judged by its own
// y7t_tracker_init (the registry only ever grew, and a stale DEEPSORT entry made the plain step refuse a valid pool)
extern "C" int y7t_tracker_release(void* state) {
    std::lock_guard<std::mutex> l(g_pool_mu);
    forget_pool(state);
    return 0;
}

extern "C" size_t y7t_tracker_state_bytes(int cap_t, int cap_d) {
    if (cap_t <= 0 || cap_d <= 0) return 0;
    return y7t_trk_layout(cap_t, cap_d).total;
}

extern "C" int y7t_tracker_init(void* state, size_t state_bytes, int tracker_kind, int kalman_kind, int cap_t, int cap_d,
                                double conf_thresh, double iou_thresh, int max_time_lost, int flags, int* id_counter,
                                y7t_stream stream) {
    Y7T_ARG_CHECK(state && id_counter && cap_t > 0 && cap_d > 0);
    Y7T_ARG_CHECK(tracker_kind == Y7T_SORT || tracker_kind == Y7T_BYTETRACK || tracker_kind == Y7T_BOTSORT || tracker_kind == Y7T_DEEPSORT ||
                  tracker_kind == Y7T_C_BIOU || tracker_kind == Y7T_UAVMOT || tracker_kind == Y7T_STRONGSORT || tracker_kind == Y7T_DEEPMOT || tracker_kind == Y7T_BOTSORT_REID);
    if (tracker_kind == Y7T_C_BIOU) kalman_kind = Y7T_KF_XYAH;      // (C-BIoU has no Kalman filter: the kind is ignored)
    if (tracker_kind == Y7T_DEEPSORT && kalman_kind == Y7T_KF_XYWH) {
        y7t_set_error("DeepSORT gates on xyah measurements (deepsort.py:59): kalman_format default / strongsort only");
        return Y7T_E_ARG;
    }
    if (tracker_kind == Y7T_STRONGSORT && kalman_kind == Y7T_KF_XYWH) {
        y7t_set_error("StrongSORT fuses the IoU of xyah means (strongsort.py:150, track.py:70-71): kalman_format default / strongsort only");
        return Y7T_E_ARG;
    }
    if (tracker_kind == Y7T_BOTSORT_REID && kalman_kind != Y7T_KF_XYWH) {
        y7t_set_error("BoT-SORT runs the xywh filter (track.py:68-69): kalman_format botsort only");
        return Y7T_E_ARG;
    }
    if (!kind_ok(kalman_kind)) { y7t_set_error("kalman kind %d is not implemented on the device", kalman_kind); return Y7T_E_ARG; }
    Y7T_ARG_CHECK(state_bytes >= y7t_trk_layout(cap_t, cap_d).total);
    Y7TTrkCfg c;
    memset(&c, 0, sizeof(c));
    c.tracker = tracker_kind; c.kf = kalman_kind; c.cap_t = cap_t; c.cap_d = cap_d; c.max_time_lost = max_time_lost;
    c.f32_quirk = flags & 1;
    c.det_thresh = conf_thresh;
    c.low_thresh = (conf_thresh - 0.3 > 0.15) ? conf_thresh - 0.3 : 0.15;  // bytetrack.py:15
    c.iou_thresh = iou_thresh;
    hipLaunchKernelGGL(k_tracker_init, dim3(1), dim3(256), 0, S(stream), state, c, (unsigned long long)(uintptr_t)id_counter);
    Y7T_LAUNCH_CHECK();
    note_pool(state, tracker_kind, cap_t, cap_d);
    return 0;
}

static int step_threads(int threads, int n_hint = -1) {
    // measured on MI355X: four waves up to ~384 detections, sixteen beyond (500-object frames 971 us with four waves, 808 us with sixteen).  Round 1
    // chose ONE wave for ~100-object scenes from stand-alone timings (no cross-wave barriers in the LAP reductions); inside the pipeline, where the step
    // runs beside the detector's kernels, four waves hide the longer memory round trips: tracker chain 14.1 -> 12.1 ms per 32 frames on the same box
    // (bench.py --tracker_threads 0 / 256, profiles/r02_bench_variants.txt), and stand-alone they are no slower any more (179 vs 186 us).
    // Round 6: the <= 512-thread launches run instances with the step's body inlined under their own register budget (no scratch spills: k_tracker_step<PROG, MAXT>); 80 objects
    // 169 -> 98 us with four waves (105 with eight), 500 objects 434 us with sixteen waves (the called copy, 128 registers a lane) -> 362 with four -> 261 with eight
    if (threads == 0) return (n_hint > 384) ? 512 : 256;
    if (threads != 64 && threads != 128 && threads != 256 && threads != 512 && threads != 1024) return -1;
    return threads;
}

extern "C" int y7t_kf_multi_gmc_f64(double* mean, double* cov, const double* warp, int N, y7t_stream stream) {
    Y7T_ARG_CHECK(N >= 0);
    if (N == 0) return 0;
    Y7T_ARG_CHECK(mean && cov && warp);
    hipLaunchKernelGGL(k_kf_gmc, dim3((N + 63) / 64), dim3(64), 0, S(stream), mean, cov, warp, N);
    Y7T_LAUNCH_CHECK();
    return 0;
}

// a pool of the wrong kind for an entry point: nothing is stepped, the pool's status word says Y7T_ERR_KIND and the frame has 0 rows (k_tracker_refuse), the error text
// is "<who>: <message>".  state null: no launch (a blob that was never initialised is not touched).  The plain entry points refuse the frames with detections of
// a StrongSORT pool (they belong to y7t_tracker_step_strongsort: the smoothed appearance vectors) and of a DeepMOT pool (y7t_tracker_step_deepmot: the Deep Hungarian
// Net sits between its two programs) through this; a DeepSORT pool's they refuse without touching the pool
static int refuse_pool(const char* who, void* state, int* out_count, y7t_stream stream, const char* fmt, ...) {
    if (state) {
        hipLaunchKernelGGL(k_tracker_refuse, dim3(1), dim3(64), 0, S(stream), state, out_count);
        Y7T_LAUNCH_CHECK();
    }
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    y7t_set_error("%s: %s", who, msg);
    return Y7T_E_STATE;
}
static const char kRefuseStrongsort[] = "this pool was initialised as StrongSORT -- frames with detections go through y7t_tracker_step_strongsort (appearance vectors); only the "
                                        "predict-only step (n < 0) is shared";
static const char kRefuseBotsortReid[] = "this pool was initialised as BoT-SORT with its appearance branch -- frames with detections go through y7t_tracker_step_botsort_reid "
                                         "(appearance vectors); only the predict-only step (n < 0) is shared";
static const char kRefuseDeepmot[] = "this pool was initialised as DeepMOT -- frames with detections go through y7t_tracker_step_deepmot (the Deep Hungarian Net); only the "
                                     "predict-only step (n < 0) is shared";

extern "C" int y7t_tracker_step_batch(void* const* states, const float* const* dets, const int* n_dets, double* const* out_rows,
                                      int* out_count, int out_cap, int batch, int threads, const double* const* gmc_warps,
                                      y7t_stream stream) {
    Y7T_ARG_CHECK(batch >= 0 && out_cap >= 0);
    if (batch == 0) return 0;
    Y7T_ARG_CHECK(states && dets && n_dets && out_rows && out_count);
    const int nt = step_threads(threads);
    Y7T_ARG_CHECK(nt > 0);
    // a C-BIoU or UAVMOT pool may be among the states while one exists in the process: the kernel that branches on each pool's kind.  Above 512 threads only UAVMOT
    // needs it (the called copy of the plain program serves C-BIoU)
    const bool uav = g_n_uavmot.load() > 0, any = nt <= 512 ? (uav || g_n_cbiou.load() > 0) : uav;
    const unsigned lds = kFastBytes + Y7T_LDS_HDR;
    // ... and while a StrongSORT pool or one of BoT-SORT with its appearance branch exists, the kernel that refuses such a pool (status bit 8; it steps through y7t_tracker_step_strongsort / y7t_tracker_step)
    // ... and while a DeepMOT pool exists, the one that refuses its frames with detections as well (they step through y7t_tracker_step_deepmot)
    if (g_n_deepmot.load() > 0) return launch_step<StepBatch<Y7T_PROG_ANY_DM>>(batch, nt, lds, lds, stream, states, dets, n_dets, out_rows, out_count, out_cap, kFastBytes, gmc_warps);
    if (g_n_strongsort.load() > 0 || g_n_botsort_reid.load() > 0) return launch_step<StepBatch<Y7T_PROG_ANY_SS>>(batch, nt, lds, lds, stream, states, dets, n_dets, out_rows, out_count, out_cap, kFastBytes, gmc_warps);
    if (any) return launch_step<StepBatch<Y7T_PROG_ANY>>(batch, nt, lds, lds, stream, states, dets, n_dets, out_rows, out_count, out_cap, kFastBytes, gmc_warps);
    return launch_step<StepBatch<Y7T_PROG_PLAIN>>(batch, nt, lds, lds, stream, states, dets, n_dets, out_rows, out_count, out_cap, kFastBytes, gmc_warps);
}

extern "C" int y7t_tracker_step(void* state, const float* dets, int n, double* out_rows, int out_cap, int* out_count, int threads,
                                const double* gmc_warp, y7t_stream stream) {
    Y7T_ARG_CHECK(state && out_rows && out_count && out_cap >= 0);
    Y7T_ARG_CHECK(n <= 0 || dets);
    const int nt = step_threads(threads, n);
    Y7T_ARG_CHECK(nt > 0);
    const int kind = pool_info(state).kind;
    if (n >= 0 && kind == Y7T_DEEPSORT) {
        y7t_set_error("y7t_tracker_step: this pool was initialised as DeepSORT -- frames with detections go through y7t_tracker_step_deepsort "
                      "(appearance rings); only the predict-only step (n < 0) is shared");
        return Y7T_E_STATE;
    }
    if (n >= 0 && kind == Y7T_STRONGSORT) return refuse_pool("y7t_tracker_step", state, out_count, stream, kRefuseStrongsort);
    if (n >= 0 && kind == Y7T_BOTSORT_REID) return refuse_pool("y7t_tracker_step", state, out_count, stream, kRefuseBotsortReid);      // (its predict-only step is the plain program's: disjoint lists)
    if (n >= 0 && kind == Y7T_DEEPMOT) return refuse_pool("y7t_tracker_step", state, out_count, stream, kRefuseDeepmot);      // (its predict-only step is the plain program's: default below)
    const unsigned fb = step_fast_bytes(n), lds_max = kFastBytes + Y7T_LDS_HDR;
    switch (kind) {
    // (predict-only: StrongSORT's own program without a feature state -- its lists may share a track, which its pool holds once, as joint_stracks does)
    case Y7T_STRONGSORT: return launch_step<StepStrongsort>(1, nt, lds_max, fb + Y7T_LDS_HDR, stream, state, (void*)nullptr, (const float*)nullptr, -1, (const float*)nullptr, out_rows, out_cap, out_count, fb, (const double*)nullptr);
    case Y7T_UAVMOT: return launch_step<StepSingle<Y7T_PROG_UAVMOT>>(1, nt, lds_max, fb + Y7T_LDS_HDR, stream, state, dets, n, out_rows, out_cap, out_count, fb, gmc_warp);
    case Y7T_C_BIOU: return launch_step<StepSingle<Y7T_PROG_CBIOU>>(1, nt, lds_max, fb + Y7T_LDS_HDR, stream, state, dets, n, out_rows, out_cap, out_count, fb, gmc_warp);
    default: return launch_step<StepSingle<Y7T_PROG_PLAIN>>(1, nt, lds_max, fb + Y7T_LDS_HDR, stream, state, dets, n, out_rows, out_cap, out_count, fb, gmc_warp);
    }
}

extern "C" int y7t_tracker_step_frames(void* state, const float* const* dets, const int* n_dets, double* const* out_rows, int* const* out_count, int out_cap,
                                       int n_frames, int threads, const double* const* gmc_warps, y7t_stream stream) {
    Y7T_ARG_CHECK(state && out_cap >= 0 && n_frames >= 0);
    if (n_frames == 0) return 0;
    Y7T_ARG_CHECK(dets && n_dets && out_rows && out_count);
    const int nt = step_threads(threads);
    Y7T_ARG_CHECK(nt > 0);
    const PoolInfo pool = pool_info(state);
    if (pool.kind == Y7T_DEEPSORT) {
        y7t_set_error("y7t_tracker_step_frames: a DeepSORT pool steps through y7t_tracker_step_deepsort (appearance rings)");
        return Y7T_E_STATE;
    }
    if (pool.kind == Y7T_DEEPMOT) return refuse_pool("y7t_tracker_step_frames", state, nullptr, stream, kRefuseDeepmot);
    if (pool.kind == Y7T_BOTSORT_REID) return refuse_pool("y7t_tracker_step_frames", state, nullptr, stream, kRefuseBotsortReid);
    if (pool.kind == Y7T_STRONGSORT) return refuse_pool("y7t_tracker_step_frames", state, nullptr, stream, kRefuseStrongsort);      // (the frames' counts are device arrays: none is written)
    // LDS of the launch: header | fast scratch (cost matrix, assignment work arrays) | the pool's index lists for the length of the launch (y7t_arena_*), when the
    // CU's 160 KiB hold them beside at least 64 KiB of fast scratch (the default capacities, 1024 tracks x 1024 detections: 68 KiB of lists, 91 KiB of scratch)
    static const unsigned kLdsMax = 160 * 1024;
    static const int use_arena = y7t_switch("Y7T_TRACKER_ARENA", 1);      // (thread-safe static initialisation)
    const size_t ab = use_arena ? pool.arena_bytes : 0;
    unsigned arena = 0, fast = kFastBytes;
    if (ab && ab + 64 * 1024 + Y7T_LDS_HDR <= kLdsMax) { arena = (unsigned)((ab + 15) & ~(size_t)15); fast = (kLdsMax - Y7T_LDS_HDR - arena) & ~15u; if (fast > kFastBytes) fast = kFastBytes; }
    const unsigned lds = Y7T_LDS_HDR + fast + arena;
    switch (pool.kind) {
    case Y7T_UAVMOT: return launch_step<StepFrames<Y7T_PROG_UAVMOT>>(1, nt, kLdsMax, lds, stream, state, dets, n_dets, out_rows, out_count, out_cap, n_frames, fast, arena, gmc_warps);
    case Y7T_C_BIOU: return launch_step<StepFrames<Y7T_PROG_CBIOU>>(1, nt, kLdsMax, lds, stream, state, dets, n_dets, out_rows, out_count, out_cap, n_frames, fast, arena, gmc_warps);
    default: return launch_step<StepFrames<Y7T_PROG_PLAIN>>(1, nt, kLdsMax, lds, stream, state, dets, n_dets, out_rows, out_count, out_cap, n_frames, fast, arena, gmc_warps);
    }
}

// The host part of a frame that the appearance trackers' entry points share (DeepSORT, StrongSORT, BoT-SORT with ReID; each checks its own arguments first, in the
// order it always did): the thread count, the pool's kind (`refuse`: 0, or what the entry point returns for another tracker's pool), then FAMILY's step between the frame's
// appearance launches (`before`) and its store launch (`after`) -- a frame without detections takes neither.  warp: the step's camera-motion argument, where it has one.
template <class FAMILY, class Refuse, class Before, class After, class... W>
static int step_appearance(void* state, void* feat_state, const float* dets, int n, const float* det_feats, double* out_rows, int out_cap, int* out_count, int threads,
                           y7t_stream stream, Refuse refuse /* (const PoolInfo&) */, Before before /* (const PoolInfo&) */, After after, W... warp) {
    const int nt = step_threads(threads, n);
    Y7T_ARG_CHECK(nt > 0);
    const PoolInfo pool = pool_info(state);
    if (int e = refuse(pool)) return e;
    if (n > 0) { if (int e = before(pool)) return e; }
    const unsigned fb = step_fast_bytes(n);
    if (int e = launch_step<FAMILY>(1, nt, kFastBytes + Y7T_LDS_HDR, fb + Y7T_LDS_HDR, stream, state, feat_state, dets, n, det_feats, out_rows, out_cap, out_count, fb, warp...)) return e;
    if (n > 0) { if (int e = after()) return e; }
    return 0;
}

extern "C" size_t y7t_deepsort_feature_bytes(int cap_t, int cap_d, int feat_dim, int budget) {
    if (cap_t <= 0 || cap_d <= 0 || feat_dim <= 0 || budget <= 0) return 0;
    return y7t_feat_layout(cap_t, cap_d, feat_dim, budget).total;
}

extern "C" int y7t_deepsort_init(void* feat_state, size_t bytes, int cap_t, int cap_d, int feat_dim, int budget, y7t_stream stream) {
    Y7T_ARG_CHECK(feat_state && cap_t > 0 && cap_d > 0 && feat_dim > 0 && budget > 0);
    Y7T_ARG_CHECK(bytes >= y7t_feat_layout(cap_t, cap_d, feat_dim, budget).total);
    hipLaunchKernelGGL(k_feat_init, dim3(1), dim3(256), 0, S(stream), feat_state, cap_t, cap_d, feat_dim, budget);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_tracker_step_deepsort(void* state, void* feat_state, int cap_tracks, const float* dets, int n, const float* det_feats,
                                         double* out_rows, int out_cap, int* out_count, int threads, y7t_stream stream) {
    Y7T_ARG_CHECK(state && feat_state && out_rows && out_count && out_cap >= 0 && cap_tracks > 0 && n >= 0);
    Y7T_ARG_CHECK(n == 0 || (dets && det_feats));
    Y7T_ARG_CHECK(cap_tracks <= 64 * Y7T_EMBED_WORKERS);      // (k_embed_dist: a workgroup owns at most 64 live slots)
    return step_appearance<StepDeepsort>(state, feat_state, dets, n, det_feats, out_rows, out_cap, out_count, threads, stream,
        [&](const PoolInfo& pool) -> int {
            const int kind = pool.kind;
            if (kind == Y7T_C_BIOU || kind == Y7T_UAVMOT || kind == Y7T_STRONGSORT || kind == Y7T_DEEPMOT || kind == Y7T_BOTSORT_REID)      // no appearance rings: the pool's status says Y7T_ERR_KIND, nothing is stepped
                return refuse_pool("y7t_tracker_step_deepsort", state, out_count, stream, "this pool was initialised as %s -- it steps through y7t_tracker_step",
                                   kind == Y7T_C_BIOU ? "C-BIoU" : kind == Y7T_UAVMOT ? "UAVMOT" : kind == Y7T_DEEPMOT ? "DeepMOT (y7t_tracker_step_deepmot)" : kind == Y7T_BOTSORT_REID ? "BoT-SORT with ReID (y7t_tracker_step_botsort_reid)" : "StrongSORT (y7t_tracker_step_strongsort)");
            return 0;
        },
        [&](const PoolInfo&) -> int {
            hipLaunchKernelGGL(k_ds_normalize, dim3((n + 3) / 4), dim3(256), 0, S(stream), feat_state, det_feats, n);      // a wave per detection
            Y7T_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_embed_dist, dim3(cap_tracks < Y7T_EMBED_WORKERS ? cap_tracks : Y7T_EMBED_WORKERS, (n + 63) / 64), dim3(256), 0, S(stream), state, feat_state, n);
            Y7T_LAUNCH_CHECK();
            return 0;
        },
        [&]() -> int { hipLaunchKernelGGL(k_ds_store, dim3((n + 3) / 4), dim3(256), 0, S(stream), feat_state, det_feats); Y7T_LAUNCH_CHECK(); return 0; });
}

extern "C" size_t y7t_strongsort_feature_bytes(int cap_t, int cap_d, int feat_dim) {
    if (cap_t <= 0 || cap_d <= 0 || feat_dim <= 0) return 0;
    return y7t_ss_layout(cap_t, cap_d, feat_dim).total;
}

extern "C" int y7t_strongsort_init(void* feat_state, size_t bytes, int cap_t, int cap_d, int feat_dim, double gamma, y7t_stream stream) {
    Y7T_ARG_CHECK(feat_state && cap_t > 0 && cap_d > 0 && feat_dim > 0);
    Y7T_ARG_CHECK(bytes >= y7t_ss_layout(cap_t, cap_d, feat_dim).total);
    hipLaunchKernelGGL(k_ss_init, dim3(1), dim3(64), 0, S(stream), feat_state, cap_t, cap_d, feat_dim, gamma);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_tracker_step_strongsort(void* state, void* feat_state, const float* dets, int n, const float* det_feats, double* out_rows, int out_cap,
                                           int* out_count, int threads, const double* gmc_warp, y7t_stream stream) {
    Y7T_ARG_CHECK(state && feat_state && out_rows && out_count && out_cap >= 0 && n >= 0);
    Y7T_ARG_CHECK(n == 0 || (dets && det_feats));
    return step_appearance<StepStrongsort>(state, feat_state, dets, n, det_feats, out_rows, out_cap, out_count, threads, stream,
        [&](const PoolInfo& pool) -> int {      // another tracker's pool: its status says Y7T_ERR_KIND, nothing is stepped (a blob that was never initialised is not touched)
            return pool.kind == Y7T_STRONGSORT ? 0 : refuse_pool("y7t_tracker_step_strongsort", pool.kind >= 0 ? state : nullptr, out_count, stream, "this pool was not initialised as StrongSORT (tracker kind %d)", pool.kind);
        },
        [&](const PoolInfo& pool) -> int {
            const int groups = (pool.cap_t + 31) / 32;
            const int vec_ok = (((uintptr_t)feat_state | (uintptr_t)det_feats) & 15) == 0;
            hipLaunchKernelGGL(k_ss_appearance, dim3(groups < Y7T_SS_WORKERS ? groups : Y7T_SS_WORKERS, (n + 63) / 64), dim3(256), 0, S(stream), state, feat_state, dets, det_feats, n, vec_ok);
            Y7T_LAUNCH_CHECK();
            return 0;
        },
        [&]() -> int { hipLaunchKernelGGL(k_ss_store, dim3((n + 3) / 4), dim3(256), 0, S(stream), feat_state, det_feats); Y7T_LAUNCH_CHECK(); return 0; }, gmc_warp);      // a wave per queued vector (at most one per detection)
}

extern "C" size_t y7t_botsort_reid_feature_bytes(int cap_t, int cap_d, int feat_dim) {
    if (cap_t <= 0 || cap_d <= 0 || feat_dim <= 0 || feat_dim > 65536) return 0;
    return y7t_br_layout(cap_t, cap_d, feat_dim).total;
}

extern "C" int y7t_botsort_reid_init(void* feat_state, size_t bytes, int cap_t, int cap_d, int feat_dim, double theta_iou, double theta_emb, y7t_stream stream) {
    Y7T_ARG_CHECK(feat_state && cap_t > 0 && cap_d > 0 && feat_dim > 0 && feat_dim <= 65536);
    Y7T_ARG_CHECK((long long)cap_t * cap_d < (1ll << 31));      // (a pair's table key is row * columns + column)
    Y7T_ARG_CHECK(theta_iou < 1.0);                             // (a pair of boxes apart costs exactly 1 and takes no cosine: what the pair pass is built on)
    Y7T_ARG_CHECK(bytes >= y7t_br_layout(cap_t, cap_d, feat_dim).total);
    hipLaunchKernelGGL(k_br_init, dim3(1), dim3(64), 0, S(stream), feat_state, cap_t, cap_d, feat_dim, theta_iou, theta_emb);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_tracker_step_botsort_reid(void* state, void* feat_state, const float* dets, int n, const float* det_feats, double* out_rows, int out_cap,
                                             int* out_count, int threads, const double* gmc_warp, y7t_stream stream) {
    Y7T_ARG_CHECK(state && feat_state && out_rows && out_count && out_cap >= 0 && n >= 0);
    Y7T_ARG_CHECK(n == 0 || (dets && det_feats));
    return step_appearance<StepBotsortReid>(state, feat_state, dets, n, det_feats, out_rows, out_cap, out_count, threads, stream,
        [&](const PoolInfo& pool) -> int {      // another tracker's pool: its status says Y7T_ERR_KIND, nothing is stepped (a blob that was never initialised is not touched)
            return pool.kind == Y7T_BOTSORT_REID ? 0 : refuse_pool("y7t_tracker_step_botsort_reid", pool.kind >= 0 ? state : nullptr, out_count, stream, "this pool was not initialised as BoT-SORT with its appearance branch (tracker kind %d)", pool.kind);
        },
        [&](const PoolInfo& pool) -> int {   // a wave per row: the live slots (at most cap_tracks) and the frame's detections; a frame without detections takes no cosine
            const int rows = pool.cap_t + n, blocks = (rows + 3) / 4;
            hipLaunchKernelGGL(k_br_prepare, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, S(stream), state, feat_state, dets, det_feats, n);
            Y7T_LAUNCH_CHECK();
            return 0;
        },
        [&]() -> int { hipLaunchKernelGGL(k_br_store, dim3((n + 3) / 4), dim3(256), 0, S(stream), feat_state, det_feats); Y7T_LAUNCH_CHECK(); return 0; }, gmc_warp);      // a wave per queued vector (at most two per detection)
}

// DeepMOT.update for one frame: the front program, the Deep Hungarian Net on the pool x high-detection matrix it wrote (skipped where either side is empty), the back
// program.  The network's launches depend on the matrix's size, which only the device knows: the call reads two ints back between the front program and the network, and
// the network's status word at the end -- it returns when the frame is done (a frame's network takes milliseconds: four passes of h x w sequential steps).
extern "C" int y7t_tracker_step_deepmot(void* state, void* dhn, const float* dets, int n, int img_h, int img_w, double* out_rows, int out_cap, int* out_count, int threads,
                                        y7t_stream stream) {
    Y7T_ARG_CHECK(state && dhn && out_rows && out_count && out_cap >= 0 && n >= 0 && img_h > 0 && img_w > 0);
    Y7T_ARG_CHECK(n == 0 || dets);
    const int nt = step_threads(threads, n);
    Y7T_ARG_CHECK(nt > 0);
    const PoolInfo pool = pool_info(state);
    if (pool.kind != Y7T_DEEPMOT)      // another tracker's pool: its status says Y7T_ERR_KIND, nothing is stepped (a blob that was never initialised is not touched)
        return refuse_pool("y7t_tracker_step_deepmot", pool.kind >= 0 ? state : nullptr, out_count, stream, "this pool was not initialised as DeepMOT (tracker kind %d)", pool.kind);
    Y7TDhnView v;
    if (int e = y7t_dhn_view(dhn, &v)) return e;
    const unsigned fb = step_fast_bytes(n), lds_max = kFastBytes + Y7T_LDS_HDR;
    if (int e = launch_step<StepDeepmotFront>(1, nt, lds_max, fb + Y7T_LDS_HDR, stream, state, dets, n, img_h, img_w, v.D, (long long)v.max_h * v.max_w, v.hw, fb)) return e;
    int hw[2] = {0, 0};
    Y7T_HIP_CHECK(hipMemcpyAsync(hw, v.hw, sizeof(hw), hipMemcpyDeviceToHost, S(stream)));
    Y7T_HIP_CHECK(hipStreamSynchronize(S(stream)));
    const bool net = hw[0] > 0 && hw[1] > 0;
    if (net) { if (int e = y7t_dhn_enqueue(dhn, v.D, hw[0], hw[1], v.out, S(stream))) return e; }
    if (int e = launch_step<StepDeepmotBack>(1, nt, lds_max, fb + Y7T_LDS_HDR, stream, state, dets, (const float*)v.out, (const unsigned*)(net ? v.status : nullptr), out_rows, out_cap, out_count, fb)) return e;
    if (net) {
        unsigned status = 0;
        Y7T_HIP_CHECK(hipMemcpyAsync(&status, v.status, 4, hipMemcpyDeviceToHost, S(stream)));
        Y7T_HIP_CHECK(hipStreamSynchronize(S(stream)));
        if (status) {
            y7t_set_error("y7t_tracker_step_deepmot: the Deep Hungarian Net's forward gave up waiting for a peer workgroup (status %u); the frame produced no rows", status);
            return Y7T_E_STATE;
        }
    }
    return 0;
}

static const char* kFieldNames[] = {"mean", "cov", "box", "score", "cls", "tid", "start", "frame", "tsu", "state", "act", "len",
                                    "inrem", "f32m", "tracked", "lost", "hdr_frame_id", "hdr_n_tracked", "hdr_n_lost",
                                    "hdr_status", "hdr_n_out", "hdr_n_removed_total", "hdr_prof", "total"};

extern "C" const char* y7t_tracker_field_name(int i) {
    const int n = (int)(sizeof(kFieldNames) / sizeof(kFieldNames[0]));
    return (i >= 0 && i < n) ? kFieldNames[i] : nullptr;
}

extern "C" int y7t_tracker_layout(int cap_t, int cap_d, int64_t* offsets, int max_fields) {
    const int n = (int)(sizeof(kFieldNames) / sizeof(kFieldNames[0]));
    if (!offsets || max_fields < n || cap_t <= 0 || cap_d <= 0) return n;
    const Y7TTrkLayout L = y7t_trk_layout(cap_t, cap_d);
    const size_t v[] = {L.mean, L.cov, L.box, L.score, L.cls, L.tid, L.start, L.frame, L.tsu, L.state, L.act, L.len, L.inrem, L.f32m,
                        L.tracked, L.lost, offsetof(Y7TTrkHdr, frame_id), offsetof(Y7TTrkHdr, n_tracked), offsetof(Y7TTrkHdr, n_lost),
                        offsetof(Y7TTrkHdr, status), offsetof(Y7TTrkHdr, n_out), offsetof(Y7TTrkHdr, n_removed_total), offsetof(Y7TTrkHdr, prof), L.total};
    for (int i = 0; i < n; ++i) offsets[i] = (int64_t)v[i];
    return n;
}
