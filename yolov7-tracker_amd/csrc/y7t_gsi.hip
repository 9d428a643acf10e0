// y7t_gsi.hip -- GSI, the Gaussian-smoothed interpolation of StrongSORT++, as gfx950 kernels (csrc/y7t_gsi.h states the arithmetic and the per-track program;
// DESIGN.md section 4 "GSI" is the specification and tests/gsi_np.py its NumPy restatement).  float64 throughout, contraction off.
//
// Interpolation, three launches, nothing read back, no atomics:
//   k_gsi_count     a workgroup per track: rows after filling = rows + sum of the admitted gaps  -> offsets_out[track + 1]
//   k_gsi_scan      one workgroup: the inclusive scan of those counts in place (offsets_out[0] = 0), the total and the status word
//   k_gsi_write     a workgroup per track: an ordered scan over its rows gives every row its place; a thread writes its row and the frames it fills behind it
// Smoothing: every track is its own dense symmetric positive-definite system A = K + reg I of its own length with four right-hand sides.
//   k_gsi_prepare   out = the columns as they came, status = PENDING: a track no launch reaches stays visible as such
//   k_gsi_classify  one workgroup: the rank of every track among the tracks of its padded-length class (<= 128 rows, 256, 512, ... 4096), in table order
//   k_gsi_smooth<true>   class 0: a workgroup per track, the triangle in the LDS (128 rows of 130 doubles: 130 KiB)
//   k_gsi_smooth<false>  class c >= 1: a workgroup per track, the triangle in a slot of the object's pool in HBM; launches of `slots` tracks each, by rank
// A workgroup never waits for another one; a track's result depends on its rows alone, not on its slot, its launch or its neighbours.  Inside the workgroup:
// y7t_gsi_track (blocked right-looking Cholesky in panels of 16, the trailing update on v_mfma_f64_16x16x4_f64; two triangular solves; K a with K recomputed).
#include "y7t_gsi.h"
#include "y7t_common.h"
#include <mutex>
#include <unordered_map>

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static const size_t kPoolBudget = (size_t)512 << 20;      // bytes of the pool one class may take: 3 slots of 4096 rows, 15 of 2048, 63 of 1024, ...

static size_t slot_doubles(int c) { const size_t cap = (size_t)Y7T_GSI_LDS_LEN << c; return cap * cap + 4 * cap; }

struct GsiLayout { size_t rank, pool, total; int slots[Y7T_GSI_CLASSES]; };
static GsiLayout gsi_layout(int max_tracks, int max_rows, int max_len) {
    GsiLayout L;
    size_t o = 256;      // (a header nothing polls)
    L.rank = o; o = al256(o + (size_t)max_tracks * 4);
    L.pool = o;
    size_t pool = 0;
    L.slots[0] = 0;
    for (int c = 1; c < Y7T_GSI_CLASSES; ++c) {
        const int lo = (Y7T_GSI_LDS_LEN << (c - 1)) + 1;      // the shortest track of the class
        int possible = lo <= max_len ? max_rows / lo : 0;
        if (possible > max_tracks) possible = max_tracks;
        const size_t bytes = slot_doubles(c) * 8;
        size_t fit = kPoolBudget / bytes;
        if (fit < 1) fit = 1;
        L.slots[c] = possible < (int)fit ? possible : (int)fit;
        if ((size_t)L.slots[c] * bytes > pool) pool = (size_t)L.slots[c] * bytes;
    }
    L.total = al256(o + pool);
    return L;
}

// ---- interpolation ----
__global__ void __launch_bounds__(256) k_gsi_count(const double* __restrict__ runs, const int* __restrict__ off, int interval, int* __restrict__ off_out) {
    __shared__ int red[256];
    const int trk = blockIdx.x, tid = threadIdx.x, r0 = off[trk], n = off[trk + 1] - r0;
    int c = 0;
    for (int r = tid; r < n; r += 256) c += 1 + (r + 1 < n ? y7t_gsi_fill(runs[(size_t)(r0 + r) * Y7T_GSI_COLS], runs[(size_t)(r0 + r + 1) * Y7T_GSI_COLS], interval) : 0);
    red[tid] = c;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) off_out[trk + 1] = red[0];
}

__global__ void __launch_bounds__(256) k_gsi_scan(int* __restrict__ off_out, int T, int max_rows, int max_len, int* __restrict__ count_out, int* __restrict__ status_out) {
    __shared__ long long part[256];
    __shared__ int longf[256];
    const int tid = threadIdx.x, seg = (T + 255) / 256, lo = tid * seg, hi = lo + seg < T ? lo + seg : T;
    long long s = 0;
    int lf = 0;
    for (int i = lo; i < hi; ++i) { const int c = off_out[i + 1]; s += c; lf |= c > max_len ? 1 : 0; }
    part[tid] = s;
    longf[tid] = lf;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        int any = 0;
        for (int k = 0; k < 256; ++k) { const long long v = part[k]; part[k] = run; run += v; any |= longf[k]; }
        off_out[0] = 0;
        count_out[0] = run > 0x7fffffffLL ? 0x7fffffff : (int)run;
        status_out[0] = (run > max_rows ? Y7T_GSI_ROWS_OVERFLOW : 0) | (any ? Y7T_GSI_LEN_OVERFLOW : 0);
    }
    __syncthreads();
    long long run = part[tid];
    for (int i = lo; i < hi; ++i) { run += off_out[i + 1]; off_out[i + 1] = run > 0x7fffffffLL ? 0x7fffffff : (int)run; }
}

__global__ void __launch_bounds__(256) k_gsi_write(const double* __restrict__ runs, const int* __restrict__ off, int interval, const int* __restrict__ off_out, int max_rows,
                                                   double* __restrict__ runs_out, int* __restrict__ src_out) {
    __shared__ int sc[256];
    const int trk = blockIdx.x, tid = threadIdx.x, r0 = off[trk], n = off[trk + 1] - r0;
    long long base = off_out[trk];
    for (int q0 = 0; q0 < n; q0 += 256) {      // (n is the workgroup's: every barrier below is reached by all of it)
        const int r = q0 + tid;
        const double* a = runs + (size_t)(r0 + (r < n ? r : 0)) * Y7T_GSI_COLS;
        const double* b = a + Y7T_GSI_COLS;
        const int fill = r + 1 < n ? y7t_gsi_fill(a[0], b[0], interval) : 0;
        const int e = r < n ? 1 + fill : 0;
        sc[tid] = e;
        __syncthreads();
        for (int w = 1; w < 256; w <<= 1) {
            const int v = tid >= w ? sc[tid - w] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const long long pos = base + sc[tid] - e;
        if (r < n) {
            for (int i = 0; i <= fill; ++i) {
                const long long o = pos + i;
                if (o >= max_rows) break;
                double* d = runs_out + (size_t)o * Y7T_GSI_COLS;
                if (i == 0) {
                    for (int c = 0; c < Y7T_GSI_COLS; ++c) d[c] = a[c];
                } else {
                    const double span = b[0] - a[0];
                    d[0] = a[0] + (double)i;
                    for (int c = 1; c < Y7T_GSI_COLS; ++c) d[c] = y7t_gsi_lerp(a[c], b[c], span, (double)i);
                }
                src_out[o] = r0 + r;
            }
        }
        base += sc[255];
        __syncthreads();
    }
}

// ---- smoothing ----
__global__ void __launch_bounds__(256) k_gsi_prepare(const double* __restrict__ runs, const int* __restrict__ off, int longest, double* __restrict__ out,
                                                     int* __restrict__ status) {
    const int trk = blockIdx.x, r0 = off[trk], n = off[trk + 1] - r0;
    for (int e = threadIdx.x; e < n * 4; e += 256) out[(size_t)r0 * 4 + e] = runs[(size_t)(r0 + (e >> 2)) * Y7T_GSI_COLS + 1 + (e & 3)];
    if (threadIdx.x == 0) status[trk] = n < 1 ? 0 : (n > longest ? Y7T_GSI_TOO_LONG : Y7T_GSI_PENDING);
}

__global__ void __launch_bounds__(64) k_gsi_classify(const int* __restrict__ off, int t0, int m, int longest, int* __restrict__ rank) {
    const int c = threadIdx.x;
    if (c >= Y7T_GSI_CLASSES) return;
    int cnt = 0;
    for (int i = 0; i < m; ++i) {
        const int n = off[t0 + i + 1] - off[t0 + i];
        const bool live = n >= 1 && n <= longest;
        if (!live) { if (c == 0) rank[i] = -1; continue; }
        if (y7t_gsi_class(n) == c) rank[i] = cnt++;
    }
}

extern __shared__ __attribute__((aligned(16))) double y7t_gsi_smem[];
enum { kLdsLd = Y7T_GSI_LDS_LEN + Y7T_GSI_LDS_PAD };
static const unsigned kLdsBytesLds = (Y7T_GSI_LDS_LEN + 272 + 4 * Y7T_GSI_LDS_LEN + Y7T_GSI_LDS_LEN * kLdsLd) * 8;
static const unsigned kLdsBytesHbm = (Y7T_GSI_MAX_LEN + 272) * 8;

template <bool LDS>
__global__ void __launch_bounds__(256) k_gsi_smooth(const double* __restrict__ runs, const int* __restrict__ off, const double* __restrict__ len_scale, int t0, int longest,
                                                    double reg, int cls, int round, int slots, double* __restrict__ pool, size_t slot_stride,
                                                    const int* __restrict__ rank, double* __restrict__ out, int* __restrict__ status) {
    // (every return below is the whole workgroup's: it depends on blockIdx alone)
    const int trk = t0 + blockIdx.x, r0 = off[trk], n = off[trk + 1] - r0;
    if (n < 1 || n > longest || n > Y7T_GSI_MAX_LEN || y7t_gsi_class(n) != cls) return;
    const int np = y7t_gsi_pad(n);
    double *t, *D, *Y, *A;
    size_t ld;
    if (LDS) {
        t = y7t_gsi_smem; D = t + Y7T_GSI_LDS_LEN; Y = D + 272; A = Y + 4 * Y7T_GSI_LDS_LEN; ld = kLdsLd;
    } else {
        const int r = rank[blockIdx.x];
        if (r < 0 || r / slots != round) return;
        t = y7t_gsi_smem; D = t + Y7T_GSI_MAX_LEN;
        A = pool + (size_t)(r % slots) * slot_stride; Y = A + (size_t)np * np; ld = np;
    }
    Y7TGsiExec ex;
    ex.tid = threadIdx.x; ex.nt = 256; ex.wave = threadIdx.x >> 6; ex.nw = 4; ex.lane = threadIdx.x & 63; ex.nl = 64;
    const int st = y7t_gsi_track(ex, A, ld, Y, t, D, runs + (size_t)r0 * Y7T_GSI_COLS, n, len_scale[trk], reg, out + (size_t)r0 * 4);
    if (threadIdx.x == 0) status[trk] = st;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct GsiInfo { int max_tracks, max_rows, max_len; };
static std::mutex g_gsi_mu;
static std::unordered_map<const void*, GsiInfo> g_gsis;
static Y7TOncePerDevice g_gsi_lds_once;

static bool caps_ok(int max_tracks, int max_rows, int max_len) {
    return max_tracks >= 1 && max_tracks <= Y7T_GSI_MAX_TRACKS && max_rows >= 1 && max_len >= 1 && max_len <= Y7T_GSI_MAX_LEN;
}

extern "C" size_t y7t_gsi_workspace_bytes(int max_tracks, int max_rows, int max_len) {
    if (!caps_ok(max_tracks, max_rows, max_len)) return 0;
    return gsi_layout(max_tracks, max_rows, max_len).total;
}

extern "C" int y7t_gsi_init(void* obj, size_t bytes, int max_tracks, int max_rows, int max_len, y7t_stream stream) {
    Y7T_ARG_CHECK(obj);
    Y7T_ARG_CHECK(caps_ok(max_tracks, max_rows, max_len));
    Y7T_ARG_CHECK(((uintptr_t)obj & 255) == 0);
    Y7T_ARG_CHECK(bytes >= gsi_layout(max_tracks, max_rows, max_len).total);
    Y7T_HIP_CHECK(hipMemsetAsync(obj, 0, 256, (hipStream_t)stream));
    std::lock_guard<std::mutex> l(g_gsi_mu);
    g_gsis[obj] = GsiInfo{max_tracks, max_rows, max_len};
    return 0;
}

extern "C" int y7t_gsi_release(void* obj) {
    std::lock_guard<std::mutex> l(g_gsi_mu);
    g_gsis.erase(obj);
    return 0;
}

static int gsi_info(const void* obj, GsiInfo* info) {
    std::lock_guard<std::mutex> l(g_gsi_mu);
    auto it = g_gsis.find(obj);
    if (it == g_gsis.end()) { y7t_set_error("this address holds no GSI object (y7t_gsi_init)"); return Y7T_E_STATE; }
    *info = it->second;
    return 0;
}

extern "C" int y7t_gsi_interpolate(void* obj, const double* runs, const int* offsets, int n_tracks, int interval, double* runs_out, int* offsets_out, int* src_out,
                                   int* count_out, int* status_out, y7t_stream stream) {
    GsiInfo info;
    if (int e = gsi_info(obj, &info)) return e;
    Y7T_ARG_CHECK(n_tracks >= 0 && interval >= 0 && offsets && offsets_out && count_out && status_out && (n_tracks == 0 || (runs && runs_out && src_out)));
    hipStream_t st = (hipStream_t)stream;
    if (n_tracks == 0) {
        Y7T_HIP_CHECK(hipMemsetAsync(offsets_out, 0, 4, st));
        Y7T_HIP_CHECK(hipMemsetAsync(count_out, 0, 4, st));
        Y7T_HIP_CHECK(hipMemsetAsync(status_out, 0, 4, st));
        return 0;
    }
    hipLaunchKernelGGL(k_gsi_count, dim3(n_tracks), dim3(256), 0, st, runs, offsets, interval, offsets_out);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gsi_scan, dim3(1), dim3(256), 0, st, offsets_out, n_tracks, info.max_rows, info.max_len, count_out, status_out);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gsi_write, dim3(n_tracks), dim3(256), 0, st, runs, offsets, interval, offsets_out, info.max_rows, runs_out, src_out);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_gsi_smooth(void* obj, const double* runs, const int* offsets, const double* len_scale, int n_tracks, int longest, double reg, double* out,
                              int* status_out, y7t_stream stream) {
    GsiInfo info;
    if (int e = gsi_info(obj, &info)) return e;
    Y7T_ARG_CHECK(n_tracks >= 0 && longest >= 0 && reg >= 0.0 && offsets && (n_tracks == 0 || (runs && len_scale && out && status_out)));
    if (longest > info.max_len) {
        y7t_set_error("y7t_gsi_smooth: a track of %d rows exceeds this object's capacity (max_len = %d)", longest, info.max_len);
        return Y7T_E_CAPACITY;
    }
    if (n_tracks == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (int e = y7t_set_max_lds(g_gsi_lds_once, (int)kLdsBytesLds, k_gsi_smooth<true>)) return e;
    const GsiLayout L = gsi_layout(info.max_tracks, info.max_rows, info.max_len);
    int* rank = (int*)((char*)obj + L.rank);
    double* pool = (double*)((char*)obj + L.pool);
    hipLaunchKernelGGL(k_gsi_prepare, dim3(n_tracks), dim3(256), 0, st, runs, offsets, longest, out, status_out);
    Y7T_LAUNCH_CHECK();
    if (longest < 1) return 0;
    const int cmax = y7t_gsi_class(longest);
    for (int t0 = 0; t0 < n_tracks; t0 += info.max_tracks) {
        const int m = n_tracks - t0 < info.max_tracks ? n_tracks - t0 : info.max_tracks;
        hipLaunchKernelGGL(k_gsi_smooth<true>, dim3(m), dim3(256), kLdsBytesLds, st, runs, offsets, len_scale, t0, longest, reg, 0, 0, 1, pool, (size_t)0, rank, out, status_out);
        Y7T_LAUNCH_CHECK();
        if (cmax < 1) continue;
        hipLaunchKernelGGL(k_gsi_classify, dim3(1), dim3(64), 0, st, offsets, t0, m, longest, rank);
        Y7T_LAUNCH_CHECK();
        for (int c = 1; c <= cmax; ++c) {
            // the most tracks of this class the table can hold; launches of `slots` of them each, by rank (a launch nobody belongs to leaves at once)
            const int lo = (Y7T_GSI_LDS_LEN << (c - 1)) + 1, slots = L.slots[c];
            int possible = info.max_rows / lo;
            if (possible > m) possible = m;
            if (possible < 1 || slots < 1) continue;
            for (int round = 0; round * slots < possible; ++round) {
                hipLaunchKernelGGL(k_gsi_smooth<false>, dim3(m), dim3(256), kLdsBytesHbm, st, runs, offsets, len_scale, t0, longest, reg, c, round, slots, pool, slot_doubles(c),
                                   rank, out, status_out);
                Y7T_LAUNCH_CHECK();
            }
        }
    }
    return 0;
}
