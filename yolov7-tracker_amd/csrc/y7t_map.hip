// y7t_map.hip -- the detector's mAP evaluation as gfx950 kernels (csrc/y7t_map.h states the arithmetic and the two workgroup programs; DESIGN.md section 4 "mAP
// evaluation" is the specification and tests/map_np.py its restatement).  Nothing is read back and there are no atomics: every element has one writer.
//
// y7t_map_update, two launches:
//   k_map_update    a workgroup per image: y7t_map_image; its rows go behind the count kept on the device plus the exclusive prefix of ndets
//   k_map_commit    a thread per class: nt[c] += the batch's targets of class c; one thread moves the row count, the images seen and the status word
// y7t_map_compute:
//   k_map_keys      key = (class, ~confidence) of every stored row, index = its arrival order
//   per digit (four of the confidence, one or two of the class), least significant first:
//     k_map_hist    a workgroup per tile of 256 rows: its digit histogram, hist[digit][tile]
//     k_map_scan    one workgroup: the exclusive scan of hist in (digit, tile) order
//     k_map_scatter a workgroup per tile: a row goes to hist[digit][tile] + the rows of the tile before it with the same digit -- a stable scatter
//   k_map_gather    confidence and correct mask in sorted order
//   k_map_segments  a thread per class: the first sorted row of the class (a binary search on the keys)
//   k_map_curve     a workgroup per (class, threshold): y7t_map_curve
//   k_map_finish    one workgroup: nt, the classes that have targets, the counts
#include "y7t_map.h"
#include "y7t_common.h"
#include <mutex>
#include <unordered_map>

static __device__ __forceinline__ int map_rows(const int* hdr) {
    const int r = hdr[Y7T_MAP_H_ROWS], cap = hdr[Y7T_MAP_H_CAP];
    return r < 0 ? 0 : (r > cap ? cap : r);
}

// ---- update ----
__global__ void __launch_bounds__(Y7T_MAP_LANES) k_map_update(char* __restrict__ obj, Y7TMapLayout L, const float* __restrict__ dets, const int* __restrict__ ndets,
                                                             const int* __restrict__ keep, const float* __restrict__ cbox, int ncand, int cand_stride, int B, int max_det,
                                                             const float* __restrict__ targets, const int* __restrict__ toff, float W, float H,
                                                             const float* __restrict__ lb, const float* __restrict__ iouv) {
    __shared__ float tb[Y7T_MAP_LANES * 4], tc[Y7T_MAP_LANES], pb[Y7T_MAP_MAX_DET * 4], bi[Y7T_MAP_MAX_DET];
    __shared__ int bt[Y7T_MAP_MAX_DET];
    int* hdr = (int*)obj;
    const int b = blockIdx.x, cap = hdr[Y7T_MAP_H_CAP];
    // (every workgroup forms the same totals from the same words; nobody writes the row count in this launch)
    long long base = map_rows(hdr), total = 0;
    for (int i = 0; i < B; ++i) {
        int n = ndets[i];
        n = n < 0 ? 0 : (n > max_det ? max_det : n);
        if (i < b) base += n;
        total += n;
    }
    const bool ok = (long long)map_rows(hdr) + total <= (long long)cap;
    if (b == 0 && threadIdx.x == 0) { hdr[Y7T_MAP_H_PENDING] = (int)total; hdr[Y7T_MAP_H_PENDING_OK] = ok ? 1 : 0; }
    if (!ok) return;      // (the whole workgroup's, and every workgroup's)
    int P = ndets[b];
    P = P < 0 ? 0 : (P > max_det ? max_det : P);
    if (P == 0) return;
    const int t0 = toff[b], T = toff[b + 1] - t0;
    const Y7TMapExec ex = {(int)threadIdx.x, Y7T_MAP_LANES};
    y7t_map_image(ex, P, dets + (size_t)b * max_det * 6, keep + (size_t)b * max_det, cbox + (size_t)b * cand_stride * 4, ncand, targets + (size_t)t0 * 6, T < 0 ? 0 : T, W, H,
                  lb + b * 5, iouv, tb, tc, pb, bi, bt, (float*)(obj + L.conf) + base, (int*)(obj + L.cls) + base, (int*)(obj + L.correct) + base);
}

__global__ void __launch_bounds__(256) k_map_commit(char* __restrict__ obj, Y7TMapLayout L, int nc, int B, const float* __restrict__ targets, const int* __restrict__ toff) {
    int* hdr = (int*)obj;
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool ok = hdr[Y7T_MAP_H_PENDING_OK] != 0;
    if (ok && c < nc) {
        long long cnt = 0;
        for (int l = toff[0]; l < toff[B]; ++l) cnt += (targets[(size_t)l * 6 + 1] == (float)c) ? 1 : 0;
        if (cnt) ((long long*)(obj + L.nt))[c] += cnt;
    }
    if (c == 0) {      // (the only reader and writer of these three words in this launch)
        if (ok) { hdr[Y7T_MAP_H_ROWS] += hdr[Y7T_MAP_H_PENDING]; hdr[Y7T_MAP_H_SEEN] += B; }
        else hdr[Y7T_MAP_H_STATUS] |= Y7T_MAP_OVERFLOW;
    }
}

// ---- sort ----
__global__ void __launch_bounds__(256) k_map_keys(char* __restrict__ obj, Y7TMapLayout L, int nc) {
    const int n = map_rows((const int*)obj), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ((uint64_t*)(obj + L.key_a))[i] = y7t_map_key(((const int*)(obj + L.cls))[i], ((const float*)(obj + L.conf))[i], nc);
    ((uint32_t*)(obj + L.idx_a))[i] = (uint32_t)i;
}

// the rows of this wave with the digit `d` (valid lanes only): eight ballots
static __device__ __forceinline__ unsigned long long map_match(int d, bool valid) {
    unsigned long long m = __ballot(valid);
    for (int b = 0; b < 8; ++b) {
        const unsigned long long v = __ballot(valid && ((d >> b) & 1));
        m &= ((d >> b) & 1) ? v : ~v;
    }
    return m;
}

// cnt[w][d] = rows of wave w with digit d; -> this row's rank among the rows of its wave with its digit
static __device__ __forceinline__ int map_tile_counts(int (*cnt)[256], int d, bool valid) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
    __syncthreads();
    const unsigned long long m = map_match(d, valid);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (valid && rank == 0) cnt[wave][d] = __popcll(m);
    __syncthreads();
    return rank;
}

__global__ void __launch_bounds__(256) k_map_hist(char* __restrict__ obj, size_t key_off, size_t hist_off, int pass) {
    __shared__ int cnt[4][256];
    const int n = map_rows((const int*)obj), tiles = (n + Y7T_MAP_TILE - 1) / Y7T_MAP_TILE, tile = blockIdx.x, tid = threadIdx.x;
    if (tile >= tiles) return;
    const int i = tile * Y7T_MAP_TILE + tid;
    const bool valid = i < n;
    const int d = valid ? y7t_map_digit(((const uint64_t*)(obj + key_off))[i], pass) : 0;
    map_tile_counts(cnt, d, valid);
    ((uint32_t*)(obj + hist_off))[(size_t)tid * tiles + tile] = (uint32_t)(cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid]);
}

__global__ void __launch_bounds__(1024) k_map_scan(char* __restrict__ obj, size_t hist_off) {
    __shared__ unsigned part[1024];
    const int n = map_rows((const int*)obj), tiles = (n + Y7T_MAP_TILE - 1) / Y7T_MAP_TILE, tid = threadIdx.x;
    const size_t M = (size_t)tiles * 256, per = (M + 1023) / 1024, lo = tid * per < M ? tid * per : M, hi = lo + per < M ? lo + per : M;
    uint32_t* h = (uint32_t*)(obj + hist_off);
    unsigned s = 0;
    for (size_t i = lo; i < hi; ++i) s += h[i];
    part[tid] = s;
    __syncthreads();
    for (int w = 1; w < 1024; w <<= 1) {
        const unsigned v = tid >= w ? part[tid - w] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned run = part[tid] - s;
    for (size_t i = lo; i < hi; ++i) { const unsigned v = h[i]; h[i] = run; run += v; }
}

__global__ void __launch_bounds__(256) k_map_scatter(char* __restrict__ obj, size_t key_in, size_t idx_in, size_t key_out, size_t idx_out, size_t hist_off, int pass) {
    __shared__ int cnt[4][256];
    const int n = map_rows((const int*)obj), tiles = (n + Y7T_MAP_TILE - 1) / Y7T_MAP_TILE, tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    if (tile >= tiles) return;
    const int i = tile * Y7T_MAP_TILE + tid;
    const bool valid = i < n;
    const uint64_t key = valid ? ((const uint64_t*)(obj + key_in))[i] : 0;
    const int d = valid ? y7t_map_digit(key, pass) : 0;
    const int rank = map_tile_counts(cnt, d, valid);
    if (!valid) return;
    unsigned pos = ((const uint32_t*)(obj + hist_off))[(size_t)d * tiles + tile] + (unsigned)rank;
    for (int w = 0; w < wave; ++w) pos += (unsigned)cnt[w][d];
    if (pos >= (unsigned)n) return;      // (cannot happen: the scan of the histograms ends at n)
    ((uint64_t*)(obj + key_out))[pos] = key;
    ((uint32_t*)(obj + idx_out))[pos] = ((const uint32_t*)(obj + idx_in))[i];
}

__global__ void __launch_bounds__(256) k_map_gather(char* __restrict__ obj, Y7TMapLayout L, size_t idx_off) {
    const int n = map_rows((const int*)obj), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = ((const uint32_t*)(obj + idx_off))[i];
    if (s >= (uint32_t)n) return;
    ((float*)(obj + L.sconf))[i] = ((const float*)(obj + L.conf))[s];
    ((int*)(obj + L.scorrect))[i] = ((const int*)(obj + L.correct))[s];
}

// seg[c] = the first sorted row whose class is >= c, c = 0 .. nc (rows of a class outside [0, nc) lie behind seg[nc])
__global__ void __launch_bounds__(256) k_map_segments(char* __restrict__ obj, Y7TMapLayout L, size_t key_off, int nc) {
    const int n = map_rows((const int*)obj), c = blockIdx.x * 256 + threadIdx.x;
    if (c > nc) return;
    const uint64_t* key = (const uint64_t*)(obj + key_off);
    const uint64_t want = (uint64_t)c << 32;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    ((int*)(obj + L.seg))[c] = lo;
}

__global__ void __launch_bounds__(Y7T_MAP_LANES) k_map_curve(char* __restrict__ obj, Y7TMapLayout L, double* __restrict__ ap, double* __restrict__ p, double* __restrict__ r) {
    __shared__ int part[Y7T_MAP_LANES + 1];
    __shared__ double pmax[Y7T_MAP_LANES], y[Y7T_MAP_GRID];
    const int c = blockIdx.x, k = blockIdx.y;
    const int* seg = (const int*)(obj + L.seg);
    const Y7TMapExec ex = {(int)threadIdx.x, Y7T_MAP_LANES};
    y7t_map_curve(ex, (const float*)(obj + L.sconf), (const int*)(obj + L.scorrect), seg[c], seg[c + 1] - seg[c], ((const long long*)(obj + L.nt))[c], k,
                  (const double*)(obj + L.grid), (const double*)(obj + L.px), part, pmax, y, ap + (size_t)c * Y7T_MAP_NIOU + k, p + (size_t)c * Y7T_MAP_PX,
                  r + (size_t)c * Y7T_MAP_PX);
}

__global__ void __launch_bounds__(256) k_map_finish(const char* __restrict__ obj, Y7TMapLayout L, int nc, long long* __restrict__ nt_out, int* __restrict__ classes_out,
                                                    int* __restrict__ info_out) {
    const long long* nt = (const long long*)(obj + L.nt);
    for (int c = threadIdx.x; c < nc; c += 256) { nt_out[c] = nt[c]; classes_out[c] = -1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int* hdr = (const int*)obj;
        int m = 0;
        for (int c = 0; c < nc; ++c)
            if (nt[c] > 0) classes_out[m++] = c;
        info_out[0] = map_rows(hdr);
        info_out[1] = hdr[Y7T_MAP_H_SEEN];
        info_out[2] = hdr[Y7T_MAP_H_STATUS];
        info_out[3] = m;
    }
}

__global__ void __launch_bounds__(256) k_map_init(char* __restrict__ obj, Y7TMapLayout L, int cap, int nc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int* hdr = (int*)obj;
    if (i < 64) hdr[i] = i == Y7T_MAP_H_CAP ? cap : (i == Y7T_MAP_H_NC ? nc : 0);
    if (i < nc) ((long long*)(obj + L.nt))[i] = 0;
    if (i < Y7T_MAP_GRID) ((double*)(obj + L.grid))[i] = y7t_map_linspace01(i, Y7T_MAP_GRID);
    if (i < Y7T_MAP_PX) ((double*)(obj + L.px))[i] = y7t_map_linspace01(i, Y7T_MAP_PX);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct MapInfo { int cap, nc; };
static std::mutex g_map_mu;
static std::unordered_map<const void*, MapInfo> g_maps;

static bool map_caps_ok(int cap, int nc) { return cap >= 1 && nc >= 1 && nc <= Y7T_MAP_MAX_NC; }

extern "C" size_t y7t_map_bytes(int cap_rows, int nc) {
    if (!map_caps_ok(cap_rows, nc)) return 0;
    return y7t_map_layout_of(cap_rows, nc).total;
}

extern "C" int y7t_map_layout(int cap_rows, int nc, size_t* out4) {
    Y7T_ARG_CHECK(out4 && map_caps_ok(cap_rows, nc));
    const Y7TMapLayout L = y7t_map_layout_of(cap_rows, nc);
    out4[0] = L.nt; out4[1] = L.conf; out4[2] = L.cls; out4[3] = L.correct;
    return 0;
}

extern "C" int y7t_map_init(void* obj, size_t bytes, int cap_rows, int nc, y7t_stream stream) {
    Y7T_ARG_CHECK(obj);
    Y7T_ARG_CHECK(map_caps_ok(cap_rows, nc));
    Y7T_ARG_CHECK(((uintptr_t)obj & 255) == 0);
    const Y7TMapLayout L = y7t_map_layout_of(cap_rows, nc);
    Y7T_ARG_CHECK(bytes >= L.total);
    const int n = nc > Y7T_MAP_PX ? nc : Y7T_MAP_PX;
    hipLaunchKernelGGL(k_map_init, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (char*)obj, L, cap_rows, nc);
    Y7T_LAUNCH_CHECK();
    std::lock_guard<std::mutex> l(g_map_mu);
    g_maps[obj] = MapInfo{cap_rows, nc};
    return 0;
}

extern "C" int y7t_map_release(void* obj) {
    std::lock_guard<std::mutex> l(g_map_mu);
    g_maps.erase(obj);
    return 0;
}

static int map_info(const void* obj, MapInfo* info) {
    std::lock_guard<std::mutex> l(g_map_mu);
    auto it = g_maps.find(obj);
    if (it == g_maps.end()) { y7t_set_error("this address holds no mAP state (y7t_map_init)"); return Y7T_E_STATE; }
    *info = it->second;
    return 0;
}

extern "C" int y7t_map_update(void* obj, const float* dets, const int* ndets, const int* keep, const float* cand_boxes, int cand_rows, int cand_stride, int batch,
                              int max_det, const float* targets, const int* target_offsets, int img_h, int img_w, const float* lb, const float* iouv, y7t_stream stream) {
    MapInfo info;
    if (int e = map_info(obj, &info)) return e;
    Y7T_ARG_CHECK(batch >= 0 && max_det >= 1 && max_det <= Y7T_MAP_MAX_DET && cand_rows >= 1 && cand_stride >= cand_rows && img_h >= 1 && img_w >= 1);
    if (batch == 0) return 0;
    Y7T_ARG_CHECK(dets && ndets && keep && cand_boxes && target_offsets && lb && iouv);      // (targets may be null when the batch has none)
    const Y7TMapLayout L = y7t_map_layout_of(info.cap, info.nc);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_map_update, dim3(batch), dim3(Y7T_MAP_LANES), 0, st, (char*)obj, L, dets, ndets, keep, cand_boxes, cand_rows, cand_stride, batch, max_det, targets,
                       target_offsets, (float)img_w, (float)img_h, lb, iouv);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_map_commit, dim3((info.nc + 255) / 256), dim3(256), 0, st, (char*)obj, L, info.nc, batch, targets, target_offsets);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_map_compute(void* obj, double* ap_out, double* p_out, double* r_out, long long* nt_out, int* classes_out, int* info_out, y7t_stream stream) {
    MapInfo info;
    if (int e = map_info(obj, &info)) return e;
    Y7T_ARG_CHECK(ap_out && p_out && r_out && nt_out && classes_out && info_out);
    const Y7TMapLayout L = y7t_map_layout_of(info.cap, info.nc);
    hipStream_t st = (hipStream_t)stream;
    char* o = (char*)obj;
    const int tiles = (info.cap + Y7T_MAP_TILE - 1) / Y7T_MAP_TILE;      // (the rows are counted on the device: tiles past them leave at once)
    hipLaunchKernelGGL(k_map_keys, dim3(tiles), dim3(256), 0, st, o, L, info.nc);
    Y7T_LAUNCH_CHECK();
    size_t key_in = L.key_a, key_out = L.key_b, idx_in = L.idx_a, idx_out = L.idx_b;
    for (int pass = 0; pass < y7t_map_passes(info.nc); ++pass) {      // digits 0-3: the confidence, 4 (and 5): the class
        hipLaunchKernelGGL(k_map_hist, dim3(tiles), dim3(256), 0, st, o, key_in, L.hist, pass);
        Y7T_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_map_scan, dim3(1), dim3(1024), 0, st, o, L.hist);
        Y7T_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_map_scatter, dim3(tiles), dim3(256), 0, st, o, key_in, idx_in, key_out, idx_out, L.hist, pass);
        Y7T_LAUNCH_CHECK();
        size_t t = key_in; key_in = key_out; key_out = t;
        t = idx_in; idx_in = idx_out; idx_out = t;
    }
    hipLaunchKernelGGL(k_map_gather, dim3(tiles), dim3(256), 0, st, o, L, idx_in);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_map_segments, dim3((info.nc + 1 + 255) / 256), dim3(256), 0, st, o, L, key_in, info.nc);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_map_curve, dim3(info.nc, Y7T_MAP_NIOU), dim3(Y7T_MAP_LANES), 0, st, o, L, ap_out, p_out, r_out);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_map_finish, dim3(1), dim3(256), 0, st, (const char*)o, L, info.nc, nt_out, classes_out, info_out);
    Y7T_LAUNCH_CHECK();
    return 0;
}
