// y7t_orb.hip -- the feature-based camera-motion estimate on the device (csrc/y7t_orb.h states the arithmetic; DESIGN.md section 4 "GMC / features").
//
// Launch scheme.  y7t_orb_extract_u8 enqueues seven launches: the plane; FAST scores from an LDS tile with a 3-pixel halo; non-maximum suppression + mask + the
// count of every row; a one-workgroup scan of the row counts; ordered compaction (a wave per row: ballot and prefix popcount, so the list is row-major without an
// atomic deciding an order); the smoothed plane; orientation + descriptor, a wave per keypoint.  y7t_orb_estimate enqueues four: best-two Hamming matching with the
// current descriptors as 32-byte rows in LDS tiles; the three filters and their statistics in one workgroup; the 2000 hypotheses, a wave each; select + refine +
// write.  Keypoint and match counts live in device memory: every launch is sized by the capacity and reads the count, and the host reads nothing back.
// All sums that cross lanes are integers, so their order does not matter; there is no float atomic and no atomic at all.
#include "y7t_common.h"
#include "y7t_orb.h"

static inline hipStream_t S(y7t_stream s) { return (hipStream_t)s; }

enum { TW = 64, TH = 16, HALO = 3, LW = TW + 2 * HALO, LH = TH + 2 * HALO, LSTRIDE = 72 };

// -- extract ---------------------------------------------------------------------------------------------------------------------------------------------------
// four consecutive pixels a work-item, one 4-byte store (the plane starts 16-byte aligned)
__global__ __launch_bounds__(256) void k_orb_plane(const uint8_t* __restrict__ bgr, int H, int W, int ds, int h, int w, uint8_t* __restrict__ plane) {
    const long long n = (long long)h * w, i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    uint8_t v[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) {
        const long long i = i0 + k;
        if (i < n) {
            const int y = (int)(i / w), x = (int)(i - (long long)y * w);
            v[k] = y7t_orb_plane_px(bgr, H, W, ds, h, w, y, x);
        }
    }
    if (i0 + 4 <= n) *(uint32_t*)(plane + i0) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    else for (int k = 0; i0 + k < n; ++k) plane[i0 + k] = v[k];
}

// the tile and its halo: coordinates outside the plane are clamped (FAST: they only reach pixels of the 3-pixel border, which score 0) or reflected (smoothing)
template <bool REFLECT>
__device__ inline void load_tile(const uint8_t* __restrict__ plane, int h, int w, int tx0, int ty0, uint8_t (*t)[LSTRIDE]) {
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int r = i / LW, c = i - r * LW;
        int y = ty0 - HALO + r, x = tx0 - HALO + c;
        if (REFLECT) { y = y7t_ecc_reflect101(y, h); x = y7t_ecc_reflect101(x, w); }
        else { y = y < 0 ? 0 : y > h - 1 ? h - 1 : y; x = x < 0 ? 0 : x > w - 1 ? w - 1 : x; }
        t[r][c] = plane[(size_t)y * w + x];
    }
}

__global__ __launch_bounds__(256) void k_orb_fast(const uint8_t* __restrict__ plane, int h, int w, uint8_t* __restrict__ scores) {
    __shared__ uint8_t t[LH][LSTRIDE];
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    load_tile<false>(plane, h, w, tx0, ty0, t);
    __syncthreads();
    const int lx = threadIdx.x & (TW - 1), x = tx0 + lx;
    for (int ly = threadIdx.x / TW; ly < TH; ly += 256 / TW) {
        const int y = ty0 + ly;
        if (x < w && y < h) {
            const bool inside = x >= HALO && x < w - HALO && y >= HALO && y < h - HALO;
            scores[(size_t)y * w + x] = inside ? (uint8_t)y7t_orb_fast_score(&t[ly + HALO][lx + HALO], LSTRIDE) : (uint8_t)0;
        }
    }
}

// a workgroup per row: keep map and the row's count.  The boxes are converted once per row, a work-item per box and BOX_CHUNK boxes at a time, and those that
// cross THIS row are compacted (ballot and prefix popcount) into LDS as the column range [x0, x1) they mask; a surviving maximum then walks a handful of integer
// ranges instead of dividing doubles for every box.  The same predicate as y7t_orb_unmasked, which supplies the frame and border part (called with no boxes) and
// the bounds (y7t_orb_slice_bound, y7t_orb_trunc).
enum { BOX_CHUNK = 256 };
__global__ __launch_bounds__(256) void k_orb_nms(const uint8_t* __restrict__ scores, int h, int w, int ds, const float* __restrict__ dets, int n_dets,
                                                 uint8_t* __restrict__ keep, int* __restrict__ rowcnt) {
    __shared__ int sW[4], sWc[4];
    __shared__ int2 sBox[BOX_CHUNK];
    const int y = blockIdx.x, tid = threadIdx.x;
    int cnt = 0;
    // the candidates of this row (at most ceil(w / 256) <= 32 a work-item): maximum, inside the frame and ORB's border
    unsigned cand = 0;
    for (int x = tid, b = 0; x < w; x += 256, ++b)
        if (y >= 1 && y < h - 1 && x >= 1 && x < w - 1 && y7t_orb_is_max(scores + (size_t)y * w + x, w) && y7t_orb_unmasked(dets, 0, ds, h, w, x, y)) cand |= 1u << b;
    for (int k0 = 0; k0 < n_dets; k0 += BOX_CHUNK) {
        const int k = k0 + tid;
        bool row = false;
        int2 rng = make_int2(0, 0);
        if (k < n_dets) {
            const float* d = dets + (size_t)k * 6;
            const int x0 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[0] / (double)ds), w), y0 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[1] / (double)ds), h);
            const int x1 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[2] / (double)ds), w), y1 = y7t_orb_slice_bound(y7t_orb_trunc((double)d[3] / (double)ds), h);
            row = y >= y0 && y < y1 && x0 < x1;
            rng = make_int2(x0, x1);
        }
        const unsigned long long bal = __ballot(row);
        __syncthreads();      // (the previous chunk has been read)
        if ((tid & 63) == 0) sWc[tid >> 6] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int v = 0; v < 4; ++v) { before += v < (tid >> 6) ? sWc[v] : 0; all += sWc[v]; }
        if (row) sBox[before + __popcll(bal & ((1ull << (tid & 63)) - 1ull))] = rng;
        __syncthreads();
        for (int x = tid, b = 0; x < w; x += 256, ++b)
            if (cand >> b & 1u) {
                int hit = 0;
                for (int j = 0; j < all; ++j) { const int2 r = sBox[j]; hit |= (x >= r.x) & (x < r.y); }
                if (hit) cand &= ~(1u << b);
            }
    }
    for (int x = tid, b = 0; x < w; x += 256, ++b) {
        const bool k = (cand >> b & 1u) != 0;
        keep[(size_t)y * w + x] = k ? 1 : 0;
        cnt += k ? 1 : 0;
    }
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((tid & 63) == 0) sW[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) rowcnt[y] = sW[0] + sW[1] + sW[2] + sW[3];
}

// exclusive scan of the row counts (h <= 8192: at most 8 rows a work-item), the state's header
__global__ __launch_bounds__(1024) void k_orb_scan(const int* __restrict__ rowcnt, int h, int w, int cap, int* __restrict__ rowoff, Y7TOrbHdr* __restrict__ hdr) {
    __shared__ int s[1024];
    const int tid = threadIdx.x, per = (h + 1023) / 1024, lo = tid * per, hi = lo + per < h ? lo + per : h;
    int mine = 0;
    for (int y = lo; y < hi; ++y) mine += rowcnt[y];
    s[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    int run = s[tid] - mine;
    for (int y = lo; y < hi; ++y) { rowoff[y] = run; run += rowcnt[y]; }
    if (tid == 1023) {
        const int total = s[1023];
        Y7TOrbHdr o;
        o.n = total < cap ? total : cap; o.total = total; o.truncated = total > cap ? 1 : 0; o.h = h; o.w = w; o.pad[0] = o.pad[1] = o.pad[2] = 0;
        *hdr = o;
    }
}

// a wave per row: the kept pixels of the row, left to right, to rowoff[y] ... ; positions at or past the capacity are dropped
__global__ __launch_bounds__(256) void k_orb_compact(const uint8_t* __restrict__ keep, const int* __restrict__ rowcnt, const int* __restrict__ rowoff, int h, int w,
                                                     int cap, Y7TOrbKp* __restrict__ kps) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= h || rowcnt[y] == 0) return;
    int base = rowoff[y];
    if (base >= cap) return;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        const bool f = x < w && keep[(size_t)y * w + x] != 0;
        const unsigned long long m = __ballot(f);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (f && pos < cap) { Y7TOrbKp k; k.x = x; k.y = y; kps[pos] = k; }
        base += __popcll(m);
    }
}

// rows, then columns, from an LDS tile with a reflected 3-pixel halo; integers throughout, so equal to y7t_orb_smooth_px
__global__ __launch_bounds__(256) void k_orb_smooth(const uint8_t* __restrict__ plane, int h, int w, uint8_t* __restrict__ out) {
    __shared__ uint8_t t[LH][LSTRIDE];
    __shared__ int rws[LH][TW + 1];
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    load_tile<true>(plane, h, w, tx0, ty0, t);
    __syncthreads();
    for (int i = threadIdx.x; i < LH * TW; i += 256) {
        const int r = i / TW, c = i - r * TW;
        int a = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) a += y7t_orb_tap(k) * (int)t[r][c + k];
        rws[r][c] = a;
    }
    __syncthreads();
    const int lx = threadIdx.x & (TW - 1), x = tx0 + lx;
    for (int ly = threadIdx.x / TW; ly < TH; ly += 256 / TW) {
        const int y = ty0 + ly;
        if (x < w && y < h) {
            int a = 0;
#pragma unroll
            for (int k = 0; k < 7; ++k) a += y7t_orb_tap(k) * rws[ly + k][lx];
            out[(size_t)y * w + x] = (uint8_t)((a + (1 << 19)) >> 20);
        }
    }
}

// a wave per keypoint: the two moments over the disc (lanes over the 961 patch positions, an integer butterfly), then 4 x 64 descriptor bits by ballot
__global__ __launch_bounds__(256) void k_orb_describe(const uint8_t* __restrict__ plane, const uint8_t* __restrict__ smooth, int w, int cap, void* __restrict__ state,
                                                      int* __restrict__ moments) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const Y7TOrbHdr* hdr = (const Y7TOrbHdr*)state;
    if (i >= cap || i >= hdr->n) return;
    const Y7TOrbKp kp = y7t_orb_kps(state, cap)[i];
    const uint8_t* c = plane + (size_t)kp.y * w + kp.x;
    int m10 = 0, m01 = 0;
    for (int idx = lane; idx < 961; idx += 64) y7t_orb_moment_term(c, w, idx, &m10, &m01);
    for (int off = 32; off >= 1; off >>= 1) { m10 += __shfl_xor(m10, off, 64); m01 += __shfl_xor(m01, off, 64); }
    double co, si;
    y7t_orb_direction(m10, m01, &co, &si);
    const uint8_t* cs = smooth + (size_t)kp.y * w + kp.x;
    unsigned long long* d = y7t_orb_desc(state) + (size_t)i * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned long long m = __ballot(y7t_orb_bit(cs, w, r * 64 + lane, co, si) != 0);
        if (lane == 0) d[r] = m;
    }
    if (lane == 0) { moments[2 * i] = m10; moments[2 * i + 1] = m01; }
}

// -- estimate --------------------------------------------------------------------------------------------------------------------------------------------------
// 64 previous descriptors a workgroup, one per lane; its 16 waves share the current descriptors, which pass through LDS 256 rows of 32 bytes at a time: wave v takes
// rows v, v + 16, ... of a tile, every lane reading the same row (a broadcast).  A wave meets its candidates with ascending index, so y7t_orb_best_two's strict comparisons
// give its best two in (distance, index) order; the 16 partial pairs of a previous descriptor are then merged under the same lexicographic order, which makes the
// result independent of how the candidates were dealt out.
enum { M_PREV = 64, M_WAVES = 16, M_TILE = 256 };
__device__ inline void merge_best_two(Y7TOrbMatch* m, int j, int d) {
    if (j < 0) return;
    if (d < m->d1 || (d == m->d1 && j < m->j1)) { m->j2 = m->j1; m->d2 = m->d1; m->j1 = j; m->d1 = d; }
    else if (d < m->d2 || (d == m->d2 && j < m->j2)) { m->j2 = j; m->d2 = d; }
}
__global__ __launch_bounds__(M_PREV * M_WAVES) void k_orb_match(const void* __restrict__ prev, const void* __restrict__ cur, int cap, Y7TOrbMatch* __restrict__ matches) {
    __shared__ unsigned long long tile[M_TILE][4];
    __shared__ Y7TOrbMatch part[M_WAVES][M_PREV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x * M_PREV + lane;
    const int n_prev = ((const Y7TOrbHdr*)prev)->n, n_cur = ((const Y7TOrbHdr*)cur)->n;
    if (blockIdx.x * M_PREV >= n_prev || n_cur < 2) return;
    const unsigned long long* pd = y7t_orb_desc((void*)prev);
    const unsigned long long* cd = y7t_orb_desc((void*)cur);
    const bool live = i < n_prev && i < cap;
    unsigned long long mine[4] = {0, 0, 0, 0};
    if (live)
        for (int k = 0; k < 4; ++k) mine[k] = pd[(size_t)i * 4 + k];
    Y7TOrbMatch m;
    m.j1 = -1; m.j2 = -1; m.d1 = 1 << 30; m.d2 = 1 << 30;
    for (int t0 = 0; t0 < n_cur; t0 += M_TILE) {
        const int cnt = n_cur - t0 < M_TILE ? n_cur - t0 : M_TILE;
        if ((tid >> 2) < cnt) tile[tid >> 2][tid & 3] = cd[(size_t)(t0 + (tid >> 2)) * 4 + (tid & 3)];      // 1024 work-items, 8 bytes each: coalesced
        __syncthreads();
        if (live)
            for (int j = wave; j < cnt; j += M_WAVES) y7t_orb_best_two(&m, t0 + j, y7t_orb_hamming(mine, tile[j]));
        __syncthreads();
    }
    part[wave][lane] = m;
    __syncthreads();
    if (wave == 0 && live) {
        Y7TOrbMatch r;
        r.j1 = -1; r.j2 = -1; r.d1 = 1 << 30; r.d2 = 1 << 30;
        for (int v = 0; v < M_WAVES; ++v) {
            const Y7TOrbMatch p = part[v][lane];
            merge_best_two(&r, p.j1, p.d1);
            merge_best_two(&r, p.j2, p.d2);
        }
        matches[i] = r;
    }
}

// one workgroup: the ratio and distance tests with their integer sums, the statistics, the one-sided test, and the good matches in the order of the previous keypoints
__global__ __launch_bounds__(1024) void k_orb_filter(const void* __restrict__ prev, const void* __restrict__ cur, int cap, const Y7TOrbMatch* __restrict__ matches,
                                                     Y7TOrbPair* __restrict__ good, Y7TOrbEst* __restrict__ est) {
    __shared__ long long sW[16][5];
    __shared__ double sStat[4];
    __shared__ int sCnt[16];
    __shared__ long long sN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Y7TOrbHdr* ph = (const Y7TOrbHdr*)prev;
    const Y7TOrbHdr* ch = (const Y7TOrbHdr*)cur;
    const int n_prev = ph->n, n_cur = ch->n, h = ch->h, w = ch->w;
    Y7TOrbEst e;
    e.n_good = 0; e.flag = Y7T_ORB_NO_MATCHES; e.n_first = 0; e.winner = -1; e.n_inliers = 0; e.pad[0] = e.pad[1] = e.pad[2] = 0;
    if (n_prev == 0 || n_cur < 2) {
        if (tid == 0) *est = e;
        return;
    }
    const Y7TOrbKp* pk = y7t_orb_kps((void*)prev, cap);
    const Y7TOrbKp* ck = y7t_orb_kps((void*)cur, cap);
    long long a[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < n_prev; i += 1024) {
        const Y7TOrbMatch m = matches[i];
        const int dx = pk[i].x - ck[m.j1].x, dy = pk[i].y - ck[m.j1].y;
        if (y7t_orb_first_tests(m, dx, dy, h, w)) { a[0] += 1; a[1] += dx; a[2] += (long long)dx * dx; a[3] += dy; a[4] += (long long)dy * dy; }
    }
    for (int k = 0; k < 5; ++k) {
        for (int off = 32; off >= 1; off >>= 1) a[k] += __shfl_down(a[k], off, 64);
        if (lane == 0) sW[wave][k] = a[k];
    }
    __syncthreads();
    if (tid == 0) {
        long long t[5] = {0, 0, 0, 0, 0};
        for (int v = 0; v < 16; ++v)
            for (int k = 0; k < 5; ++k) t[k] += sW[v][k];
        sN = t[0];
        if (t[0] > 0) {
            y7t_orb_mean_std(t[0], t[1], t[2], &sStat[0], &sStat[1]);
            y7t_orb_mean_std(t[0], t[3], t[4], &sStat[2], &sStat[3]);
        }
    }
    __syncthreads();
    const long long n_first = sN;
    if (n_first == 0) {      // (np.mean of nothing: the reference goes on with NaN and finds no good match)
        e.flag = Y7T_ORB_NOT_ENOUGH;
        if (tid == 0) *est = e;
        return;
    }
    const double mx = sStat[0], sx = sStat[1], my = sStat[2], sy = sStat[3];
    int run = 0;
    for (int i0 = 0; i0 < n_prev; i0 += 1024) {
        const int i = i0 + tid;
        bool g = false;
        Y7TOrbPair p;
        p.px = p.py = p.cx = p.cy = 0;
        if (i < n_prev) {
            const Y7TOrbMatch m = matches[i];
            p.px = pk[i].x; p.py = pk[i].y; p.cx = ck[m.j1].x; p.cy = ck[m.j1].y;
            const int dx = p.px - p.cx, dy = p.py - p.cy;
            g = y7t_orb_first_tests(m, dx, dy, h, w) && y7t_orb_one_sided(dx, mx, sx) && y7t_orb_one_sided(dy, my, sy);
        }
        const unsigned long long bal = __ballot(g);
        if (lane == 0) sCnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int v = 0; v < 16; ++v) { before += v < wave ? sCnt[v] : 0; all += sCnt[v]; }
        if (g) good[run + before + __popcll(bal & ((1ull << lane) - 1ull))] = p;
        run += all;
        __syncthreads();
    }
    if (tid == 0) {
        e.n_good = run; e.n_first = (int)n_first; e.flag = run <= 4 ? Y7T_ORB_NOT_ENOUGH : Y7T_ORB_OK;
        *est = e;
    }
}

// a wave per hypothesis: the inliers of the similarity through its two matches, counted by ballot and popcount
__global__ __launch_bounds__(256) void k_orb_hyp(const Y7TOrbPair* __restrict__ good, const Y7TOrbEst* __restrict__ est, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= Y7T_ORB_NHYP || est->flag != Y7T_ORB_OK) return;
    const int n = est->n_good;
    Y7TOrbModel m;
    int cnt = 0;
    if (y7t_orb_model(good[y7t_orb_pick(k, 0, n)], good[y7t_orb_pick(k, 1, n)], &m))
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int t = t0 + lane;
            cnt += __popcll(__ballot(t < n && y7t_orb_inlier(m, good[t])));
        }
    if (lane == 0) counts[k] = cnt;
}

// one workgroup: the hypothesis with the most inliers (the lowest k among equals), the integer sums over its inliers, the closed-form similarity, warp and status
__global__ __launch_bounds__(256) void k_orb_select(const void* __restrict__ prev, const void* __restrict__ cur, const Y7TOrbPair* __restrict__ good,
                                                    const int* __restrict__ counts, int ds, Y7TOrbEst* __restrict__ est, double* __restrict__ warp6,
                                                    double* __restrict__ status6) {
    __shared__ int sC[256], sK[256];
    __shared__ long long sW[4][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Y7TOrbHdr* ph = (const Y7TOrbHdr*)prev;
    const Y7TOrbHdr* ch = (const Y7TOrbHdr*)cur;
    const int trunc = ch->truncated | ph->truncated << 1;
    Y7TOrbEst e = *est;
    if (e.flag != Y7T_ORB_OK) {
        if (tid == 0) y7t_orb_finish(ph->n, ch->n, trunc, &e, false, warp6, status6);
        return;
    }
    int bc = -1, bk = Y7T_ORB_NHYP;
    for (int k = tid; k < Y7T_ORB_NHYP; k += 256) {      // (ascending k: a strict comparison keeps the lowest)
        const int c = counts[k];
        if (c > bc) { bc = c; bk = k; }
    }
    sC[tid] = bc; sK[tid] = bk;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) {
            const int c = sC[tid + off], k = sK[tid + off];
            if (c > sC[tid] || (c == sC[tid] && k < sK[tid])) { sC[tid] = c; sK[tid] = k; }
        }
        __syncthreads();
    }
    const int n = e.n_good, win = sK[0];
    e.winner = win; e.n_inliers = sC[0];
    bool have = false;
    if (e.n_inliers >= 2) {
        Y7TOrbModel m;
        y7t_orb_model(good[y7t_orb_pick(win, 0, n)], good[y7t_orb_pick(win, 1, n)], &m);
        long long a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int t = tid; t < n; t += 256) {
            const Y7TOrbPair g = good[t];
            if (y7t_orb_inlier(m, g)) {
                const long long x = g.px, y = g.py, u = g.cx, v = g.cy;
                a[0] += x; a[1] += y; a[2] += u; a[3] += v; a[4] += x * x + y * y; a[5] += x * u + y * v; a[6] += x * v - y * u; a[7] += 1;
            }
        }
        for (int k = 0; k < 8; ++k) {
            for (int off = 32; off >= 1; off >>= 1) a[k] += __shfl_down(a[k], off, 64);
            if (lane == 0) sW[wave][k] = a[k];
        }
        __syncthreads();
        if (tid == 0) {
            long long t[8];
            for (int k = 0; k < 8; ++k) t[k] = sW[0][k] + sW[1][k] + sW[2][k] + sW[3][k];
            have = y7t_orb_refine(t[7], t, ds, warp6);
        }
    }
    if (tid == 0) {
        if (!have) e.flag = Y7T_ORB_NO_MODEL;
        *est = e;
        y7t_orb_finish(ph->n, ch->n, trunc, &e, have, warp6, status6);
    }
}

// -- C ABI -----------------------------------------------------------------------------------------------------------------------------------------------------
static int orb_dims_ok(int h, int w, int cap) {
    return h > 2 * Y7T_ORB_EDGE && w > 2 * Y7T_ORB_EDGE && h <= Y7T_ORB_MAX_DIM && w <= Y7T_ORB_MAX_DIM && cap >= 1 && cap <= Y7T_ORB_MAX_CAP;
}

extern "C" int y7t_orb_workspace_bytes(int h, int w, int max_keypoints, size_t* out) {
    Y7T_ARG_CHECK(out && orb_dims_ok(h, w, max_keypoints));
    size_t off[Y7T_ORB_NTAP];
    y7t_orb_layout(h, w, max_keypoints, off);
    *out = off[Y7T_ORB_NTAP - 1];
    return 0;
}

extern "C" int y7t_orb_state_bytes(int max_keypoints, size_t* out) {
    Y7T_ARG_CHECK(out && max_keypoints >= 1 && max_keypoints <= Y7T_ORB_MAX_CAP);
    *out = y7t_orb_state_size(max_keypoints);
    return 0;
}

extern "C" int y7t_orb_tap_layout(int h, int w, int max_keypoints, size_t* offsets12) {
    Y7T_ARG_CHECK(offsets12 && orb_dims_ok(h, w, max_keypoints));
    y7t_orb_layout(h, w, max_keypoints, offsets12);
    return 0;
}

extern "C" int y7t_orb_extract_u8(const uint8_t* bgr, int H, int W, int downscale, const float* dets, int n_dets, int max_keypoints, void* workspace, void* state_out,
                                  y7t_stream stream) {
    Y7T_ARG_CHECK(bgr && workspace && state_out && downscale >= 1 && H >= 1 && W >= 1 && n_dets >= 0 && (dets || n_dets == 0));
    const int h = H / downscale, w = W / downscale, cap = max_keypoints;
    Y7T_ARG_CHECK(orb_dims_ok(h, w, cap));
    Y7T_ARG_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)state_out & 15) == 0);
    size_t off[Y7T_ORB_NTAP];
    y7t_orb_layout(h, w, cap, off);
    char* ws = (char*)workspace;
    uint8_t *plane = (uint8_t*)(ws + off[0]), *scores = (uint8_t*)(ws + off[1]), *keep = (uint8_t*)(ws + off[2]), *smooth = (uint8_t*)(ws + off[3]);
    int *rowcnt = (int*)(ws + off[4]), *rowoff = (int*)(ws + off[5]), *moments = (int*)(ws + off[6]);
    const dim3 tiles((w + TW - 1) / TW, (h + TH - 1) / TH);
    const long long npix = (long long)h * w;
    y7t_note_kernel("k_orb_extract");
    hipLaunchKernelGGL(k_orb_plane, dim3((unsigned)((npix + 1023) / 1024)), dim3(256), 0, S(stream), bgr, H, W, downscale, h, w, plane);
    hipLaunchKernelGGL(k_orb_fast, tiles, dim3(256), 0, S(stream), (const uint8_t*)plane, h, w, scores);
    hipLaunchKernelGGL(k_orb_nms, dim3(h), dim3(256), 0, S(stream), (const uint8_t*)scores, h, w, downscale, dets, n_dets, keep, rowcnt);
    hipLaunchKernelGGL(k_orb_scan, dim3(1), dim3(1024), 0, S(stream), (const int*)rowcnt, h, w, cap, rowoff, (Y7TOrbHdr*)state_out);
    hipLaunchKernelGGL(k_orb_compact, dim3((h + 3) / 4), dim3(256), 0, S(stream), (const uint8_t*)keep, (const int*)rowcnt, (const int*)rowoff, h, w, cap,
                       y7t_orb_kps(state_out, cap));
    hipLaunchKernelGGL(k_orb_smooth, tiles, dim3(256), 0, S(stream), (const uint8_t*)plane, h, w, smooth);
    hipLaunchKernelGGL(k_orb_describe, dim3((cap + 3) / 4), dim3(256), 0, S(stream), (const uint8_t*)plane, (const uint8_t*)smooth, w, cap, state_out, moments);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_orb_estimate(const void* prev_state, const void* cur_state, int h, int w, int downscale, int max_keypoints, void* workspace,
                                double* warp_out6_f64, double* status_out6_f64, y7t_stream stream) {
    Y7T_ARG_CHECK(prev_state && cur_state && workspace && warp_out6_f64 && status_out6_f64 && downscale >= 1);
    const int cap = max_keypoints;
    Y7T_ARG_CHECK(orb_dims_ok(h, w, cap));
    Y7T_ARG_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)prev_state & 15) == 0 && ((uintptr_t)cur_state & 15) == 0);
    size_t off[Y7T_ORB_NTAP];
    y7t_orb_layout(h, w, cap, off);
    char* ws = (char*)workspace;
    Y7TOrbMatch* matches = (Y7TOrbMatch*)(ws + off[7]);
    Y7TOrbPair* good = (Y7TOrbPair*)(ws + off[8]);
    Y7TOrbEst* est = (Y7TOrbEst*)(ws + off[9]);
    int* counts = (int*)(ws + off[10]);
    y7t_note_kernel("k_orb_estimate");
    hipLaunchKernelGGL(k_orb_match, dim3((cap + M_PREV - 1) / M_PREV), dim3(M_PREV * M_WAVES), 0, S(stream), prev_state, cur_state, cap, matches);
    hipLaunchKernelGGL(k_orb_filter, dim3(1), dim3(1024), 0, S(stream), prev_state, cur_state, cap, (const Y7TOrbMatch*)matches, good, est);
    hipLaunchKernelGGL(k_orb_hyp, dim3(Y7T_ORB_NHYP / 4), dim3(256), 0, S(stream), (const Y7TOrbPair*)good, (const Y7TOrbEst*)est, counts);
    hipLaunchKernelGGL(k_orb_select, dim3(1), dim3(256), 0, S(stream), prev_state, cur_state, (const Y7TOrbPair*)good, (const int*)counts, downscale, est, warp_out6_f64,
                       status_out6_f64);
    Y7T_LAUNCH_CHECK();
    return 0;
}
