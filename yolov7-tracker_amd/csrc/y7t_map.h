// y7t_map.h -- the detector's mAP evaluation (the reference's test.py:126-209 per image, utils/metrics.py:18-106 after the sequence; DESIGN.md section 4 "mAP
// evaluation" is the specification and tests/map_np.py its NumPy / torch restatement).  This file states the arithmetic and the two workgroup programs ONCE, for
// the device kernels (csrc/y7t_map.hip) and for the CPU build of the same bodies (tests/_hostsim/map.py, -DY7T_HOSTSIM): programs over an execution context
// (thread tid of nt) whose strided loops run at nt = 1 on the host, every per-lane value in an array the caller provides (the LDS on the device).
//
//   y7t_map_image   one image of y7t_map_update: boxes to native space, box_iou, the matching rule, the stored rows
//   y7t_map_curve   one (class, IoU threshold) of y7t_map_compute: counts, recall / precision, envelope, the 101-point AP, the two 1000-point curves
//
// The matching arithmetic is float32, ONE correctly rounded operation at a time in torch's order (contraction off), so device, host build and torch agree bit for
// bit; the curves are float64.  No atomics anywhere: every output element has one writer.  Portable text: the host build needs no HIP header.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(Y7T_HOSTSIM)
#include <hip/hip_runtime.h>
#define Y7T_MAP_FN __device__ __forceinline__
#define Y7T_MAP_HD __host__ __device__ inline
#define Y7T_MAP_DEVICE 1
#else
#define Y7T_MAP_FN static inline
#define Y7T_MAP_HD static inline
#define Y7T_MAP_DEVICE 0
#endif
#if !defined(Y7T_NO_CONTRACT)
#if defined(__clang__)
#define Y7T_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define Y7T_NO_CONTRACT      // (the CPU build is compiled with -ffp-contract=off)
#endif
#endif

enum {
    Y7T_MAP_NIOU = 10,                 // IoU thresholds: torch.linspace(0.5, 0.95, 10), passed in by the caller
    Y7T_MAP_LANES = 256,               // virtual lanes of a workgroup program = threads of a device workgroup
    Y7T_MAP_TILE = 256,                // rows of a sort tile (one per thread)
    Y7T_MAP_MAX_DET = 1024,            // the most rows of one image (the per-prediction arrays of y7t_map_image live in the LDS)
    Y7T_MAP_MAX_NC = 65535,
    Y7T_MAP_GRID = 101,                // np.linspace(0, 1, 101) of compute_ap
    Y7T_MAP_PX = 1000,                 // np.linspace(0, 1, 1000) of ap_per_class
    // header words of the state blob (int32)
    Y7T_MAP_H_ROWS = 0, Y7T_MAP_H_SEEN = 1, Y7T_MAP_H_STATUS = 2, Y7T_MAP_H_PENDING = 3, Y7T_MAP_H_PENDING_OK = 4, Y7T_MAP_H_CAP = 5, Y7T_MAP_H_NC = 6,
    // status word
    Y7T_MAP_OVERFLOW = 1,              // an update would have passed cap_rows: that call stored nothing (no rows, no targets, no images)
};

// the state blob: [header 256 B][nt int64 nc][conf f32 cap][cls i32 cap][correct i32 cap] and the workspace of y7t_map_compute behind them, each 256-byte aligned
struct Y7TMapLayout { size_t nt, conf, cls, correct, key_a, key_b, idx_a, idx_b, hist, sconf, scorrect, seg, grid, px, total; };
Y7T_MAP_HD size_t y7t_map_al256(size_t x) { return (x + 255) & ~(size_t)255; }
Y7T_MAP_HD Y7TMapLayout y7t_map_layout_of(int cap, int nc) {
    Y7TMapLayout L;
    const size_t c = (size_t)cap, tiles = (c + Y7T_MAP_TILE - 1) / Y7T_MAP_TILE;
    size_t o = 256;
    L.nt = o; o = y7t_map_al256(o + (size_t)nc * 8);
    L.conf = o; o = y7t_map_al256(o + c * 4);
    L.cls = o; o = y7t_map_al256(o + c * 4);
    L.correct = o; o = y7t_map_al256(o + c * 4);
    L.key_a = o; o = y7t_map_al256(o + c * 8);
    L.key_b = o; o = y7t_map_al256(o + c * 8);
    L.idx_a = o; o = y7t_map_al256(o + c * 4);
    L.idx_b = o; o = y7t_map_al256(o + c * 4);
    L.hist = o; o = y7t_map_al256(o + tiles * 256 * 4);
    L.sconf = o; o = y7t_map_al256(o + c * 4);
    L.scorrect = o; o = y7t_map_al256(o + c * 4);
    L.seg = o; o = y7t_map_al256(o + ((size_t)nc + 2) * 4);
    L.grid = o; o = y7t_map_al256(o + Y7T_MAP_GRID * 8);
    L.px = o; o = y7t_map_al256(o + Y7T_MAP_PX * 8);
    L.total = o;
    return L;
}

// np.linspace(0, 1, n)[q]: arange(n) * (1 / (n - 1)), the last point set to 1
Y7T_MAP_HD double y7t_map_linspace01(int q, int n) {
    Y7T_NO_CONTRACT
    const double step = 1.0 / (double)(n - 1);
    return q == n - 1 ? 1.0 : (double)q * step;
}

struct Y7TMapExec { int tid, nt; };

Y7T_MAP_FN void y7t_map_sync() {
#if Y7T_MAP_DEVICE
    __syncthreads();
#endif
}

// ---- boxes (float32, torch's order) ----
// scale_coords with ratio_pad: subtract the pad, divide by the gain, clamp to the native image.  lb = (gain, padx, pady, h0, w0)
Y7T_MAP_HD float y7t_map_clamp(float v, float hi) { v = v < 0.0f ? 0.0f : v; return v > hi ? hi : v; }
Y7T_MAP_HD void y7t_map_scale_coords(float* b, const float* lb) {
    Y7T_NO_CONTRACT
    const float gain = lb[0], padx = lb[1], pady = lb[2], h0 = lb[3], w0 = lb[4];
    const float x1 = b[0] - padx, x2 = b[2] - padx, y1 = b[1] - pady, y2 = b[3] - pady;
    b[0] = y7t_map_clamp(x1 / gain, w0);
    b[1] = y7t_map_clamp(y1 / gain, h0);
    b[2] = y7t_map_clamp(x2 / gain, w0);
    b[3] = y7t_map_clamp(y2 / gain, h0);
}

// a target row [image, class, x, y, w, h] (normalised) -> its native-space xyxy: *= (W, H, W, H), xywh2xyxy, scale_coords
Y7T_MAP_HD void y7t_map_target_box(const float* t, float W, float H, const float* lb, float* b) {
    Y7T_NO_CONTRACT
    const float cx = t[2] * W, cy = t[3] * H, w = t[4] * W, h = t[5] * H;
    const float hw = w / 2.0f, hh = h / 2.0f;
    b[0] = cx - hw;
    b[1] = cy - hh;
    b[2] = cx + hw;
    b[3] = cy + hh;
    y7t_map_scale_coords(b, lb);
}

// box_iou(a, b) = inter / ((area_a + area_b) - inter)
Y7T_MAP_HD float y7t_map_iou(const float* a, const float* b) {
    Y7T_NO_CONTRACT
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
    const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
    float w = (a[2] < b[2] ? a[2] : b[2]) - (a[0] > b[0] ? a[0] : b[0]);
    float h = (a[3] < b[3] ? a[3] : b[3]) - (a[1] > b[1] ? a[1] : b[1]);
    w = w < 0.0f ? 0.0f : w;
    h = h < 0.0f ? 0.0f : h;
    const float inter = w * h;
    const float sum = area_a + area_b;
    const float uni = sum - inter;
    return inter / uni;
}

// One image (test.py:126-209).  P predictions: dets (P x 6: [.., .., .., .., conf, cls]; only conf and cls are read), keep (P) -> rows of cbox (candidate xyxy in
// network pixels, `ncand` rows); T targets `tg` (T x 6).  Scratch: tb (LANES x 4), tc (LANES), pb (P x 4), bi (P), bt (P).  Output rows [0, P) of conf / cls / correct.
// The rule: every prediction takes its same-class target of largest IoU (lowest index on a tie); it claims that target when the IoU is > iouv[0]; a target's first
// claimant in row order gets correct = iou > iouv, every later one stays all-false.
Y7T_MAP_FN void y7t_map_image(const Y7TMapExec ex, int P, const float* dets, const int* keep, const float* cbox, int ncand, const float* tg, int T, float W, float H,
                              const float* lb, const float* iouv, float* tb, float* tc, float* pb, float* bi, int* bt, float* conf_out, int* cls_out, int* correct_out) {
    for (int p = ex.tid; p < P; p += ex.nt) {
        int k = keep[p];
        k = k < 0 ? 0 : (k >= ncand ? ncand - 1 : k);
        for (int c = 0; c < 4; ++c) pb[p * 4 + c] = cbox[(size_t)k * 4 + c];
        y7t_map_scale_coords(pb + p * 4, lb);
        bi[p] = 0.0f;
        bt[p] = -1;
    }
    for (int t0 = 0; t0 < T; t0 += Y7T_MAP_LANES) {
        const int m = T - t0 < Y7T_MAP_LANES ? T - t0 : Y7T_MAP_LANES;
        y7t_map_sync();
        for (int j = ex.tid; j < m; j += ex.nt) {
            y7t_map_target_box(tg + (size_t)(t0 + j) * 6, W, H, lb, tb + j * 4);
            tc[j] = tg[(size_t)(t0 + j) * 6 + 1];
        }
        y7t_map_sync();
        for (int p = ex.tid; p < P; p += ex.nt) {
            const float pc = dets[p * 6 + 5];
            float best = bi[p];
            int bj = bt[p];
            for (int j = 0; j < m && bj != -2; ++j) {
                if (tc[j] != pc) continue;
                const float iou = y7t_map_iou(pb + p * 4, tb + j * 4);
                if (iou != iou) { bj = -2; break; }      // (torch's max carries a NaN on: nothing is claimed)
                if (bj < 0 || iou > best) { best = iou; bj = t0 + j; }
            }
            bi[p] = best;
            bt[p] = bj;
        }
    }
    y7t_map_sync();
    const float thr = iouv[0];
    for (int p = ex.tid; p < P; p += ex.nt) {
        const int t = bt[p];
        bool win = t >= 0 && bi[p] > thr;
        for (int q = 0; q < p && win; ++q) win = !(bt[q] == t && bi[q] > thr);
        int mask = 0;
        if (win)
            for (int k = 0; k < Y7T_MAP_NIOU; ++k) mask |= (bi[p] > iouv[k] ? 1 : 0) << k;
        conf_out[p] = dets[p * 6 + 4];
        cls_out[p] = (int)dets[p * 6 + 5];
        correct_out[p] = mask;
    }
}

// ---- the sort key: class ascending, confidence descending; arrival order is the stable sort's ----
Y7T_MAP_HD uint64_t y7t_map_key(int cls, float conf, int nc) {
    union { float f; uint32_t u; } v;
    v.f = conf == 0.0f ? 0.0f : conf;      // (-0 and +0 are equal confidences)
    const uint32_t ord = v.u ^ ((v.u >> 31) ? 0xffffffffu : 0x80000000u);      // ascending with the float
    const uint32_t c = (cls < 0 || cls >= nc) ? (uint32_t)nc : (uint32_t)cls;    // a class no target can have: behind every segment
    return ((uint64_t)c << 32) | (uint64_t)(0xffffffffu - ord);
}
Y7T_MAP_HD int y7t_map_digit(uint64_t key, int pass) { return (int)((key >> (8 * pass)) & 255); }
Y7T_MAP_HD int y7t_map_passes(int nc) { return nc <= 255 ? 5 : 6; }      // four digits of the confidence, one or two of the class (0 .. nc)

// ---- one (class, threshold k): rows [s0, s0 + n) of the sorted table, n_l targets ----
// Scratch: part (LANES + 1 int), pmax (LANES double), y (GRID double).  ap_out: one double; p_out / r_out: PX doubles each, written only when k == 0.
// Lane t owns the contiguous rows [t R, (t + 1) R) with R = ceil(n / LANES): counts by lane, a scan of the lane totals, the suffix maximum of the precision by lane,
// then a walk backwards through the lane's rows that knows for every row its own and its successor's (recall, envelope) and settles the grid points between them.
Y7T_MAP_FN int y7t_map_bit(const int* corr, int i, int k) { return (corr[i] >> k) & 1; }

// np.interp inside [xa, xb): fa at xa, the line to (xb, fb) elsewhere
Y7T_MAP_FN double y7t_map_lerp(double x, double xa, double fa, double xb, double fb) {
    Y7T_NO_CONTRACT
    if (x == xa) return fa;
    const double slope = (fb - fa) / (xb - xa);
    return slope * (x - xa) + fa;
}

// grid points x with a <= x < b take the line (a, fa) -- (b, fb)
Y7T_MAP_FN void y7t_map_settle(const double* grid, double* y, double a, double fa, double b, double fb) {
    if (!(b > a) || !(a <= 1.0)) return;
    int q = (int)(a * 100.0) - 1;
    q = q < 0 ? 0 : q;
    while (q < Y7T_MAP_GRID && grid[q] < a) ++q;
    for (; q < Y7T_MAP_GRID && grid[q] < b; ++q) y[q] = y7t_map_lerp(grid[q], a, fa, b, fb);
}

// the P / R curves over -conf: points px with c_next < px <= c take the line from this row's value to the next row's (x = -px between -c and -c_next)
Y7T_MAP_FN void y7t_map_settle_pr(const double* px, double* p_out, double* r_out, double c, double c_next, double rec, double prec, double rec_n, double prec_n, bool last) {
    int q = 0;
    if (!last) {
        if (!(c > c_next)) return;
        q = c_next >= 0.0 && c_next <= 1.0 ? (int)(c_next * (double)(Y7T_MAP_PX - 1)) - 1 : 0;
        q = q < 0 ? 0 : q;
        while (q < Y7T_MAP_PX && px[q] <= c_next) ++q;
    }
    for (; q < Y7T_MAP_PX && px[q] <= c; ++q) {
        r_out[q] = last ? rec : y7t_map_lerp(-px[q], -c, rec, -c_next, rec_n);
        p_out[q] = last ? prec : y7t_map_lerp(-px[q], -c, prec, -c_next, prec_n);
    }
}

Y7T_MAP_FN void y7t_map_curve(const Y7TMapExec ex, const float* sconf, const int* scorrect, int s0, int n, long long n_l, int k, const double* grid, const double* px,
                              int* part, double* pmax, double* y, double* ap_out, double* p_out, double* r_out) {
    Y7T_NO_CONTRACT
    const bool pr = k == 0;
    const bool live = n > 0 && n_l > 0;
    if (pr)
        for (int q = ex.tid; q < Y7T_MAP_PX; q += ex.nt) { p_out[q] = live ? 1.0 : 0.0; r_out[q] = 0.0; }      // (left = 1 / left = 0; an empty class keeps zeros)
    if (!live) {
        if (ex.tid == 0) ap_out[0] = 0.0;
        return;
    }
    const float* cf = sconf + s0;
    const int* cr = scorrect + s0;
    const int R = (n + Y7T_MAP_LANES - 1) / Y7T_MAP_LANES;
    const double dn = (double)n_l + 1e-16;
    for (int t = ex.tid; t < Y7T_MAP_LANES; t += ex.nt) {
        const long long lo_ = (long long)t * R, hi_ = lo_ + R;
        const int lo = lo_ < n ? (int)lo_ : n, hi = hi_ < n ? (int)hi_ : n;
        int c = 0;
        for (int i = lo; i < hi; ++i) c += y7t_map_bit(cr, i, k);
        part[t] = c;
    }
    for (int q = ex.tid; q < Y7T_MAP_GRID; q += ex.nt) y[q] = 0.0;      // (at and past recall[-1] + 0.01 the envelope is its closing sentinel)
    y7t_map_sync();
    if (ex.tid == 0) {
        int run = 0;
        for (int t = 0; t < Y7T_MAP_LANES; ++t) { const int v = part[t]; part[t] = run; run += v; }
        part[Y7T_MAP_LANES] = run;
    }
    y7t_map_sync();
    for (int t = ex.tid; t < Y7T_MAP_LANES; t += ex.nt) {
        const long long lo_ = (long long)t * R, hi_ = lo_ + R;
        const int lo = lo_ < n ? (int)lo_ : n, hi = hi_ < n ? (int)hi_ : n;
        int tpc = part[t];
        double m = 0.0;
        for (int i = lo; i < hi; ++i) {
            tpc += y7t_map_bit(cr, i, k);
            const double prec = (double)tpc / (double)(i + 1);
            m = prec > m ? prec : m;
        }
        pmax[t] = m;
    }
    y7t_map_sync();
    if (ex.tid == 0) {
        double run = 0.0;      // (the closing sentinel of mpre)
        for (int t = Y7T_MAP_LANES - 1; t >= 0; --t) { const double v = pmax[t]; pmax[t] = run; run = v > run ? v : run; }
    }
    y7t_map_sync();
    for (int t = ex.tid; t < Y7T_MAP_LANES; t += ex.nt) {
        const long long lo_ = (long long)t * R, hi_ = lo_ + R;
        const int lo = lo_ < n ? (int)lo_ : n, hi = hi_ < n ? (int)hi_ : n;
        if (hi <= lo) continue;
        int tpc = part[t + 1];                       // true positives through row hi - 1
        double env_n = pmax[t];                      // the envelope at row hi
        double xn, rec_n = 0.0, prec_n = 0.0, c_n = 0.0;
        if (hi == n) {
            xn = (double)tpc / dn + 0.01;            // mrec's closing sentinel, mpre's is 0
        } else {
            const int tn = tpc + y7t_map_bit(cr, hi, k);
            xn = (double)tn / dn;
            rec_n = xn;
            prec_n = (double)tn / (double)(hi + 1);
            c_n = (double)cf[hi];
        }
        for (int i = hi - 1; i >= lo; --i) {
            const double rec = (double)tpc / dn, prec = (double)tpc / (double)(i + 1);
            const double env = prec > env_n ? prec : env_n;
            y7t_map_settle(grid, y, rec, env, xn, env_n);
            const double c = (double)cf[i];
            if (pr) y7t_map_settle_pr(px, p_out, r_out, c, c_n, rec, prec, rec_n, prec_n, i == n - 1);
            xn = rec; env_n = env; rec_n = rec; prec_n = prec; c_n = c;
            tpc -= y7t_map_bit(cr, i, k);
        }
        if (lo == 0) y7t_map_settle(grid, y, 0.0, 1.0, xn, env_n);      // mrec[0] = 0, mpre[0] = 1 (no precision is above 1)
    }
    y7t_map_sync();
    if (ex.tid == 0) {
        double s = 0.0;      // np.trapz: sum of d * (y[1:] + y[:-1]) / 2
        for (int q = 0; q + 1 < Y7T_MAP_GRID; ++q) s += (grid[q + 1] - grid[q]) * (y[q + 1] + y[q]) / 2.0;
        ap_out[0] = s;
    }
}
