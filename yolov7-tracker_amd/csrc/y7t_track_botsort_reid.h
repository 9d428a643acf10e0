// y7t_track_botsort_reid.h -- BoT-SORT with its appearance branch (use_apperance_model = True: equations 12-13 of the BoT-SORT paper) as a workgroup program over
// the same device-resident track pool as the other trackers (y7t_track_step.h).  Portable text (device: hipcc; CPU tests: -DY7T_HOSTSIM).
//
// Restates /root/reference/tracker/botsort.py:313-493 (BoTSORT.update with use_apperance_model = True), tracker/matching.py:84-103 (embedding_distance, metric
// 'cosine'), :165-178 (cal_cosine_distance), tracker/basetrack.py:296-339 (STrack.re_activate / update: the float32 moving average of the normalised features,
// y7t_ss_store_pending of y7t_track_strongsort.h -- StrongSORT's store, the same code), tracker/botsort.py:250-269 (multi_gmc).
//
// The fused cost of the first (0.9) and the unconfirmed (0.7) association is
//     App = 0.5 * (1 - cos);  App[IoU_dist > theta_iou] = 1;  App[App > theta_emb] = 1;  cost = min(IoU_dist, App)
// so cost differs from IoU_dist only where IoU_dist <= theta_iou = 0.5 < 1: on pairs of boxes that overlap.  That is exact, and it is what this program is built
// on: an association first walks its box pairs like every IoU pass (y7t_pairs with the group rejection of boxes apart) and files the pairs at or under theta_iou
// in a hash table of the feature state, then a LANE PER FILED PAIR evaluates the cosine (one sequential float64 FMA chain over the normalised rows), and the
// solvers' cost functions look the value up.  No track x detection appearance matrix exists, the candidate graph of the sparse solver is the IoU graph.
//
// Reference behaviours reproduced literally:
//   * high detections are score >= det_thresh (botsort.py:339; DeepSORT / StrongSORT: >), low ones low_conf_thresh < score < det_thresh; only high ones carry a vector;
//   * multi_predict first, then multi_gmc on strack_pool and on the unconfirmed tracks (botsort.py:376-382);
//   * the second association (IoU only, 0.5) takes EVERY unmatched pool track (botsort.py:411); a track matched there keeps its vector (the low detection has none);
//   * new tracks come from every detection left after the FIRST association with score > det_thresh + 0.1 (botsort.py:462-466) and start with the RAW vector;
//   * re_activate keeps the vector, update runs the float32 moving average.
#pragma once
#include "y7t_track_step.h"
#include "y7t_track_strongsort.h"      // Y7TSsHdr / Y7TSs and y7t_ss_store_pending: the one-vector store with its float32 moving average is StrongSORT's, on this state's memory
#include "y7t_track_pend.h"            // the queue of vectors to store
#include "y7t_np_arith.h"        // numpy's float64 row norms and dot products, Y7T_NO_CONTRACT

// (Y7T_BOTSORT_REID = 8: y7t_track_core.h)

// feature state of one tracker: caller-owned device memory next to the track-pool blob.  The header BEGINS with StrongSORT's (the status word at byte 20, the
// pending-store counter: the queue of y7t_track_pend.h and y7t_ss_store_pending run on it as they are); its spare words carry this program's own values:
//   ss.pad1 = the frame's count of cosines evaluated, ss.gamma = theta_iou, ss.pad2 = theta_emb
struct Y7TBrHdr { Y7TSsHdr ss; int n_emb /* evaluated pairs of the frame that theta_emb sent to 1 */, hcap, h_nb /* columns of the association the table holds */, pad; };
#define Y7T_BR_NDOTS(h) ((h)->ss.pad1)
#define Y7T_BR_THETA_IOU(h) ((h)->ss.gamma)
#define Y7T_BR_THETA_EMB(h) ((h)->ss.pad2)
static_assert(sizeof(Y7TBrHdr) == sizeof(Y7TSsHdr) + 4 * 4, "the feature-state header of BoT-SORT with ReID: n_dots at byte 28, theta_iou at 32, theta_emb at 40, its four own ints from 48");
#define Y7T_BR_PPD 2      // pending stores per detection of the capacity: a detection left after the first association may update an unconfirmed track AND start a track
enum { Y7T_BR_ERR_VEC = 4 /* a zero-norm or non-finite appearance vector: the frame was not stepped */, Y7T_BR_ERR_PAIRS = 32 /* more pairs at or under theta_iou than the table holds */ };
struct Y7TBrLayout { size_t vec, pend, tn, dn, hkey, hlist, hval, total; };
struct Y7TBr {
    Y7TBrHdr* h;
    Y7TSs ss;           // h, vec [cap_t][dim] (STrack.features[-1] of the slot's track), pend [2 cap_d][3]: StrongSORT's view of the same memory (app: null)
    double* tn;         // [cap_t][dim]  the slot's vector / its np.linalg.norm, float64: cal_cosine_distance's mat1 rows of this frame (slots of the tracked / lost lists)
    double* dn;         // [cap_d][dim]  the same of the frame's detection rows at or above det_thresh (mat2)
    int* hkey;          // [hcap]        open-addressing table of the association in flight: row * h_nb + column of a pair with IoU_dist <= theta_iou, -1 = empty
    int* hlist;         // [hcap]        the table entries in the order they were filed
    double* hval;       // [hcap]        0.5 * (1 - cos) of the entry's pair
};
// a pair files once per association; 8 entries per track or detection of the capacities, filled to three quarters at most
Y7T_HD int y7t_br_hcap(int cap_t, int cap_d) {
    const long long m = 8ll * (cap_t > cap_d ? cap_t : cap_d);
    int h = 256;
    while (h < m && h < (1 << 28)) h <<= 1;
    return h;
}
Y7T_HD Y7TBrLayout y7t_br_layout(int cap_t, int cap_d, int dim) {
    Y7TBrLayout L;
    size_t o = y7t_al(sizeof(Y7TBrHdr));
    const size_t T = (size_t)cap_t, D = (size_t)cap_d, H = (size_t)y7t_br_hcap(cap_t, cap_d);
#define Y7T_TAKE(f, bytes) L.f = o; o = y7t_al(o + (bytes));
    Y7T_TAKE(vec, T * dim * 4) Y7T_TAKE(pend, Y7T_BR_PPD * D * 3 * 4) Y7T_TAKE(tn, T * dim * 8) Y7T_TAKE(dn, D * dim * 8) Y7T_TAKE(hkey, H * 4) Y7T_TAKE(hlist, H * 4) Y7T_TAKE(hval, H * 8)
#undef Y7T_TAKE
    L.total = o;
    return L;
}
Y7T_FN Y7TBr y7t_br_bind(void* blob) {
    Y7TBrHdr* h = (Y7TBrHdr*)blob;
    const Y7TBrLayout L = y7t_br_layout(h->ss.cap_t, h->ss.cap_d, h->ss.dim);
    char* b = (char*)blob;
    Y7TBr f;
    f.h = h;
    f.ss.h = &h->ss; f.ss.vec = (float*)(b + L.vec); f.ss.app = nullptr; f.ss.pend = (int*)(b + L.pend);
    f.tn = (double*)(b + L.tn); f.dn = (double*)(b + L.dn);
    f.hkey = (int*)(b + L.hkey); f.hlist = (int*)(b + L.hlist); f.hval = (double*)(b + L.hval);
    return f;
}
Y7T_FN void y7t_br_init(const Y7TExec& ex, void* blob, int cap_t, int cap_d, int dim, double theta_iou, double theta_emb) {
    Y7TBrHdr* h = (Y7TBrHdr*)blob;
    if (ex.tid == 0) {
        h->ss.magic = 0x59374252; h->ss.dim = dim; h->ss.budget = 1; h->ss.cap_t = cap_t; h->ss.cap_d = cap_d; h->ss.status = 0; h->ss.n_pend = 0;
        Y7T_BR_NDOTS(h) = 0; Y7T_BR_THETA_IOU(h) = theta_iou; Y7T_BR_THETA_EMB(h) = theta_emb;
        h->n_emb = 0; h->hcap = y7t_br_hcap(cap_t, cap_d); h->h_nb = 0; h->pad = 0;
    }
    y7t_sync(ex);
}

// 1. - cal_cosine_distance(mat1, mat2) in float64: y7t_np_arith.h -- the rows divided by their np.linalg.norm (y7t_np_normalize_f64), np.dot as one FMA chain per pair (y7t_np_dot_f64)
// 0.5 * (1. - dot): a rounded difference, an exact halving
Y7T_FN double y7t_br_half(double dot) {
    Y7T_NO_CONTRACT
    const double d = 1.0 - dot;
    return 0.5 * d;
}
// equations 12-13 on one pair: App = half; App[IoU_dist > theta_iou] = 1; App[App > theta_emb] = 1; np.minimum(IoU_dist, App) (both comparisons strict, NaN passes)
Y7T_FN double y7t_br_gate(double iou_d, double half, double theta_iou, double theta_emb) {
    double app = half;
    if (iou_d > theta_iou) app = 1.0;
    if (app > theta_emb) app = 1.0;
    return (iou_d <= app || iou_d != iou_d) ? iou_d : app;
}
// np.linalg.norm of one float32 row, and the cosine of two, on their own (tests): norm[] holds 2 * dim doubles
Y7T_FN double y7t_br_norm(const float* x, int dim) { return y7t_np_norm_f64(x, dim); }
Y7T_FN double y7t_br_cosine(const float* u, const float* v, int dim, double* norm) {
    y7t_np_normalize_f64(u, dim, norm);
    y7t_np_normalize_f64(v, dim, norm + dim);
    return y7t_np_dot_f64(norm, norm + dim, dim);
}

// is detection row j one the reference extracts a feature for (botsort.py:339: score >= det_thresh, compared in float32)?
Y7T_FN bool y7t_br_row_used(const float* dets, int j, float det_t) { return dets[6 * (size_t)j + 4] >= det_t; }

// the frame's normalised rows (ex may span a whole grid: on the device a wave per row): the vectors of the slots of the tracked / lost lists and the detection
// rows at or above det_thresh.  They do not depend on the Kalman state, so this runs before the step.  A row that cannot be normalised sets Y7T_BR_ERR_VEC.
Y7T_FN void y7t_br_prepare(const Y7TExec& ex, const Y7TTrk& s, const Y7TBr& f, const float* dets, const float* det_feats, int n) {
    const int dim = f.h->ss.dim, cap_t = s.h->cfg.cap_t;
    const int nt0 = s.h->n_tracked < cap_t ? s.h->n_tracked : cap_t, nl0 = s.h->n_lost < cap_t ? s.h->n_lost : cap_t, n_live = nt0 + nl0;
    const float det_t = (float)s.h->cfg.det_thresh;
    if (n > f.h->ss.cap_d) n = f.h->ss.cap_d;
    if (n > s.h->cfg.cap_d) n = s.h->cfg.cap_d;
    const int rows = n_live + (n > 0 ? n : 0);
#if Y7T_DEVICE
    const int lane = ex.tid & 63;
    for (int r = ex.tid >> 6; r < rows; r += ex.nt >> 6) {      // wave-uniform
#else
    for (int r = ex.tid; r < rows; r += ex.nt) {
#endif
        const float* src;
        double* dst;
        if (r < n_live) {
            const int sl = y7t_ss_live_slot(s, nt0, r);
            if (sl < 0 || sl >= f.h->ss.cap_t) continue;
            src = f.ss.vec + (size_t)sl * dim; dst = f.tn + (size_t)sl * dim;
        } else {
            const int j = r - n_live;
            if (!y7t_br_row_used(dets, j, det_t)) continue;
            src = det_feats + (size_t)j * dim; dst = f.dn + (size_t)j * dim;
        }
#if Y7T_DEVICE
        const bool ok = y7t_np_wave_normalize_f64(src, dim, dst, lane);
        if (!ok && lane == 0) atomicOr(&f.h->ss.status, Y7T_BR_ERR_VEC);
#else
        if (!y7t_np_normalize_f64(src, dim, dst)) f.h->ss.status |= Y7T_BR_ERR_VEC;
#endif
    }
}

// ---- the association's pair table ----
#if Y7T_DEVICE
#define Y7T_BR_CAS(p, cmp, val) atomicCAS((p), (cmp), (val))
#define Y7T_BR_OR(p, v) atomicOr((p), (v))
#else
static inline int y7t_br_cas_host(int* p, int cmp, int val) { const int o = *p; if (o == cmp) *p = val; return o; }
#define Y7T_BR_CAS(p, cmp, val) y7t_br_cas_host((p), (cmp), (val))
#define Y7T_BR_OR(p, v) (*(p) |= (v))
#endif
Y7T_FN int y7t_br_hash(int key, int mask) { return (int)(((unsigned)key * 2654435761u) >> 7) & mask; }
// -> 0.5 * (1 - cos) of the pair, or 1 for a pair the table does not hold (it overflowed: Y7T_BR_ERR_PAIRS is set, the cost falls back to the IoU distance)
Y7T_FN double y7t_br_lookup(const Y7TBr& f, int key) {
    const int mask = f.h->hcap - 1;
    for (int e = y7t_br_hash(key, mask), probes = 0; probes <= mask; e = (e + 1) & mask, ++probes) {
        const int k = f.hkey[e];
        if (k == key) return f.hval[e];
        if (k < 0) break;
    }
    return 1.0;
}
// the fused cost of one pair from its IoU distance
Y7T_FN double y7t_br_cost(const Y7TBr& f, double iou_d, int i, int j, int nb, double theta_iou, double theta_emb) {
    if (iou_d > theta_iou) return y7t_br_gate(iou_d, 1.0, theta_iou, theta_emb);      // (no cosine was taken)
    return y7t_br_gate(iou_d, y7t_br_lookup(f, i * nb + j), theta_iou, theta_emb);
}

// an association's cosines: the pairs of the boxes gathered in ttlbr[0..na) / dtlbr[0..nb) with IoU_dist <= theta_iou are filed (the same pair pass as the IoU
// associations: a lane per column, the rows apart from a wave's strip of columns skipped 64 at a time), then a lane per filed pair runs its chain.
// slots[i] / drows[j]: the pool slot of row i, the detection row of column j (they name the normalised rows).
Y7T_FN void y7t_br_cosines(const Y7TExec& ex, const Y7TTrk& s, const Y7TBr& f, int na, int nb, const int* slots, const int* drows) {
    const int hcap = f.h->hcap, mask = hcap - 1, room = hcap - hcap / 4, dim = f.h->ss.dim;
    const double theta_iou = Y7T_BR_THETA_IOU(f.h), theta_emb = Y7T_BR_THETA_EMB(f.h);
    for (int e = ex.tid; e < hcap; e += ex.nt) f.hkey[e] = -1;
    if (ex.tid == 0) f.h->h_nb = nb;
    y7t_sync(ex);
    const int base = Y7T_BR_NDOTS(f.h);
    y7t_sync(ex);
    const int* colperm = nullptr;
#if Y7T_DEVICE
    if (nb > 128 && ex.nt >= 64 && (size_t)nb * 12 + 512 <= (size_t)s.h->cfg.cap_t * (s.h->cfg.cap_t > s.h->cfg.cap_d ? s.h->cfg.cap_t : s.h->cfg.cap_d) * 8) {      // (as y7t_assoc_sparse_try: the columns in the order of 64 bins of their left edge; keys, order and histogram in the idle dense cost matrix)
        double* key = s.cost;
        int* perm = (int*)(key + nb);
        int* hist = perm + nb;
        for (int j = ex.tid; j < nb; j += ex.nt) key[j] = s.dtlbr[4 * (size_t)j];
        y7t_sync(ex);
        y7t_bin_perm(ex, nb, key, perm, hist);
        colperm = perm;
    }
#endif
    y7t_pairs(ex, na, nb, [&](int j) { return y7t_box_col(s.dtlbr + 4 * (size_t)j); }, [&](int i) { return y7t_box_row(s.ttlbr + 4 * (size_t)i); },
              [&](int i, int j, const Y7TBoxR& rl, int r, const Y7TBoxC& cj) {
                  if (y7t_box_iou_dist(rl, r, cj) > theta_iou) return;
                  const int k = Y7T_FETCH_ADD(&Y7T_BR_NDOTS(f.h), 1) - base;
                  if (k >= room) { Y7T_BR_OR(&f.h->ss.status, Y7T_BR_ERR_PAIRS); return; }
                  const int key = i * nb + j;
                  int e = y7t_br_hash(key, mask);
                  while (Y7T_BR_CAS(&f.hkey[e], -1, key) != -1) e = (e + 1) & mask;      // (at most three quarters full: an empty entry exists)
                  f.hlist[k] = e;
              }, colperm, Y7TBoxGeo());
    y7t_sync(ex);
    int cnt = Y7T_BR_NDOTS(f.h) - base;
    y7t_sync(ex);
    if (cnt > room) { cnt = room; if (ex.tid == 0) Y7T_BR_NDOTS(f.h) = base + room; }      // (the counter says what was evaluated)
    int gated = 0;
    for (int k = ex.tid; k < cnt; k += ex.nt) {
        const int e = f.hlist[k], key = f.hkey[e];
        const int i = key / nb, j = key - i * nb;
        const double half = y7t_br_half(y7t_np_dot_f64(f.tn + (size_t)slots[i] * dim, f.dn + (size_t)drows[j] * dim, dim));
        f.hval[e] = half;
        gated += half > theta_emb ? 1 : 0;
    }
    if (gated) Y7T_ATOMIC_ADD(&f.h->n_emb, gated);
    y7t_sync(ex);
}

struct Y7TBrC { Y7TBoxC b; int j; };
struct Y7TBrR { Y7TBoxR b; int i; };
struct Y7TBrGeo {
    static constexpr bool on = true;
    using G = Y7TBoxGeo::G;
    Y7T_MFN G group(const Y7TBrC& c, bool valid) const { return Y7TBoxGeo().group(c.b, valid); }
    Y7T_MFN double key(const Y7TBrC& c) const { return c.b.v[0]; }
    Y7T_MFN bool near(const Y7TBrR& r, const G& g) const { return Y7TBoxGeo().near(r.b, g); }
};

// matching.linear_assignment(np.minimum(IoU_dist, App), thresh) for the boxes gathered in ttlbr / dtlbr -> xrow / ycol.  y7t_assoc with the fused cost: the cosines
// first (y7t_br_cosines), then the sparse component solver (a candidate costs <= thresh < 1, so its boxes overlap: the IoU geometry rejects as for IoU), the dense
// lapjv on the fused matrix where it declines, lapjv.cpp run literally on ties (as y7t_assoc_amf).
Y7T_FN void y7t_assoc_br(const Y7TExec& ex, const Y7TTrk& s, const Y7TBr& f, int na, int nb, double thresh, const int* slots, const int* drows) {
    if (na == 0 || nb == 0) {
        for (int i = ex.tid; i < na; i += ex.nt) s.xrow[i] = -1;
        for (int j = ex.tid; j < nb; j += ex.nt) s.ycol[j] = -1;
        y7t_sync(ex);
        return;
    }
    y7t_br_cosines(ex, s, f, na, nb, slots, drows);
    const double theta_iou = Y7T_BR_THETA_IOU(f.h), theta_emb = Y7T_BR_THETA_EMB(f.h);
    int sp = 0;
    if ((long long)na * nb >= Y7T_SPARSE_MIN &&
        (sp = y7t_assoc_sparse_fn(ex, s, na, nb, thresh,
                                  [&](int j) { return Y7TBrC{y7t_box_col(s.dtlbr + 4 * (size_t)j), j}; },
                                  [&](int i) { return Y7TBrR{y7t_box_row(s.ttlbr + 4 * (size_t)i), i}; },
                                  [&](const Y7TBrR& rl, int r, const Y7TBrC& q) {
                                      const double iou = y7t_box_iou_dist(rl.b, r, q.b);
                                      if (iou == 1.0) return 1.0;      // (apart)
                                      return y7t_br_cost(f, iou, y7t_row_at(rl.i, r), q.j, nb, theta_iou, theta_emb);
                                  }, Y7TBrGeo())) == 1)
        return;
    Y7TLap L;
    L.nr = na; L.nc = nb; L.ld = nb; L.n = na + nb; L.half = thresh / 2.0;
    L.prof = nullptr;
    const size_t ws = y7t_al(y7t_lap_ws_bytes(L.n)), cb = (size_t)na * nb * sizeof(double);
    void* lapws = s.lapws;
    double* cost = s.cost;
    size_t off = 0;
    if (ex.fast && ws <= ex.fast_bytes) { lapws = ex.fast; off = ws; }
    if (ex.fast && off + cb <= ex.fast_bytes) cost = (double*)(ex.fast + off);
    {   // (as y7t_cost_matrix: a lane per column, a wave per row residue)
        const int lanes = ex.nt < 64 ? ex.nt : 64, nw = ex.nt / lanes, wave = ex.tid / lanes, lane = ex.tid - wave * lanes;
        for (int j = lane; j < nb; j += lanes)
            for (int i = wave; i < na; i += nw)
                cost[(size_t)i * nb + j] = y7t_br_cost(f, y7t_iou_dist(s.ttlbr + 4 * (size_t)i, s.dtlbr + 4 * (size_t)j), i, j, nb, theta_iou, theta_emb);
        y7t_sync(ex);
    }
    L.c = cost;
    y7t_lap_bind(L, lapws, L.n);
    if (sp == 2 || y7t_lap_solve_sap(ex, L)) y7t_lap_solve_literal(ex, L);
    for (int i = ex.tid; i < na; i += ex.nt) s.xrow[i] = (L.x[i] >= nb) ? -1 : L.x[i];
    for (int j = ex.tid; j < nb; j += ex.nt) s.ycol[j] = (L.y[j] >= na) ? -1 : L.y[j];
    y7t_sync(ex);
}

// One frame (botsort.py:313-493, use_apperance_model = True).  dets: n x 6 float32 rows, n >= 0; det_feats: n x dim float32, row j = what get_feature returns for
// detection row j (rows below det_thresh are never read).  f.tn / f.dn must hold this frame's normalised rows (y7t_br_prepare).  gmc_warp: the frame's 2x3
// camera-motion matrix or null.  update_without_detection is the plain step's predict-only form (y7t_tracker_step, n < 0): this pool's lists are disjoint.
// (inlined into its one kernel, k_tracker_step_botsort_reid<MAXT>: a called function would not inherit the kernel's __launch_bounds__ -- see y7t_step_one, y7t_track_step.h)
Y7T_FN void y7t_tracker_step_botsort_reid(const Y7TExec& ex, void* blob, void* fblob, const float* dets, int n, const float* det_feats,
                                          double* out_rows, int out_cap, int* out_count, const double* gmc_warp) {
    Y7TTrkHdr* h = (Y7TTrkHdr*)blob;
    const Y7TTrkCfg cfg = h->cfg;
    const Y7TTrk s = y7t_trk_bind(blob, cfg.cap_t, cfg.cap_d);
    const Y7TBr f = y7t_br_bind(fblob);
    const int kf = cfg.kf;
    (void)det_feats;      // (the vectors are read by the launches around the step: y7t_br_prepare, y7t_ss_store_pending)
    // not this program's pool / a feature state too small for it / a vector that cannot be normalised (the reference would hand NaN costs to lapjv): refuse, loudly;
    // neither the pool nor the vectors change
    if (cfg.tracker != Y7T_BOTSORT_REID || n < 0 || f.h->ss.cap_t < cfg.cap_t || f.h->ss.cap_d < cfg.cap_d || (f.h->ss.status & Y7T_BR_ERR_VEC)) {
        if (ex.tid == 0) {
            if (cfg.tracker != Y7T_BOTSORT_REID || n < 0) h->status |= Y7T_ERR_KIND;
            else if (!(f.h->ss.status & Y7T_BR_ERR_VEC)) f.h->ss.status |= Y7T_PEND_ERR_CAP;
            else f.h->ss.n_pend = 0;      // (the store launch behind the step finds nothing queued)
            if (out_count) *out_count = 0;
        }
        return;
    }
    y7t_sync(ex);
    if (ex.tid == 0) {
        h->frame_id += 1;
        f.h->ss.n_pend = 0; Y7T_BR_NDOTS(f.h) = 0; f.h->n_emb = 0;
        h->n_act_last = h->n_refind_last = h->n_lostn_last = h->n_removed_last = 0;
        if (n > cfg.cap_d) h->status |= Y7T_ERR_CAP_D;
    }
    y7t_sync(ex);
    if (n > cfg.cap_d) n = cfg.cap_d;
    const int frame_id = h->frame_id;
    const int nt0 = h->n_tracked, nl0 = h->n_lost;
    Y7T_PROF(h, 0);
    const int n_unc = y7t_compact(ex, nt0, [&](int i) { return !s.act[s.tracked[i]]; }, s.tmpa, 0);
    for (int k = ex.tid; k < n_unc; k += ex.nt) s.unconf[k] = s.tracked[s.tmpa[k]];
    const int n_conf = y7t_compact(ex, nt0, [&](int i) { return s.act[s.tracked[i]] != 0; }, s.tmpb, 0);
    for (int k = ex.tid; k < n_conf; k += ex.nt) s.pool[k] = s.tracked[s.tmpb[k]];
    for (int k = ex.tid; k < nl0; k += ex.nt) s.pool[n_conf + k] = s.lost[k];      // (joint_stracks: the two lists are disjoint)
    y7t_sync(ex);
    const int n_pool = n_conf + nl0;
    y7t_multi_predict(ex, s, s.pool, n_pool);
    if (gmc_warp) {      // botsort.py:380-382: multi_gmc(strack_pool), multi_gmc(unconfirmed) -- after the prediction
        const Y7TWarp Hm = y7t_warp_load(gmc_warp);
        for (int i = ex.tid; i < n_pool + n_unc; i += ex.nt) {
            const int sl = i < n_pool ? s.pool[i] : s.unconf[i - n_pool];
            y7t_kf_gmc(Hm, s.mean + 8 * (size_t)sl, s.cov + 64 * (size_t)sl);
            s.f32m[sl] = 0;
        }
        y7t_sync(ex);
    }
    Y7T_PROF(h, 1);
    for (int j = ex.tid; j < n; j += ex.nt) {
        const float* r = dets + 6 * (size_t)j;
        s.dbox[4 * (size_t)j + 0] = r[0]; s.dbox[4 * (size_t)j + 1] = r[1];
        s.dbox[4 * (size_t)j + 2] = r[2] - r[0]; s.dbox[4 * (size_t)j + 3] = r[3] - r[1];
    }
    y7t_sync(ex);
    const float det_t = (float)cfg.det_thresh, low_t = (float)cfg.low_thresh;
    const float new_gate = (float)(cfg.det_thresh + 0.1);
    const int n_hi = y7t_compact(ex, n, [&](int j) { return y7t_br_row_used(dets, j, det_t); }, s.dhi, 0);
    const int n_lo = y7t_compact(ex, n, [&](int j) { const float c = dets[6 * (size_t)j + 4]; return !(c >= det_t) && c > low_t; }, s.dlo, 0);
    int na, nr, n_left = 0;
    // the three associations as ONE loop (y7t_tracker_step_body_t: one inlined copy of the solvers and of the Kalman updates)
    //   0: pool x high detections, fused, 0.9     1: every unmatched pool track x low detections, IoU, 0.5     2: unconfirmed x the high detections left, fused, 0.7
#if Y7T_DEVICE
#pragma clang loop unroll(disable)
#endif
    for (int ph = 0; ph < 3; ++ph) {
        const int* la; const int* ld;
        int nA, nD, mode;
        double th;
        if (ph == 0) { la = s.pool; nA = n_pool; ld = s.dhi; nD = n_hi; th = 0.9; mode = 0; }
        else if (ph == 1) {
            const int n_rem = y7t_compact(ex, n_pool, [&](int i) { return s.xrow[i] < 0; }, s.tmpa, 0);
            for (int k = ex.tid; k < n_rem; k += ex.nt) s.rem[k] = s.pool[s.tmpa[k]];
            y7t_sync(ex);
            la = s.rem; nA = n_rem; ld = s.dlo; nD = n_lo; th = 0.5; mode = 0;
        } else { la = s.unconf; nA = n_unc; ld = s.left; nD = n_left; th = 0.7; mode = 2; }
        y7t_gather_track_tlbr(ex, s, la, nA);
        y7t_gather_det_tlbr(ex, s, ld, nD);
        y7t_sync(ex);
        Y7T_PROF(h, 2 + 2 * ph);
        if (ph == 1) y7t_assoc(ex, s, nA, nD, th);
        else y7t_assoc_br(ex, s, f, nA, nD, th, la, ld);
        Y7T_PROF(h, 3 + 2 * ph);
        y7t_apply_matches(ex, s, la, nA, ld, dets, mode, na, nr);
        if (ph != 1) y7t_pend_queue_updates<Y7T_BR_PPD>(ex, s, y7t_pend_of(f.ss), la, nA, ld);      // (ph 1: det.has_feature is False -- the track keeps its vector)
        if (ph == 0) {
            n_left = y7t_compact(ex, n_hi, [&](int j) { return s.ycol[j] < 0; }, s.tmpa, 0);
            for (int k = ex.tid; k < n_left; k += ex.nt) s.left[k] = s.dhi[s.tmpa[k]];
            y7t_sync(ex);
        } else if (ph == 1) {
            const int nl_new = y7t_compact(ex, nA, [&](int i) { return s.xrow[i] < 0; }, s.tmpa, 0);
            for (int k = ex.tid; k < nl_new; k += ex.nt) { const int sl = s.rem[s.tmpa[k]]; s.lostn[k] = sl; s.state[sl] = Y7T_LOST; }
            if (ex.tid == 0) h->n_lostn_last = nl_new;
            y7t_sync(ex);
        } else {
            const int n_rm = y7t_compact(ex, n_unc, [&](int i) { return s.xrow[i] < 0; }, s.tmpa, 0);
            for (int k = ex.tid; k < n_rm; k += ex.nt) { const int sl = s.unconf[s.tmpa[k]]; s.removedl[k] = sl; s.state[sl] = Y7T_REMOVED; }
            if (ex.tid == 0) h->n_removed_last = n_rm;
            y7t_sync(ex);
        }
    }
    Y7T_PROF(h, 8);
    // new tracks from u_dets0 -- every detection left after the FIRST association -- with score > det_thresh + 0.1 (botsort.py:462-466; ids in order)
    {
        const int n_new = y7t_compact(ex, n_left, [&](int j) { return dets[6 * (size_t)s.left[j] + 4] > new_gate; }, s.tmpa, 0);
        int* idc = (int*)(uintptr_t)h->id_counter_ptr;
        if (ex.tid == 0) {
            int nf = h->n_free;
            const int base = h->n_act_last, made = n_new < nf ? n_new : nf;
            if (n_new > nf) h->status |= Y7T_ERR_CAP_T;
            const int id0 = made > 0 ? Y7T_FETCH_ADD(idc, made) : 0;
            for (int k = 0; k < made; ++k) {
                const int sl = s.freel[--nf];
                s.tmpb[k] = sl;
                s.tid[sl] = id0 + 1 + k;
                s.actl[base + k] = sl;
            }
            h->n_free = nf;
            h->n_act_last = base + made;
            s.xrow[0] = made;
        }
        y7t_sync(ex);
        const int made = s.xrow[0];
        for (int k = ex.tid; k < made; k += ex.nt) {
            const int sl = s.tmpb[k], dj = s.left[s.tmpa[k]];
            double z[4];
            for (int c = 0; c < 4; ++c) s.box[4 * (size_t)sl + c] = s.dbox[4 * (size_t)dj + c];
            y7t_meas(kf, s.dbox + 4 * (size_t)dj, z);
            y7t_kf_initiate(kf, z, cfg.f32_quirk, s.mean + 8 * (size_t)sl, s.cov + 64 * (size_t)sl);
            s.f32m[sl] = cfg.f32_quirk;
            s.score[sl] = dets[6 * (size_t)dj + 4];
            s.cls[sl] = dets[6 * (size_t)dj + 5];
            s.state[sl] = Y7T_TRACKED;
            s.act[sl] = (frame_id == 1) ? 1 : 0;
            s.frame[sl] = frame_id; s.start[sl] = frame_id;
            s.tsu[sl] = 0; s.len[sl] = 0; s.inrem[sl] = 0;
        }
        y7t_sync(ex);
        // STrack(..., feature=f): features = [f] (the raw vector, basetrack.py:97-103): whatever the slot's previous occupant left is overwritten
        y7t_pend_queue<Y7T_BR_PPD>(ex, y7t_pend_of(f.ss), made, 0, [&](int k, int& sl, int& row) {
            sl = s.tmpb[k];
            row = s.left[s.tmpa[k]];
            return true;
        });
    }
    // age out long-lost tracks (botsort.py:469-472)
    {
        const int n_old = y7t_compact(ex, nl0, [&](int i) { return frame_id - s.frame[s.lost[i]] > cfg.max_time_lost; }, s.tmpa, 0);
        const int base = h->n_removed_last;
        for (int k = ex.tid; k < n_old; k += ex.nt) { const int sl = s.lost[s.tmpa[k]]; s.removedl[base + k] = sl; s.state[sl] = Y7T_REMOVED; }
        y7t_sync(ex);
        if (ex.tid == 0) h->n_removed_last = base + n_old;
        y7t_sync(ex);
    }
    Y7T_PROF(h, 9);
    y7t_finish(ex, s, out_rows, out_cap, out_count);
    Y7T_PROF(h, 10);
}
