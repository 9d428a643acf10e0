// y7t_track_strongsort.h -- StrongSORT's per-frame association (one smoothed appearance vector per track, Euclidean appearance distance fused
// with the IoU distance) as a workgroup program over the same device-resident track pool as the other trackers (y7t_track_step.h).
// Portable text (device: hipcc; CPU tests: -DY7T_HOSTSIM).
//
// Restates /root/reference/tracker/strongsort.py:91-250 (StrongSORT.update), tracker/matching.py:84-103 (embedding_distance, metric
// 'euclidean': np.maximum(0.0, scipy cdist) of features[-1] cast to float64), tracker/basetrack.py:324-332 (STrack.update with
// use_avg_of_feature=True: the float32 moving average of the normalised features), tracker/botsort.py:250-269 (multi_gmc).
//
// Reference behaviours that decide WHICH tracks are touched, reproduced literally:
//   * multi_gmc runs BEFORE multi_predict and on strack_pool only (strongsort.py:138-145; BoT-SORT: after, and on the unconfirmed tracks too);
//   * strongsort.py:195-198 marks `strack_pool[idx]` lost for idx in the unmatched ROWS of u_tracks0 (an index into the filtered list applied to
//     the unfiltered pool): a track the first association has just updated may be marked lost, the real leftovers stay Tracked with a stale frame_id;
//   * only STrack.update touches the appearance vector: re_activate keeps it, a new track starts with the detection's RAW (unnormalised) vector, and
//     the first update mixes that raw vector with a normalised one.
#pragma once
#include "y7t_track_step.h"
#include "y7t_track_pend.h"      // the header's first words, the queue of vectors to store
#include "y7t_np_arith.h"        // scipy's cdist, OpenBLAS's sdot, the float32 mix, Y7T_NO_CONTRACT

// (Y7T_STRONGSORT = 6: y7t_track_core.h)
#ifndef Y7T_SS_STAT
#define Y7T_SS_STAT(k) do { } while (0)      // (the CPU test build counts which solver path a fused association took)
#endif

// feature state of one StrongSORT tracker: caller-owned device memory next to the track-pool blob
struct Y7TSsHdr : Y7TPendHdr { int pad1; double gamma; double pad2; };
static_assert(sizeof(Y7TSsHdr) == 28 + 4 + 8 + 8, "StrongSORT's feature-state header: the shared words, pad1 at byte 28, gamma at 32, pad2 at 40");
struct Y7TSsLayout { size_t vec, app, pend, total; };
struct Y7TSs {
    Y7TSsHdr* h;
    float* vec;         // [cap_t][dim]      STrack.features[-1] of the slot's track: the raw vector of its first detection, later the smoothed one
    double* app;        // [cap_t][cap_d]    embedding_distance(slot, detection row) of this frame (rows: the slots of the tracked / lost lists; columns: rows above det_thresh)
    int* pend;          // [cap_d][3]        vectors this frame's step decided to store: (slot, detection row, 1 = update (moving average) / 0 = new track (raw copy)): the queue of y7t_track_pend.h
};

Y7T_HD Y7TSsLayout y7t_ss_layout(int cap_t, int cap_d, int dim) {
    Y7TSsLayout L;
    size_t o = y7t_al(sizeof(Y7TSsHdr));
    const size_t T = (size_t)cap_t, D = (size_t)cap_d;
#define Y7T_TAKE(f, bytes) L.f = o; o = y7t_al(o + (bytes));
    Y7T_TAKE(vec, T * dim * 4) Y7T_TAKE(app, T * D * 8) Y7T_TAKE(pend, D * 3 * 4)
#undef Y7T_TAKE
    L.total = o;
    return L;
}

Y7T_FN Y7TSs y7t_ss_bind(void* blob) {
    Y7TSsHdr* h = (Y7TSsHdr*)blob;
    const Y7TSsLayout L = y7t_ss_layout(h->cap_t, h->cap_d, h->dim);
    char* b = (char*)blob;
    Y7TSs f;
    f.h = h; f.vec = (float*)(b + L.vec); f.app = (double*)(b + L.app); f.pend = (int*)(b + L.pend);
    return f;
}

Y7T_FN void y7t_ss_init(const Y7TExec& ex, void* blob, int cap_t, int cap_d, int dim, double gamma) {
    Y7TSsHdr* h = (Y7TSsHdr*)blob;
    if (ex.tid == 0) { h->magic = 0x59375331; h->dim = dim; h->budget = 1; h->cap_t = cap_t; h->cap_d = cap_d; h->status = 0; h->n_pend = 0; h->pad1 = 0; h->gamma = gamma; h->pad2 = 0.0; }
    y7t_sync(ex);
}

// Dist_mat = self.gamma * IoU_dist + (1. - self.gamma) * Apperance_dist (strongsort.py:152): two rounded products and one sum
Y7T_FN double y7t_ss_fuse(double gamma, double iou_d, double app_d) {
    Y7T_NO_CONTRACT
    const double a = gamma * iou_d, w = 1.0 - gamma;
    const double b = w * app_d;
    return a + b;
}

// is detection row j one the reference extracts a feature for (strongsort.py:110: conf > det_thresh, compared in float32)?  Every other row of det_feats is never read
Y7T_FN bool y7t_ss_row_used(const float* dets, int j, float det_t) { return dets[6 * (size_t)j + 4] > det_t; }

// matching.embedding_distance(..., 'euclidean') of one pair: scipy's cdist (y7t_np_arith.h)
Y7T_FN double y7t_ss_dist(const float* u, const float* v, int dim) { return y7t_scipy_euclidean(u, v, dim); }

// the slot behind rank r of a frame's appearance rows: the tracked list, then the lost list (a slot in both lists is computed twice, to the same value)
Y7T_FN int y7t_ss_live_slot(const Y7TTrk& s, int n_tracked, int r) { return r < n_tracked ? s.tracked[r] : s.lost[r - n_tracked]; }

// Plain form of the frame's appearance matrix (a lane per pair): every slot of the tracked / lost lists x every detection row above det_thresh.
// The device runs the tiled k_ss_appearance (y7t_tracker.hip) with the same chains instead; feature dimensions that are not a multiple of its k chunk come here.
Y7T_FN void y7t_ss_appearance_plain(const Y7TExec& ex, const Y7TTrk& s, const Y7TSs& f, const float* dets, const float* det_feats, int n) {
    const int dim = f.h->dim, nt0 = s.h->n_tracked, n_live = nt0 + s.h->n_lost;
    const float det_t = (float)s.h->cfg.det_thresh;
    if (n > f.h->cap_d) n = f.h->cap_d;
    if (n > s.h->cfg.cap_d) n = s.h->cfg.cap_d;
    const long long tot = (long long)n_live * (n > 0 ? n : 0);
    for (long long e = ex.tid; e < tot; e += ex.nt) {
        const int r = (int)(e / n), j = (int)(e - (long long)r * n);
        const int sl = y7t_ss_live_slot(s, nt0, r);
        if (sl < 0 || sl >= f.h->cap_t || !y7t_ss_row_used(dets, j, det_t)) continue;
        f.app[(size_t)sl * f.h->cap_d + j] = y7t_ss_dist(f.vec + (size_t)sl * dim, det_feats + (size_t)j * dim, dim);
    }
}

// The one-vector store: vec[cap_t][dim] holds STrack.features[-1] of the slot's track -- the raw vector of its first detection, later the smoothed one.
// STrack.update's feature bookkeeping (basetrack.py:324-332, use_avg_of_feature = True), all float32 as numpy evaluates it:
//   f = raw / np.linalg.norm(raw);  smooth = 0.9 * features[-1] + (1 - 0.9) * f;  smooth /= np.linalg.norm(smooth)
// (y7t_np_mix_f32; np.linalg.norm of a float32 vector is sqrt(sdot(x, x)): y7t_blas_sdot_self).  In place on the slot's vector.  Serial (one thread).
Y7T_FN void y7t_ss_ema(float* vec, const float* raw, int dim) {
    const float nb = sqrtf(y7t_blas_sdot_self(raw, dim));
    for (int d = 0; d < dim; ++d) vec[d] = y7t_np_mix_f32(vec[d], raw[d] / nb);
    const float ns = sqrtf(y7t_blas_sdot_self(vec, dim));
    for (int d = 0; d < dim; ++d) vec[d] = vec[d] / ns;
}

// write the queued vectors (ex may span a whole grid: on the device a wave per vector): the moving average for an update, the raw copy for a new track.  The
// entries are independent (see y7t_pend_queue).
template <int PPD = 1>
Y7T_FN void y7t_ss_store_pending(const Y7TExec& ex, const Y7TSs& f, const float* det_feats) {
    const Y7TPend q = y7t_pend_of(f);
    const int dim = q.h->dim;
    const int count = y7t_pend_count<PPD>(q);
#if Y7T_DEVICE
    if (y7t_dim_wave_ok(dim) && (ex.nt & 63) == 0) {      // 128 / 256 / 512 / 1024: a lane owns elements lane, lane + 64, ... (at most 16) in registers
        const int lane = ex.tid & 63, nc = dim >> 6;
        for (int i = ex.tid >> 6; i < count; i += ex.nt >> 6) {          // wave-uniform
            const int sl = q.pend[3 * i], update = q.pend[3 * i + 2];
            const float* b = det_feats + (size_t)q.pend[3 * i + 1] * dim;
            float* dst = f.vec + (size_t)sl * dim;
            if (sl < 0 || sl >= q.h->cap_t) continue;
            float raw[16], sm[16];
            float a5 = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) if (c < nc) { raw[c] = b[lane + 64 * c]; a5 = y7t_fmaf(raw[c], raw[c], a5); }
            if (!update) {
#pragma unroll
                for (int c = 0; c < 16; ++c) if (c < nc) dst[lane + 64 * c] = raw[c];
                continue;
            }
            const float nb = sqrtf(y7t_blas_wave_sdot_fold(y7t_blas_wave_sdot_halve(a5, lane), lane));
            a5 = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) if (c < nc) { sm[c] = y7t_np_mix_f32(dst[lane + 64 * c], raw[c] / nb); a5 = y7t_fmaf(sm[c], sm[c], a5); }
            const float ns = sqrtf(y7t_blas_wave_sdot_fold(y7t_blas_wave_sdot_halve(a5, lane), lane));
#pragma unroll
            for (int c = 0; c < 16; ++c) if (c < nc) dst[lane + 64 * c] = sm[c] / ns;
        }
        return;
    }
#endif
    for (int i = ex.tid; i < count; i += ex.nt) {
        const int sl = q.pend[3 * i], update = q.pend[3 * i + 2];
        if (sl < 0 || sl >= q.h->cap_t) continue;
        const float* b = det_feats + (size_t)q.pend[3 * i + 1] * dim;
        float* dst = f.vec + (size_t)sl * dim;
        if (update) y7t_ss_ema(dst, b, dim);
        else for (int d = 0; d < dim; ++d) dst[d] = b[d];
    }
}

// the fused pair: a box with the slot / detection row that names its entry of the appearance matrix (y7t_pairs contexts).  No geometry: boxes apart
// cost gamma + (1 - gamma) * appearance, which an identical appearance brings under the limit
struct Y7TSsC { Y7TBoxC b; int row; };
struct Y7TSsR { Y7TBoxR b; int slot; };

// matching.linear_assignment(gamma * iou_distance + (1. - gamma) * embedding_distance, thresh) for the boxes gathered in ttlbr / dtlbr of the tracks in
// slots[0..na) and the detection rows drows[0..nb) -> xrow / ycol.  y7t_assoc with the fused cost: the sparse component solver first (candidates: pairs
// at or under the limit -- a dearer pair is beaten by leaving both sides unmatched), the dense lapjv on the fused matrix when a row has more candidates
// than the lists hold or a pair sits at the limit, lapjv.cpp run literally on ties (exactly UAVMOT's AMF pass, y7t_assoc_amf).
Y7T_FN void y7t_assoc_ss(const Y7TExec& ex, const Y7TTrk& s, int na, int nb, double thresh, const int* slots, const int* drows, double gamma, const double* app, int app_ld) {
    if (na == 0 || nb == 0) {
        for (int i = ex.tid; i < na; i += ex.nt) s.xrow[i] = -1;
        for (int j = ex.tid; j < nb; j += ex.nt) s.ycol[j] = -1;
        y7t_sync(ex);
        return;
    }
    int sp = 0;
    if ((long long)na * nb >= Y7T_SPARSE_MIN) {
        sp = y7t_assoc_sparse_fn(ex, s, na, nb, thresh,
                                 [&](int j) { return Y7TSsC{y7t_box_col(s.dtlbr + 4 * (size_t)j), drows[j]}; },
                                 [&](int i) { return Y7TSsR{y7t_box_row(s.ttlbr + 4 * (size_t)i), slots[i]}; },
                                 [&](const Y7TSsR& rl, int r, const Y7TSsC& q) {
                                     const double iou = y7t_box_iou_dist(rl.b, r, q.b);
                                     return y7t_ss_fuse(gamma, iou, app[(size_t)y7t_row_at(rl.slot, r) * app_ld + q.row]);
                                 });
        if (sp == 1) { Y7T_SS_STAT(0); return; }
        Y7T_SS_STAT(sp == 2 ? 2 : 1);
    } else Y7T_SS_STAT(3);
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
                cost[(size_t)i * nb + j] = y7t_ss_fuse(gamma, y7t_iou_dist(s.ttlbr + 4 * (size_t)i, s.dtlbr + 4 * (size_t)j), app[(size_t)slots[i] * app_ld + drows[j]]);
        y7t_sync(ex);
    }
    // tie watch.  Appearance vectors repeat exactly (two detections with one feature, two tracks born from such detections, every pair of boxes apart sharing the
    // IoU distance 1), so one row equally far from two columns -- or one column from two rows -- at or under the limit is an everyday event here, and which of the equal
    // optima lapjv returns is a property of its own scan order: such a problem goes to lapjv.cpp run literally.  (The sparse solver watches its candidate lists the same
    // way; the dense solver's own watch only looks at problems of up to Y7T_TIE_FULL_N rows + columns.)
    bool tied = sp == 2;
    if (!tied) {
        int* flag = s.xrow;      // (written below)
        if (ex.tid == 0) flag[0] = 0;
        y7t_sync(ex);
        for (int k = ex.tid; k < na + nb; k += ex.nt) {
            const bool row = k < na;
            const int n = row ? nb : na;
            const double* p = row ? cost + (size_t)k * nb : cost + (k - na);
            const size_t st = row ? 1 : (size_t)nb;
            bool dup = false;
            for (int a = 1; a < n && !dup; ++a) {
                const double c = p[a * st];
                if (!(c <= thresh)) continue;
                for (int b = 0; b < a; ++b) dup |= y7t_near(p[b * st], c);
            }
            if (dup) { flag[0] = 1; Y7T_TIE_REASON(6); }
        }
        y7t_sync(ex);
        tied = flag[0] != 0;
        y7t_sync(ex);
    }
    L.c = cost;
    y7t_lap_bind(L, lapws, L.n);
    if (tied || y7t_lap_solve_sap(ex, L)) y7t_lap_solve_literal(ex, L);
    for (int i = ex.tid; i < na; i += ex.nt) s.xrow[i] = (L.x[i] >= nb) ? -1 : L.x[i];
    for (int j = ex.tid; j < nb; j += ex.nt) s.ycol[j] = (L.y[j] >= na) ? -1 : L.y[j];
    y7t_sync(ex);
}

// One StrongSORT frame (strongsort.py:91-250).  dets: n x 6 float32 rows; det_feats: n x dim float32, row j = what get_feature returns for detection
// row j (rows with conf <= det_thresh are never read).  f.app must hold this frame's appearance distances (y7t_ss_appearance_plain / k_ss_appearance for
// every slot of the tracked / lost lists) -- they do not depend on the Kalman state.  gmc_warp: the frame's 2x3 camera-motion matrix or null.
// n < 0: update_without_detection -- the prediction of the (deduplicated) pool and the list bookkeeping; fblob, dets and det_feats are not touched.
// (inlined into its one kernel, k_tracker_step_strongsort<MAXT>: a called function would not inherit the kernel's __launch_bounds__ -- see y7t_step_one, y7t_track_step.h)
Y7T_FN void y7t_tracker_step_strongsort(const Y7TExec& ex, void* blob, void* fblob, const float* dets, int n, const float* det_feats,
                                        double* out_rows, int out_cap, int* out_count, const double* gmc_warp) {
    Y7TTrkHdr* h = (Y7TTrkHdr*)blob;
    const Y7TTrkCfg cfg = h->cfg;
    const Y7TTrk s = y7t_trk_bind(blob, cfg.cap_t, cfg.cap_d);
    const bool predict_only = n < 0;      // update_without_detection (basetrack.py:489-537): no feature state is needed or touched (fblob may be null)
    Y7TSs f;
    f.h = nullptr; f.vec = nullptr; f.app = nullptr; f.pend = nullptr;
    if (!predict_only) f = y7t_ss_bind(fblob);
    const int kf = cfg.kf;
    if (cfg.tracker != Y7T_STRONGSORT || (!predict_only && (f.h->cap_t < cfg.cap_t || f.h->cap_d < cfg.cap_d))) {      // not this program's pool / a feature state too small for it: refuse, loudly
        if (ex.tid == 0) {
            if (cfg.tracker != Y7T_STRONGSORT) h->status |= Y7T_ERR_KIND; else f.h->status |= Y7T_PEND_ERR_CAP;
            if (out_count) *out_count = 0;
        }
        return;
    }
    const double gamma = predict_only ? 0.0 : f.h->gamma;
    const double* app = f.app;
    const int app_ld = predict_only ? 0 : f.h->cap_d;
    y7t_sync(ex);
    if (ex.tid == 0) {
        h->frame_id += 1;
        if (!predict_only) f.h->n_pend = 0;
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
    // strack_pool = joint_stracks(confirmed, lost) drops a lost entry whose id is among the confirmed ones: here the lists are NOT disjoint -- the index quirk below puts a
    // track into both, and remove_duplicate_stracks takes it out of one only when its box overlaps itself, which a box of negative width (multi_gmc turns the xyah pair
    // (a, h) like a point) does not
    for (int k = ex.tid; k < cfg.cap_t; k += ex.nt) s.mark[k] = 0;
    y7t_sync(ex);
    for (int k = ex.tid; k < n_conf; k += ex.nt) s.mark[s.pool[k]] = 1;
    y7t_sync(ex);
    const int n_lp = y7t_compact(ex, nl0, [&](int i) { return !s.mark[s.lost[i]]; }, s.tmpa, 0);
    for (int k = ex.tid; k < n_lp; k += ex.nt) s.pool[n_conf + k] = s.lost[s.tmpa[k]];
    y7t_sync(ex);
    const int n_pool = n_conf + n_lp;
    if (predict_only) {      // the plain step's predict-only form with THIS pool: the other trackers' lists are disjoint and their step does not look
        y7t_multi_predict(ex, s, s.pool, n_pool);
        y7t_finish(ex, s, out_rows, out_cap, out_count);
        return;
    }
    if (gmc_warp) {      // strongsort.py:141-142: multi_gmc(strack_pool, warp) -- before the prediction, the pool only
        const Y7TWarp Hm = y7t_warp_load(gmc_warp);
        for (int i = ex.tid; i < n_pool; i += ex.nt) {
            const int sl = s.pool[i];
            y7t_kf_gmc(Hm, s.mean + 8 * (size_t)sl, s.cov + 64 * (size_t)sl);
            s.f32m[sl] = 0;
        }
        y7t_sync(ex);
    }
    y7t_multi_predict(ex, s, s.pool, n_pool);
    Y7T_PROF(h, 1);
    // detections with conf > det_thresh (strongsort.py:110), float32 tlwh
    for (int j = ex.tid; j < n; j += ex.nt) {
        const float* r = dets + 6 * (size_t)j;
        s.dbox[4 * (size_t)j + 0] = r[0]; s.dbox[4 * (size_t)j + 1] = r[1];
        s.dbox[4 * (size_t)j + 2] = r[2] - r[0]; s.dbox[4 * (size_t)j + 3] = r[3] - r[1];
    }
    y7t_sync(ex);
    const float det_t = (float)cfg.det_thresh;
    const float new_gate = (float)(cfg.det_thresh + 0.1);
    const int n_hi = y7t_compact(ex, n, [&](int j) { return dets[6 * (size_t)j + 4] > det_t; }, s.dhi, 0);
    int na, nr;
    // ---- Step 2: strack_pool x detections, the fused cost at 0.7 (Tracked -> update, Lost -> re_activate) ----
    y7t_gather_track_tlbr(ex, s, s.pool, n_pool);
    y7t_gather_det_tlbr(ex, s, s.dhi, n_hi);
    y7t_sync(ex);
    Y7T_PROF(h, 2);
    y7t_assoc_ss(ex, s, n_pool, n_hi, 0.7, s.pool, s.dhi, gamma, app, app_ld);
    Y7T_PROF(h, 3);
    y7t_apply_matches(ex, s, s.pool, n_pool, s.dhi, dets, 0, na, nr);
    y7t_pend_queue_updates(ex, s, y7t_pend_of(f), s.pool, n_pool, s.dhi);
    // ---- Step 3: the still-Tracked leftovers (u_tracks0) x the leftover detections, IoU at 0.5 ----
    const int n_left = y7t_compact(ex, n_hi, [&](int j) { return s.ycol[j] < 0; }, s.tmpb, 0);
    for (int k = ex.tid; k < n_left; k += ex.nt) s.left[k] = s.dhi[s.tmpb[k]];
    y7t_sync(ex);
    const int n_t0 = y7t_compact(ex, n_pool, [&](int i) { return s.xrow[i] < 0 && s.state[s.pool[i]] == Y7T_TRACKED; }, s.tmpa, 0);
    for (int k = ex.tid; k < n_t0; k += ex.nt) s.rem[k] = s.pool[s.tmpa[k]];
    y7t_sync(ex);
    y7t_gather_track_tlbr(ex, s, s.rem, n_t0);
    y7t_gather_det_tlbr(ex, s, s.left, n_left);
    y7t_sync(ex);
    Y7T_PROF(h, 4);
    y7t_assoc(ex, s, n_t0, n_left, 0.5);
    y7t_apply_matches(ex, s, s.rem, n_t0, s.left, dets, 0, na, nr);
    y7t_pend_queue_updates(ex, s, y7t_pend_of(f), s.rem, n_t0, s.left);
    Y7T_PROF(h, 5);
    // u_det1 (detection rows), in column order
    const int n_d1 = y7t_compact(ex, n_left, [&](int c) { return s.ycol[c] < 0; }, s.tmpb, 0);
    for (int k = ex.tid; k < n_d1; k += ex.nt) s.dlo[k] = s.left[s.tmpb[k]];
    y7t_sync(ex);
    // ---- Step 4: `for idx in u_tracks1_idx: track = strack_pool[idx]` (sic, strongsort.py:195-198): the unmatched ROW NUMBERS of u_tracks0 index the pool ----
    {
        const int nl_new = y7t_compact(ex, n_t0, [&](int r) { return s.xrow[r] < 0; }, s.tmpa, 0);
        for (int k = ex.tid; k < nl_new; k += ex.nt) s.lostn[k] = s.pool[s.tmpa[k]];
        y7t_sync(ex);
        for (int k = ex.tid; k < nl_new; k += ex.nt) s.state[s.lostn[k]] = Y7T_LOST;
        if (ex.tid == 0) h->n_lostn_last = nl_new;
        y7t_sync(ex);
    }
    // unconfirmed tracks x u_det1, the fused cost at 0.7: update only, the rest removed
    y7t_gather_track_tlbr(ex, s, s.unconf, n_unc);
    y7t_gather_det_tlbr(ex, s, s.dlo, n_d1);
    y7t_sync(ex);
    Y7T_PROF(h, 6);
    y7t_assoc_ss(ex, s, n_unc, n_d1, 0.7, s.unconf, s.dlo, gamma, app, app_ld);
    y7t_apply_matches(ex, s, s.unconf, n_unc, s.dlo, dets, 2, na, nr);
    y7t_pend_queue_updates(ex, s, y7t_pend_of(f), s.unconf, n_unc, s.dlo);
    Y7T_PROF(h, 7);
    {
        const int n_rm = y7t_compact(ex, n_unc, [&](int i) { return s.xrow[i] < 0; }, s.tmpa, 0);
        for (int k = ex.tid; k < n_rm; k += ex.nt) { const int sl = s.unconf[s.tmpa[k]]; s.removedl[k] = sl; s.state[sl] = Y7T_REMOVED; }
        if (ex.tid == 0) h->n_removed_last = n_rm;
        y7t_sync(ex);
    }
    // new tracks from u_det2 with score > det_thresh + 0.1 (strongsort.py:218-222; ids in order)
    {
        const int n_new = y7t_compact(ex, n_d1, [&](int j) { return s.ycol[j] < 0 && dets[6 * (size_t)s.dlo[j] + 4] > new_gate; }, s.tmpa, 0);
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
            const int sl = s.tmpb[k], dj = s.dlo[s.tmpa[k]];
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
        y7t_pend_queue(ex, y7t_pend_of(f), made, 0, [&](int k, int& sl, int& row) {
            sl = s.tmpb[k];
            row = s.dlo[s.tmpa[k]];
            return true;
        });
    }
    // age out long-lost tracks (strongsort.py:226-229)
    Y7T_PROF(h, 8);
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
