// y7t_track_deepmot.h -- DeepMOT's per-frame association (the first association's cost is 1 - DHN(distance matrix), the Deep Hungarian Net of csrc/y7t_dhn.hip)
// as TWO workgroup programs over the same device-resident track pool as the other trackers (y7t_track_step.h), one on either side of the network.
// Portable text (device: hipcc; CPU tests: -DY7T_HOSTSIM).
//
// Restates /root/reference/tracker/deepmot.py:161-324 (DeepMOT.update) and tracker/matching.py:129-162 (ecu_iou_distance).
//   front   the detection filter, the lists, multi_predict, and Dist_mat = ecu_iou_distance(strack_pool, D_high, ori_img.shape[:2]) in float64, written as the
//           float32 h x w matrix the network reads (deepmot.py:226: torch.tensor(Dist_mat, dtype=torch.float32)).  The pool order, the high / low detection lists,
//           the unconfirmed list and the detections' float32 tlwh stay in the blob's work arrays; the frame's counts in the first words of its cost array.
//   back    matching.linear_assignment(1.0 - DHN(D), 0.9) -- float32 `1.0 - x`, cast to float64 by lapjv -- then ByteTrack's second association (IoU at 0.5 against
//           the low detections), the unconfirmed one (IoU at 0.7), the new tracks and the bookkeeping.
// Reference behaviours that decide WHICH tracks are touched, reproduced literally:
//   * deepmot.py:269-272 marks `strack_pool[idx]` lost for idx in the unmatched ROWS of u_tracks0 (an index into the filtered list applied to the unfiltered pool), as
//     uavmot.py:222-225 and strongsort.py:195-198 do;
//   * where the pool or D_high is empty the network is skipped and the (empty) ecu matrix is solved: nothing matches.
#pragma once
#include "y7t_track_step.h"
#include "y7t_np_arith.h"      // Y7T_NO_CONTRACT

// (Y7T_DEEPMOT = 7: y7t_track_core.h)
enum { Y7T_ERR_DHN_CAP = 32 /* the frame's h x w matrix exceeds the DHN object's workspace */, Y7T_ERR_DHN = 64 /* the network's forward gave up (a bounded spin ran out) */ };

// the frame's counts, front -> back: ints at the head of the blob's cost array (which the back program only uses from its first association on)
struct Y7TDmFrame { int magic, n, n_pool, n_hi, n_lo, n_unc, net, pad; };      // net: 1 = the network runs on n_pool x n_hi
#define Y7T_DM_MAGIC 0x59374d31

// matching.ecu_iou_distance's image term: float((h**2 + w**2)**0.5) of Python ints
Y7T_FN double y7t_dm_norm_factor(int img_h, int img_w) { return sqrt((double)((long long)img_h * img_h + (long long)img_w * img_w)); }

// one element of ecu_iou_distance as numpy evaluates it (matching.py:145-161).  t: the track's float64 tlwh (a predicted pool track: basetrack.py:185-197);
// b: the detection's float32 tlwh.  det_cx = b[0] + 0.5 * b[2] in FLOAT32 (a float32 array and a Python scalar), trk_cx in float64; their difference in float64
// (a float32 array minus a float64 scalar), squared, summed, sqrt; 1 - exp(-5 d / norm); 0.5 * (ecu + iou)
Y7T_FN double y7t_dm_ecu_iou(const double* t, const float* b, double iou_d, double norm) {
    Y7T_NO_CONTRACT
    const float hw = 0.5f * b[2], hh = 0.5f * b[3];
    const float dcx = b[0] + hw, dcy = b[1] + hh;
    const double tw = 0.5 * t[2], th = 0.5 * t[3];
    const double tcx = t[0] + tw, tcy = t[1] + th;
    const double dx = (double)dcx - tcx, dy = (double)dcy - tcy;
    const double xx = dx * dx, yy = dy * dy;
    const double dist = sqrt(xx + yy);
    const double m = -5.0 * dist;
    const double e = 1.0 - exp(m / norm);
    return 0.5 * (e + iou_d);
}

// the refusal both programs share: not a DeepMOT pool
Y7T_FN bool y7t_dm_refuse(const Y7TExec& ex, Y7TTrkHdr* h, int* out_count) {
    if (h->cfg.tracker == Y7T_DEEPMOT) return false;
    if (ex.tid == 0) { h->status |= Y7T_ERR_KIND; if (out_count) *out_count = 0; }
    return true;
}

// ---- front: deepmot.py:173-221.  D: d_cap floats; hw[0..1] <- rows, columns of the matrix the network is to run on (0, 0: skipped) ----
Y7T_FN void y7t_deepmot_front(const Y7TExec& ex, void* blob, const float* dets, int n, int img_h, int img_w, float* D, long long d_cap, int* hw) {
    Y7TTrkHdr* h = (Y7TTrkHdr*)blob;
    const Y7TTrkCfg cfg = h->cfg;
    if (ex.tid == 0 && hw) { hw[0] = 0; hw[1] = 0; }
    if (y7t_dm_refuse(ex, h, nullptr)) return;
    const Y7TTrk s = y7t_trk_bind(blob, cfg.cap_t, cfg.cap_d);
    Y7TDmFrame* fr = (Y7TDmFrame*)s.cost;
    y7t_sync(ex);
    if (ex.tid == 0) {
        h->frame_id += 1;
        h->n_act_last = h->n_refind_last = h->n_lostn_last = h->n_removed_last = 0;
        if (n > cfg.cap_d) h->status |= Y7T_ERR_CAP_D;
    }
    y7t_sync(ex);
    if (n > cfg.cap_d) n = cfg.cap_d;
    const int nt0 = h->n_tracked, nl0 = h->n_lost;
    // unconfirmed / confirmed split of tracked (deepmot.py:206-212); strack_pool = joint_stracks(confirmed, lost)
    const int n_unc = y7t_compact(ex, nt0, [&](int i) { return !s.act[s.tracked[i]]; }, s.tmpa, 0);
    for (int k = ex.tid; k < n_unc; k += ex.nt) s.unconf[k] = s.tracked[s.tmpa[k]];
    const int n_conf = y7t_compact(ex, nt0, [&](int i) { return s.act[s.tracked[i]] != 0; }, s.tmpb, 0);
    for (int k = ex.tid; k < n_conf; k += ex.nt) s.pool[k] = s.tracked[s.tmpb[k]];
    for (int k = ex.tid; k < nl0; k += ex.nt) s.pool[n_conf + k] = s.lost[k];
    y7t_sync(ex);
    const int n_pool = n_conf + nl0;
    y7t_multi_predict(ex, s, s.pool, n_pool);
    // detections -> STrack(cls, tlbr2tlwh(tlbr), score): float32 tlwh
    for (int j = ex.tid; j < n; j += ex.nt) {
        const float* r = dets + 6 * (size_t)j;
        s.dbox[4 * (size_t)j + 0] = r[0];
        s.dbox[4 * (size_t)j + 1] = r[1];
        s.dbox[4 * (size_t)j + 2] = r[2] - r[0];
        s.dbox[4 * (size_t)j + 3] = r[3] - r[1];
    }
    y7t_sync(ex);
    const float det_t = (float)cfg.det_thresh, low_t = (float)cfg.low_thresh;
    const int n_hi = y7t_compact(ex, n, [&](int j) { return dets[6 * (size_t)j + 4] >= det_t; }, s.dhi, 0);
    const int n_lo = y7t_compact(ex, n, [&](int j) { const float c = dets[6 * (size_t)j + 4]; return !(c >= det_t) && c > low_t; }, s.dlo, 0);
    int net = (n_pool > 0 && n_hi > 0) ? 1 : 0;
    if (net && (long long)n_pool * n_hi > d_cap) {      // the DHN object was sized for less: refuse, loudly (the back program returns no rows)
        if (ex.tid == 0) h->status |= Y7T_ERR_DHN_CAP;
        net = 0;
    }
    if (net) {
        y7t_gather_track_tlbr(ex, s, s.pool, n_pool);
        y7t_gather_det_tlbr(ex, s, s.dhi, n_hi);
        y7t_sync(ex);
        const double norm = y7t_dm_norm_factor(img_h, img_w);
        const int kf = cfg.kf;
        const long long tot = (long long)n_pool * n_hi;
        for (long long e = ex.tid; e < tot; e += ex.nt) {
            const int i = (int)(e / n_hi), j = (int)(e - (long long)i * n_hi);
            const int sl = s.pool[i];
            double t[4];
            y7t_track_tlwh(kf, s.mean + 8 * (size_t)sl, s.f32m[sl], t);
            const double iou_d = y7t_iou_dist(s.ttlbr + 4 * (size_t)i, s.dtlbr + 4 * (size_t)j);
            D[e] = (float)y7t_dm_ecu_iou(t, s.dbox + 4 * (size_t)s.dhi[j], iou_d, norm);
        }
    }
    y7t_sync(ex);
    if (ex.tid == 0) {
        fr->magic = Y7T_DM_MAGIC; fr->n = n; fr->n_pool = n_pool; fr->n_hi = n_hi; fr->n_lo = n_lo; fr->n_unc = n_unc; fr->net = net; fr->pad = 0;
        if (hw && net) { hw[0] = n_pool; hw[1] = n_hi; }
    }
    y7t_sync(ex);
}

// matching.linear_assignment(1.0 - net_out, thresh) for the na x nb float32 network output -> xrow / ycol.  The network's costs are dense (every pair has one under 1),
// so this is the dense lapjv on the float64 casts, with StrongSORT's tie watch (y7t_assoc_ss): a saturated sigmoid repeats costs exactly, and which of the equal
// optima lapjv returns is a property of its own scan order -- such a problem goes to lapjv.cpp run literally.
Y7T_FN void y7t_assoc_dm(const Y7TExec& ex, const Y7TTrk& s, int na, int nb, double thresh, const float* net_out) {
    if (na == 0 || nb == 0) {
        for (int i = ex.tid; i < na; i += ex.nt) s.xrow[i] = -1;
        for (int j = ex.tid; j < nb; j += ex.nt) s.ycol[j] = -1;
        y7t_sync(ex);
        return;
    }
    Y7TLap L;
    L.nr = na; L.nc = nb; L.ld = nb; L.n = na + nb; L.half = thresh / 2.0;
    L.prof = nullptr;
    const size_t ws = y7t_al(y7t_lap_ws_bytes(L.n)), cb = (size_t)na * nb * sizeof(double);
    void* lapws = s.lapws;
    double* cost = s.cost;
    size_t off = 0;
    if (ex.fast && ws <= ex.fast_bytes) { lapws = ex.fast; off = ws; }
    if (ex.fast && off + cb <= ex.fast_bytes) cost = (double*)(ex.fast + off);
    for (long long e = ex.tid; e < (long long)na * nb; e += ex.nt) { const float c = 1.0f - net_out[e]; cost[e] = (double)c; }
    y7t_sync(ex);
    int* flag = s.xrow;      // (written below)
    if (ex.tid == 0) flag[0] = 0;
    y7t_sync(ex);
    for (int k = ex.tid; k < na + nb; k += ex.nt) {
        const bool row = k < na;
        const int cnt = row ? nb : na;
        const double* p = row ? cost + (size_t)k * nb : cost + (k - na);
        const size_t st = row ? 1 : (size_t)nb;
        bool dup = false;
        for (int a = 1; a < cnt && !dup; ++a) {
            const double c = p[a * st];
            if (!(c <= thresh)) continue;
            for (int b = 0; b < a; ++b) dup |= y7t_near(p[b * st], c);
        }
        if (dup) { flag[0] = 1; Y7T_TIE_REASON(6); }
    }
    y7t_sync(ex);
    const bool tied = flag[0] != 0;
    y7t_sync(ex);
    L.c = cost;
    y7t_lap_bind(L, lapws, L.n);
    if (tied || y7t_lap_solve_sap(ex, L)) y7t_lap_solve_literal(ex, L);
    for (int i = ex.tid; i < na; i += ex.nt) s.xrow[i] = (L.x[i] >= nb) ? -1 : L.x[i];
    for (int j = ex.tid; j < nb; j += ex.nt) s.ycol[j] = (L.y[j] >= na) ? -1 : L.y[j];
    y7t_sync(ex);
}

// ---- back: deepmot.py:233-324.  net_out: the network's output for the front program's matrix (read when the frame ran it); net_status: the forward's status word ----
Y7T_FN void y7t_deepmot_back(const Y7TExec& ex, void* blob, const float* dets, const float* net_out, const unsigned* net_status, double* out_rows, int out_cap, int* out_count) {
    Y7TTrkHdr* h = (Y7TTrkHdr*)blob;
    const Y7TTrkCfg cfg = h->cfg;
    if (y7t_dm_refuse(ex, h, out_count)) return;
    const Y7TTrk s = y7t_trk_bind(blob, cfg.cap_t, cfg.cap_d);
    const Y7TDmFrame fr = *(const Y7TDmFrame*)s.cost;
    y7t_sync(ex);
    const bool net_failed = fr.net && net_status && *net_status != 0u;
    if (fr.magic != Y7T_DM_MAGIC || (h->status & Y7T_ERR_DHN_CAP) || net_failed) {      // no front program ran / no network output: the frame produces no rows
        if (ex.tid == 0) { if (net_failed) h->status |= Y7T_ERR_DHN; else if (fr.magic != Y7T_DM_MAGIC) h->status |= Y7T_ERR_KIND; if (out_count) *out_count = 0; }
        return;
    }
    if (ex.tid == 0) ((Y7TDmFrame*)s.cost)->magic = 0;      // (a frame's counts serve one back program)
    y7t_sync(ex);
    const int kf = cfg.kf, frame_id = h->frame_id, nl0 = h->n_lost;
    const int n_pool = fr.n_pool, n_hi = fr.n_hi, n_lo = fr.n_lo, n_unc = fr.n_unc;
    const float new_gate = (float)(cfg.det_thresh + 0.1);
    int na, nr;
    // ---- Step 2: strack_pool x D_high, 1 - DHN at 0.9 (Tracked -> update, Lost -> re_activate); without the network the ecu matrix is empty: nothing matches ----
    if (fr.net) y7t_assoc_dm(ex, s, n_pool, n_hi, 0.9, net_out);
    else {
        for (int i = ex.tid; i < n_pool; i += ex.nt) s.xrow[i] = -1;
        for (int j = ex.tid; j < n_hi; j += ex.nt) s.ycol[j] = -1;
        y7t_sync(ex);
    }
    y7t_apply_matches(ex, s, s.pool, n_pool, s.dhi, dets, 0, na, nr);
    // u_dets0, in detection order
    const int n_left = y7t_compact(ex, n_hi, [&](int j) { return s.ycol[j] < 0; }, s.tmpa, 0);
    for (int k = ex.tid; k < n_left; k += ex.nt) s.left[k] = s.dhi[s.tmpa[k]];
    y7t_sync(ex);
    // ---- Step 3: the still-Tracked leftovers (u_tracks0) x D_low, IoU at 0.5 ----
    const int n_rem = y7t_compact(ex, n_pool, [&](int i) { return s.xrow[i] < 0 && s.state[s.pool[i]] == Y7T_TRACKED; }, s.tmpa, 0);
    for (int k = ex.tid; k < n_rem; k += ex.nt) s.rem[k] = s.pool[s.tmpa[k]];
    y7t_sync(ex);
    y7t_gather_track_tlbr(ex, s, s.rem, n_rem);
    y7t_gather_det_tlbr(ex, s, s.dlo, n_lo);
    y7t_sync(ex);
    y7t_assoc(ex, s, n_rem, n_lo, 0.5);
    y7t_apply_matches(ex, s, s.rem, n_rem, s.dlo, dets, 0, na, nr);
    // ---- Step 4: `for idx in u_tracks1_idx: track = strack_pool[idx]` (sic, deepmot.py:269-272): the unmatched ROW NUMBERS of u_tracks0 index the pool ----
    {
        const int nl_new = y7t_compact(ex, n_rem, [&](int r) { return s.xrow[r] < 0; }, s.tmpa, 0);
        for (int k = ex.tid; k < nl_new; k += ex.nt) { const int sl = s.pool[s.tmpa[k]]; s.lostn[k] = sl; s.state[sl] = Y7T_LOST; }
        if (ex.tid == 0) h->n_lostn_last = nl_new;
        y7t_sync(ex);
    }
    // unconfirmed tracks x u_dets0, IoU at 0.7: update only, the rest removed
    y7t_gather_track_tlbr(ex, s, s.unconf, n_unc);
    y7t_gather_det_tlbr(ex, s, s.left, n_left);
    y7t_sync(ex);
    y7t_assoc(ex, s, n_unc, n_left, 0.7);
    y7t_apply_matches(ex, s, s.unconf, n_unc, s.left, dets, 2, na, nr);
    {
        const int n_rm = y7t_compact(ex, n_unc, [&](int i) { return s.xrow[i] < 0; }, s.tmpa, 0);
        for (int k = ex.tid; k < n_rm; k += ex.nt) { const int sl = s.unconf[s.tmpa[k]]; s.removedl[k] = sl; s.state[sl] = Y7T_REMOVED; }
        if (ex.tid == 0) h->n_removed_last = n_rm;
        y7t_sync(ex);
    }
    // new tracks from u_det2 with score > det_thresh + 0.1 (deepmot.py:293-297; ids in order)
    {
        const int n_new = y7t_compact(ex, n_left, [&](int j) { return s.ycol[j] < 0 && dets[6 * (size_t)s.left[j] + 4] > new_gate; }, s.tmpa, 0);
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
    }
    // age out long-lost tracks (deepmot.py:300-303)
    {
        const int n_old = y7t_compact(ex, nl0, [&](int i) { return frame_id - s.frame[s.lost[i]] > cfg.max_time_lost; }, s.tmpa, 0);
        const int base = h->n_removed_last;
        for (int k = ex.tid; k < n_old; k += ex.nt) { const int sl = s.lost[s.tmpa[k]]; s.removedl[base + k] = sl; s.state[sl] = Y7T_REMOVED; }
        y7t_sync(ex);
        if (ex.tid == 0) h->n_removed_last = base + n_old;
        y7t_sync(ex);
    }
    y7t_finish(ex, s, out_rows, out_cap, out_count);
}
