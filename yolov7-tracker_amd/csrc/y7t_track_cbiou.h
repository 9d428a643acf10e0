// y7t_track_cbiou.h -- the C-BIoU tracker's frame step (reference tracker/c_biou_tracker.py: C_BIoUSTrack :17-209, C_BIoUTracker.update
// :218-353) as ONE workgroup program over the same struct-of-arrays pool as the Kalman trackers (y7t_track_step.h).  Portable text like the
// rest of the tracker programs; y7t_step_one (end of y7t_track_step.h) runs it for pools of kind Y7T_C_BIOU.
//
// C-BIoU has no motion model: a track is its last detection boxes and two "buffered" boxes, and the three associations compare buffered boxes
// by IoU.  Per slot (the slot's `cov` storage, 64 doubles that only a Kalman filter uses, so the state blob's layout is the same for every tracker):
//   cov[0, 24)   origin_bbox_buffer: up to 6 tlwh boxes, oldest first (the deque's `len > n -> popleft; append` rule with n = 5 lets it hold 6)
//   cov[24, 28)  motion_state1 (tlwh, buffer b1 = 0.3)        cov[28, 32)  motion_state2 (tlwh, buffer b2 = 0.5)
//   cov[32]      number of boxes in the buffer
//   cov[36, 40)  buffer_bbox1, cov[40, 44) buffer_bbox2: the buffered boxes of the box the track was activated / last re-activated with (update leaves them)
// box[] holds the last box (= the track's tlwh / tlbr, which nothing predicts forward); tsu[] is time_since_update, the δ of the paper.
//
// Float types follow the reference as it runs: the boxes are float32 (tlbr2tlwh of the float32 detection rows).  Under numpy >= 2 (NEP 50;
// cfg.f32_quirk = 1) the buffered boxes, the extrapolated motion state and the tlwh2tlbr sums are float32 too -- the Python floats b, 2*b and
// tsu/5 are rounded to float32 first.  Under numpy 1.x (f32_quirk = 0) `b * box[2]` of a float32 scalar is float64, so the buffered boxes and
// their tlbr are float64, while the extrapolated state (a float32 array times a Python float) stays float32.  The association's IoU is float64
// either way (matching.ious).
#pragma once
#include "y7t_track_step.h"

#define Y7T_CB_MS1 24
#define Y7T_CB_MS2 28
#define Y7T_CB_LEN 32
#define Y7T_CB_BB1 36
#define Y7T_CB_BB2 40

// get_buffer_bbox (c_biou_tracker.py:48-62) of a float32 tlwh: tlwh + [-b*w, -b*h, 2b*w, 2b*h], then np.maximum(0.0, .)
Y7T_FN void y7t_cb_buffer(const float* t, double b, int f32, double* o) {
    if (f32) {
        const float nb = (float)(-b), b2 = (float)(2.0 * b);
        const float r[4] = {t[0] + nb * t[2], t[1] + nb * t[3], t[2] + b2 * t[2], t[3] + b2 * t[3]};
        for (int k = 0; k < 4; ++k) o[k] = (0.0f >= r[k]) ? 0.0 : (double)r[k];
    } else {
        const double x = t[0], y = t[1], w = t[2], h = t[3];
        const double r[4] = {x + (-b) * w, y + (-b) * h, w + (2.0 * b) * w, h + (2.0 * b) * h};
        for (int k = 0; k < 4; ++k) o[k] = (0.0 >= r[k]) ? 0.0 : r[k];
    }
}

// tlwh2tlbr (c_biou_tracker.py:198-209) of a buffered box, in the box's dtype
Y7T_FN void y7t_cb_tlbr(const double* t, int f32, double* o) {
    o[0] = t[0]; o[1] = t[1];
    if (f32) { o[2] = (float)t[2] + (float)t[0]; o[3] = (float)t[3] + (float)t[1]; }
    else { o[2] = t[2] + t[0]; o[3] = t[3] + t[1]; }
}

// a new box for slot `sl`: append to the buffer (update :127-131 / re_activate :103-107), the last box, the motion states.
// upd: update (:133-146: extrapolate o^t + (δ/n)(o^t - o^{t-n}) when δ = tsu > 0 and the buffer holds at least n boxes); else re_activate (:109-112)
Y7T_FN void y7t_cb_take(const Y7TTrk& s, int sl, const float* box, bool upd, int f32) {
    double* c = s.cov + 64 * (size_t)sl;
    int len = (int)c[Y7T_CB_LEN];
    if (len > 5) {
        for (int k = 0; k < 20; ++k) c[k] = c[k + 4];
        len = 5;
    }
    for (int k = 0; k < 4; ++k) { c[4 * len + k] = box[k]; s.box[4 * (size_t)sl + k] = box[k]; }
    len += 1;
    c[Y7T_CB_LEN] = len;
    float ms[4] = {box[0], box[1], box[2], box[3]};
    const int tsu = s.tsu[sl];
    if (upd && tsu != 0 && len >= 5) {
        const float f = (float)((double)tsu / 5.0);
        for (int k = 0; k < 4; ++k) { const float last = (float)c[4 * (len - 1) + k], first = (float)c[k]; ms[k] = last + f * (last - first); }
    }
    y7t_cb_buffer(ms, 0.3, f32, c + Y7T_CB_MS1);
    y7t_cb_buffer(ms, 0.5, f32, c + Y7T_CB_MS2);
    if (!upd) for (int k = 0; k < 4; ++k) { c[Y7T_CB_BB1 + k] = c[Y7T_CB_MS1 + k]; c[Y7T_CB_BB2 + k] = c[Y7T_CB_MS2 + k]; }
}

// apply the matches of one association: a Tracked track is updated, a Lost one re-activated (which leaves time_since_update as it was:
// the next update of a re-found track extrapolates with that stale δ -- reference behaviour, kept)
Y7T_FN void y7t_cb_apply(const Y7TExec& ex, const Y7TTrk& s, const int* tracks, int na, const int* dets, const float* det_rows, int& n_act, int& n_refind) {
    const int frame_id = s.h->frame_id, f32 = s.h->cfg.f32_quirk;
    for (int i = ex.tid; i < na; i += ex.nt) {
        const int jd = s.xrow[i];
        if (jd < 0) continue;
        const int sl = tracks[i], dj = dets[jd];
        const int what = s.state[sl] == Y7T_TRACKED ? 1 : 2;
        s.tmpa[i] = what;
        y7t_cb_take(s, sl, s.dbox + 4 * (size_t)dj, what == 1, f32);
        s.frame[sl] = frame_id;
        s.score[sl] = det_rows[6 * (size_t)dj + 4];
        s.state[sl] = Y7T_TRACKED;
        s.act[sl] = 1;
        if (what == 1) { s.len[sl] += 1; s.tsu[sl] = 0; }
        else s.len[sl] = 0;
    }
    y7t_sync(ex);
    y7t_append_matches(ex, s, tracks, na, n_act, n_refind);
}

// the bookkeeping of the Kalman trackers with C_BIoUSTrack's geometry: tlwh / tlbr are the last box (float32)
Y7T_FN void y7t_cb_finish(const Y7TExec& ex, const Y7TTrk& s, double* out_rows, int out_cap, int* out_count) {
    y7t_finish_g(ex, s, out_rows, out_cap, out_count,
                 [&](int sl, double* o) {
                     const float* b = s.box + 4 * (size_t)sl;
                     o[0] = b[0]; o[1] = b[1]; o[2] = b[2] + b[0]; o[3] = b[3] + b[1];
                 },
                 [&](int sl, double* o) { const float* b = s.box + 4 * (size_t)sl; for (int k = 0; k < 4; ++k) o[k] = b[k]; });
}

// One C-BIoU frame.  dets: n x 6 float32 rows [x1, y1, x2, y2, conf, cls].  n < 0: update_without_detection, which the reference inherits from
// BaseTracker (basetrack.py:489-537) and which calls STrack.multi_predict -- C_BIoUSTrack has no Kalman mean, so it raises as soon as the pool
// holds a track: here Y7T_ERR_PREDICT and nothing changes; with an empty pool it only advances the frame.
Y7T_FN void y7t_tracker_step_cbiou_body(const Y7TExec& ex, void* blob, const float* dets, int n, double* out_rows, int out_cap, int* out_count) {
    Y7TTrkHdr* h = (Y7TTrkHdr*)blob;
    const Y7TTrkCfg cfg = h->cfg;
    const Y7TTrk s = y7t_trk_bind_ex(ex, blob, cfg.cap_t, cfg.cap_d);
    const int f32 = cfg.f32_quirk;
    y7t_sync(ex);
    Y7T_PROF(h, 0);
    const int nt0 = h->n_tracked, nl0 = h->n_lost;
    // unconfirmed / confirmed split of tracked (:250-256); strack_pool = joint_stracks(confirmed, lost) (:259): disjoint by construction
    const int n_unc = y7t_compact(ex, nt0, [&](int i) { return !s.act[s.tracked[i]]; }, s.tmpa, 0);
    for (int k = ex.tid; k < n_unc; k += ex.nt) s.unconf[k] = s.tracked[s.tmpa[k]];
    const int n_conf = y7t_compact(ex, nt0, [&](int i) { return s.act[s.tracked[i]] != 0; }, s.tmpb, 0);
    for (int k = ex.tid; k < n_conf; k += ex.nt) s.pool[k] = s.tracked[s.tmpb[k]];
    for (int k = ex.tid; k < nl0; k += ex.nt) s.pool[n_conf + k] = s.lost[k];
    y7t_sync(ex);
    const int n_pool = n_conf + nl0;
    if (n < 0 && n_pool > 0) {
        if (ex.tid == 0) { h->status |= Y7T_ERR_PREDICT; if (out_count) *out_count = 0; }
        return;
    }
    if (ex.tid == 0) {
        h->frame_id += 1;
        h->n_act_last = h->n_refind_last = h->n_lostn_last = h->n_removed_last = 0;
        if (n > cfg.cap_d) h->status |= Y7T_ERR_CAP_D;
    }
    y7t_sync(ex);
    if (n > cfg.cap_d) n = cfg.cap_d;
    const int frame_id = h->frame_id;
    Y7T_PROF(h, 1);
    if (n < 0) {
        y7t_cb_finish(ex, s, out_rows, out_cap, out_count);
        return;
    }
    // detections with conf > det_thresh (:238) -> C_BIoUSTrack(cls, tlbr2tlwh(tlbr), score): float32 tlwh
    for (int j = ex.tid; j < n; j += ex.nt) {
        const float* r = dets + 6 * (size_t)j;
        s.dbox[4 * (size_t)j + 0] = r[0];
        s.dbox[4 * (size_t)j + 1] = r[1];
        s.dbox[4 * (size_t)j + 2] = r[2] - r[0];
        s.dbox[4 * (size_t)j + 3] = r[3] - r[1];
    }
    y7t_sync(ex);
    const float det_t = (float)cfg.det_thresh, new_gate = (float)(cfg.det_thresh + 0.1);
    const int n_det = y7t_compact(ex, n, [&](int j) { return dets[6 * (size_t)j + 4] > det_t; }, s.dhi, 0);
    Y7T_PROF(h, 2);
    // ---- the three associations as ONE loop (one inlined copy of the solvers):
    //   0: pool vs every detection, level 1, 0.9 (:260-275)   1: the pool's still-Tracked leftovers vs the leftover detections, level 2, 0.5 (:278-298)
    //   2: unconfirmed tracks vs the detections left after level 2, level 1, 0.7 (:300-314)
    // left[] holds the detections left after association 0, dlo[] those left after association 1 ----
    int n_left = 0, n_left2 = 0, na, nr;
#if Y7T_DEVICE
#pragma clang loop unroll(disable)
#endif
    for (int ph = 0; ph < 3; ++ph) {
        const int* la; const int* ld;
        int nA, nD, ms;
        double th, b;
        if (ph == 0) { la = s.pool; nA = n_pool; ld = s.dhi; nD = n_det; ms = Y7T_CB_MS1; b = 0.3; th = 0.9; }
        else if (ph == 1) {
            const int n_rem = y7t_compact(ex, n_pool, [&](int i) { return s.xrow[i] < 0 && s.state[s.pool[i]] == Y7T_TRACKED; }, s.tmpa, 0);
            for (int k = ex.tid; k < n_rem; k += ex.nt) s.rem[k] = s.pool[s.tmpa[k]];
            y7t_sync(ex);
            la = s.rem; nA = n_rem; ld = s.left; nD = n_left; ms = Y7T_CB_MS2; b = 0.5; th = 0.5;
        } else { la = s.unconf; nA = n_unc; ld = s.dlo; nD = n_left2; ms = Y7T_CB_MS1; b = 0.3; th = 0.7; }
        // buffered_iou_distance (matching.py:391-407): the tracks' motion states against the detections' buffered boxes, both as tlbr
        for (int i = ex.tid; i < nA; i += ex.nt) y7t_cb_tlbr(s.cov + 64 * (size_t)la[i] + ms, f32, s.ttlbr + 4 * (size_t)i);
        for (int i = ex.tid; i < nD; i += ex.nt) {
            double bb[4];
            y7t_cb_buffer(s.dbox + 4 * (size_t)ld[i], b, f32, bb);
            y7t_cb_tlbr(bb, f32, s.dtlbr + 4 * (size_t)i);
        }
        y7t_sync(ex);
        const int stamp = ph == 0 ? 3 : ph == 1 ? 6 : 8;
        Y7T_PROF(h, stamp);
        y7t_assoc(ex, s, nA, nD, th);
        Y7T_PROF(h, stamp + 1);
        y7t_cb_apply(ex, s, la, nA, ld, dets, na, nr);
        if (ph == 0) {
            n_left = y7t_compact(ex, n_det, [&](int j) { return s.ycol[j] < 0; }, s.tmpa, 0);
            for (int k = ex.tid; k < n_left; k += ex.nt) s.left[k] = s.dhi[s.tmpa[k]];
            y7t_sync(ex);
        } else if (ph == 1) {
            // step 4 (:323-331): the unmatched tracks of association 1 are Lost with time_since_update = frame_id - end_frame, or Removed past max_time_lost
            const int nl_new = y7t_compact(ex, nA, [&](int i) { return s.xrow[i] < 0 && frame_id - s.frame[s.rem[i]] <= cfg.max_time_lost; }, s.tmpa, 0);
            for (int k = ex.tid; k < nl_new; k += ex.nt) {
                const int sl = s.rem[s.tmpa[k]];
                s.lostn[k] = sl; s.state[sl] = Y7T_LOST; s.tsu[sl] = frame_id - s.frame[sl];
            }
            y7t_sync(ex);
            const int n_old = y7t_compact(ex, nA, [&](int i) { return s.xrow[i] < 0 && frame_id - s.frame[s.rem[i]] > cfg.max_time_lost; }, s.tmpb, 0);
            for (int k = ex.tid; k < n_old; k += ex.nt) { const int sl = s.rem[s.tmpb[k]]; s.removedl[k] = sl; s.state[sl] = Y7T_REMOVED; }
            if (ex.tid == 0) { h->n_lostn_last = nl_new; h->n_removed_last = n_old; }
            y7t_sync(ex);
            n_left2 = y7t_compact(ex, n_left, [&](int j) { return s.ycol[j] < 0; }, s.tmpa, 0);
            for (int k = ex.tid; k < n_left2; k += ex.nt) s.dlo[k] = s.left[s.tmpa[k]];
            y7t_sync(ex);
        } else {
            const int n_rm = y7t_compact(ex, n_unc, [&](int i) { return s.xrow[i] < 0; }, s.tmpa, 0);
            const int base = h->n_removed_last;
            for (int k = ex.tid; k < n_rm; k += ex.nt) { const int sl = s.unconf[s.tmpa[k]]; s.removedl[base + k] = sl; s.state[sl] = Y7T_REMOVED; }
            y7t_sync(ex);
            if (ex.tid == 0) h->n_removed_last = base + n_rm;
            y7t_sync(ex);
        }
    }
    // ---- new tracks from the detections left after association 2 with score > det_thresh + 0.1 (:317-321; activate :76-87, ids in order) ----
    {
        const int n_new = y7t_compact(ex, n_left2, [&](int j) { return s.ycol[j] < 0 && dets[6 * (size_t)s.dlo[j] + 4] > new_gate; }, s.tmpa, 0);
        int* idc = (int*)(uintptr_t)h->id_counter_ptr;
        if (ex.tid == 0) {
            int nf = h->n_free;
            const int base = h->n_act_last, made = n_new < nf ? n_new : nf;
            if (n_new > nf) h->status |= Y7T_ERR_CAP_T;
            const int id0 = made > 0 ? Y7T_FETCH_ADD(idc, made) : 0;      // (one atomic add per frame: see y7t_tracker_step_body)
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
            const float* box = s.dbox + 4 * (size_t)dj;
            double* c = s.cov + 64 * (size_t)sl;
            for (int q = 0; q < 4; ++q) { s.box[4 * (size_t)sl + q] = box[q]; c[q] = box[q]; }
            c[Y7T_CB_LEN] = 1;
            y7t_cb_buffer(box, 0.3, f32, c + Y7T_CB_MS1);
            y7t_cb_buffer(box, 0.5, f32, c + Y7T_CB_MS2);
            for (int q = 0; q < 4; ++q) { c[Y7T_CB_BB1 + q] = c[Y7T_CB_MS1 + q]; c[Y7T_CB_BB2 + q] = c[Y7T_CB_MS2 + q]; }
            s.f32m[sl] = 0;
            s.score[sl] = dets[6 * (size_t)dj + 4];
            s.cls[sl] = dets[6 * (size_t)dj + 5];
            s.state[sl] = Y7T_TRACKED;
            s.act[sl] = (frame_id == 1) ? 1 : 0;
            s.frame[sl] = frame_id; s.start[sl] = frame_id;
            s.tsu[sl] = 0; s.len[sl] = 0; s.inrem[sl] = 0;
        }
        y7t_sync(ex);
    }
    // (no ageing of old lost tracks: the reference has none, its lost list grows with the sequence)
    Y7T_PROF(h, 10);
    y7t_cb_finish(ex, s, out_rows, out_cap, out_count);
    Y7T_PROF(h, 11);
}
