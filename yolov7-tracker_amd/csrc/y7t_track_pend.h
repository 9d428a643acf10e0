// y7t_track_pend.h -- what the appearance trackers' feature states share (DeepSORT, StrongSORT, BoT-SORT with ReID: y7t_track_*.h): the words every state's header
// begins with and the queue of appearance vectors a frame's step decides to store (written out by a launch of its own after the step).  Portable text, as they are.
#pragma once
#include "y7t_track_step.h"

// The first seven words of every feature state (caller-owned device memory next to the track-pool blob): each tracker's header DERIVES from this one and names its own
// words behind them, so the queue below runs on any of them as the Y7TPendHdr it is.  The host reads `status` by its byte offset (tracker/appearance.py).  budget: vectors
// kept per track -- DeepSORT's ring depth, 1 for the one-vector stores.  (offsetof may not be asked of a derived header, no standard-layout type: its sizeof is asserted,
// and where that is these 28 bytes plus the sizes of its own words there is no padding -- every word is where the sum puts it.)
struct Y7TPendHdr { int magic, dim, budget, cap_t, cap_d, status, n_pend; };
static_assert(sizeof(Y7TPendHdr) == 28 && offsetof(Y7TPendHdr, status) == 20 && offsetof(Y7TPendHdr, n_pend) == 24, "the feature states' shared header words");
// status bits every feature state shares (a tracker's own bits: its header)
enum { Y7T_PEND_ERR_CAP = 2 /* the feature state is smaller than the pool it is stepped with */, Y7T_PEND_ERR_FULL = 16 /* more queued vectors than the queue holds */ };

// the queue: n_pend entries (slot, detection row, 1 = update / 0 = new track) in pend[PPD * cap_d][3], PPD = entries per detection of the capacity
struct Y7TPend { Y7TPendHdr* h; int* pend; };
// ... of a bound feature state f (Y7TFeat, Y7TSs: f.h points to a header derived from Y7TPendHdr, f.pend is its queue)
template <class F> Y7T_FN Y7TPend y7t_pend_of(const F& f) { return Y7TPend{f.h, f.pend}; }
template <int PPD>
Y7T_FN int y7t_pend_cap(const Y7TPend& q) {
    if constexpr (PPD == 1) return q.h->cap_d;
    else return PPD * q.h->cap_d;
}
template <int PPD>
Y7T_FN int y7t_pend_count(const Y7TPend& q) { return q.h->n_pend < y7t_pend_cap<PPD>(q) ? q.h->n_pend : y7t_pend_cap<PPD>(q); }

// Queue the vectors a step decides to store; the store launch writes them after the step (nothing in the step reads the stored vectors: this frame's distances were
// taken before it).  A detection row is stored at most once per association and a slot receives at most one vector.  The step zeroes n_pend when it begins.
template <int PPD = 1, class PairFn>
Y7T_FN void y7t_pend_queue(const Y7TExec& ex, const Y7TPend& q, int count, int update, PairFn pair /* (i, slot&, detection row&) -> bool */) {
    for (int i = ex.tid; i < count; i += ex.nt) {
        int sl, row;
        if (!pair(i, sl, row)) continue;
        const int k = Y7T_FETCH_ADD(&q.h->n_pend, 1);
        if (k < y7t_pend_cap<PPD>(q)) { q.pend[3 * k] = sl; q.pend[3 * k + 1] = row; q.pend[3 * k + 2] = update; }
        else q.h->status |= Y7T_PEND_ERR_FULL;
    }
    y7t_sync(ex);
}
// ... for the rows of `tracks` that apply_matches UPDATED (tmpa[i] == 1: STrack.update, basetrack.py:324-332; re_activate keeps what the track has)
template <int PPD = 1>
Y7T_FN void y7t_pend_queue_updates(const Y7TExec& ex, const Y7TTrk& s, const Y7TPend& q, const int* tracks, int na, const int* dets) {
    y7t_pend_queue<PPD>(ex, q, na, 1, [&](int i, int& sl, int& row) {
        if (s.xrow[i] < 0 || s.tmpa[i] != 1) return false;
        sl = tracks[i];
        row = dets[s.xrow[i]];
        return true;
    });
}
