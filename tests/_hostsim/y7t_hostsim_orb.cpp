// tests/_hostsim/y7t_hostsim_orb.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of the feature-estimator bodies of yolov7-tracker_amd/csrc/y7t_orb.h: every per-pixel, per-keypoint, per-match and per-hypothesis program of
// csrc/y7t_orb.hip run one item at a time, into the SAME workspace and state layout (y7t_orb_layout), so that every intermediate array can be compared with the
// device's and with the NumPy restatement.  All cross-item sums are integers, so no reduction order needs mirroring.  The product package never loads this library.
#include <string.h>
#include <vector>
#include "../../yolov7-tracker_amd/csrc/y7t_orb.h"

// hypotheses, selection, refinement over a list of good matches (csrc/y7t_orb.hip: k_orb_hyp, k_orb_select); e->flag must be Y7T_ORB_OK on entry
static bool hs_ransac(const Y7TOrbPair* good, int ds, Y7TOrbEst* e, int* counts, double* warp6) {
    const int n = e->n_good;
    for (int k = 0; k < Y7T_ORB_NHYP; ++k) {
        Y7TOrbModel m;
        int cnt = 0;
        if (y7t_orb_model(good[y7t_orb_pick(k, 0, n)], good[y7t_orb_pick(k, 1, n)], &m))
            for (int t = 0; t < n; ++t) cnt += y7t_orb_inlier(m, good[t]) ? 1 : 0;
        counts[k] = cnt;
    }
    int bc = -1, bk = Y7T_ORB_NHYP;
    for (int k = 0; k < Y7T_ORB_NHYP; ++k)
        if (counts[k] > bc) { bc = counts[k]; bk = k; }
    e->winner = bk; e->n_inliers = bc;
    bool have = false;
    if (bc >= 2) {
        Y7TOrbModel m;
        y7t_orb_model(good[y7t_orb_pick(bk, 0, n)], good[y7t_orb_pick(bk, 1, n)], &m);
        long long a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int t = 0; t < n; ++t) {
            const Y7TOrbPair g = good[t];
            if (!y7t_orb_inlier(m, g)) continue;
            const long long x = g.px, y = g.py, u = g.cx, v = g.cy;
            a[0] += x; a[1] += y; a[2] += u; a[3] += v; a[4] += x * x + y * y; a[5] += x * u + y * v; a[6] += x * v - y * u; a[7] += 1;
        }
        have = y7t_orb_refine(a[7], a, ds, warp6);
    }
    if (!have) e->flag = Y7T_ORB_NO_MODEL;
    return have;
}

extern "C" {
void hs_orb_layout(int h, int w, int cap, size_t* off12) { y7t_orb_layout(h, w, cap, off12); }
size_t hs_orb_state_bytes(int cap) { return y7t_orb_state_size(cap); }

void hs_orb_extract(const uint8_t* bgr, int H, int W, int ds, const float* dets, int n_dets, int cap, void* workspace, void* state) {
    const int h = H / ds, w = W / ds;
    size_t off[Y7T_ORB_NTAP];
    y7t_orb_layout(h, w, cap, off);
    char* ws = (char*)workspace;
    uint8_t *plane = (uint8_t*)(ws + off[0]), *scores = (uint8_t*)(ws + off[1]), *keep = (uint8_t*)(ws + off[2]), *smooth = (uint8_t*)(ws + off[3]);
    int *rowcnt = (int*)(ws + off[4]), *rowoff = (int*)(ws + off[5]), *moments = (int*)(ws + off[6]);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) plane[(size_t)y * w + x] = y7t_orb_plane_px(bgr, H, W, ds, h, w, y, x);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const bool inside = x >= 3 && x < w - 3 && y >= 3 && y < h - 3;
            scores[(size_t)y * w + x] = inside ? (uint8_t)y7t_orb_fast_score(plane + (size_t)y * w + x, w) : (uint8_t)0;
        }
    int total = 0;
    Y7TOrbKp* kps = y7t_orb_kps(state, cap);
    for (int y = 0; y < h; ++y) {
        rowoff[y] = total;
        int cnt = 0;
        for (int x = 0; x < w; ++x) {
            bool k = false;
            if (y >= 1 && y < h - 1 && x >= 1 && x < w - 1) k = y7t_orb_is_max(scores + (size_t)y * w + x, w) && y7t_orb_unmasked(dets, n_dets, ds, h, w, x, y);
            keep[(size_t)y * w + x] = k ? 1 : 0;
            if (k) {
                if (total + cnt < cap) { kps[total + cnt].x = x; kps[total + cnt].y = y; }
                ++cnt;
            }
        }
        rowcnt[y] = cnt;
        total += cnt;
    }
    Y7TOrbHdr* hdr = (Y7TOrbHdr*)state;
    memset(hdr, 0, sizeof(*hdr));
    hdr->n = total < cap ? total : cap; hdr->total = total; hdr->truncated = total > cap ? 1 : 0; hdr->h = h; hdr->w = w;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) smooth[(size_t)y * w + x] = y7t_orb_smooth_px(plane, h, w, y, x);
    unsigned long long* desc = y7t_orb_desc(state);
    for (int i = 0; i < hdr->n; ++i) {
        const uint8_t* c = plane + (size_t)kps[i].y * w + kps[i].x;
        int m10 = 0, m01 = 0;
        for (int idx = 0; idx < 961; ++idx) y7t_orb_moment_term(c, w, idx, &m10, &m01);
        moments[2 * i] = m10; moments[2 * i + 1] = m01;
        double co, si;
        y7t_orb_direction(m10, m01, &co, &si);
        const uint8_t* cs = smooth + (size_t)kps[i].y * w + kps[i].x;
        for (int r = 0; r < 4; ++r) {
            unsigned long long m = 0;
            for (int l = 0; l < 64; ++l) m |= (unsigned long long)y7t_orb_bit(cs, w, r * 64 + l, co, si) << l;
            desc[(size_t)i * 4 + r] = m;
        }
    }
}

void hs_orb_estimate(const void* prev, const void* cur, int h, int w, int ds, int cap, void* workspace, double* warp6, double* status6) {
    size_t off[Y7T_ORB_NTAP];
    y7t_orb_layout(h, w, cap, off);
    char* ws = (char*)workspace;
    Y7TOrbMatch* matches = (Y7TOrbMatch*)(ws + off[7]);
    Y7TOrbPair* good = (Y7TOrbPair*)(ws + off[8]);
    Y7TOrbEst* est = (Y7TOrbEst*)(ws + off[9]);
    int* counts = (int*)(ws + off[10]);
    const Y7TOrbHdr *ph = (const Y7TOrbHdr*)prev, *ch = (const Y7TOrbHdr*)cur;
    const int n_prev = ph->n, n_cur = ch->n, trunc = ch->truncated | ph->truncated << 1;
    Y7TOrbEst e;
    memset(&e, 0, sizeof(e));
    e.flag = Y7T_ORB_NO_MATCHES; e.winner = -1;
    bool have = false;
    if (n_prev > 0 && n_cur >= 2) {
        const unsigned long long *pd = y7t_orb_desc((void*)prev), *cd = y7t_orb_desc((void*)cur);
        const Y7TOrbKp *pk = y7t_orb_kps((void*)prev, cap), *ck = y7t_orb_kps((void*)cur, cap);
        long long a[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < n_prev; ++i) {
            Y7TOrbMatch m;
            m.j1 = -1; m.j2 = -1; m.d1 = 1 << 30; m.d2 = 1 << 30;
            for (int j = 0; j < n_cur; ++j) y7t_orb_best_two(&m, j, y7t_orb_hamming(pd + (size_t)i * 4, cd + (size_t)j * 4));
            matches[i] = m;
            const int dx = pk[i].x - ck[m.j1].x, dy = pk[i].y - ck[m.j1].y;
            if (y7t_orb_first_tests(m, dx, dy, ch->h, ch->w)) { a[0] += 1; a[1] += dx; a[2] += (long long)dx * dx; a[3] += dy; a[4] += (long long)dy * dy; }
        }
        e.flag = Y7T_ORB_NOT_ENOUGH;
        if (a[0] > 0) {
            double mx, sx, my, sy;
            y7t_orb_mean_std(a[0], a[1], a[2], &mx, &sx);
            y7t_orb_mean_std(a[0], a[3], a[4], &my, &sy);
            int run = 0;
            for (int i = 0; i < n_prev; ++i) {
                const Y7TOrbMatch m = matches[i];
                Y7TOrbPair p;
                p.px = pk[i].x; p.py = pk[i].y; p.cx = ck[m.j1].x; p.cy = ck[m.j1].y;
                const int dx = p.px - p.cx, dy = p.py - p.cy;
                if (y7t_orb_first_tests(m, dx, dy, ch->h, ch->w) && y7t_orb_one_sided(dx, mx, sx) && y7t_orb_one_sided(dy, my, sy)) good[run++] = p;
            }
            e.n_good = run; e.n_first = (int)a[0];
            if (run > 4) {
                e.flag = Y7T_ORB_OK;
                have = hs_ransac(good, ds, &e, counts, warp6);
            }
        }
    }
    *est = e;
    y7t_orb_finish(n_prev, n_cur, trunc, &e, have, warp6, status6);
}

// the RANSAC and the refinement alone over a given list of matches {px, py, cx, cy}: est5 = {good, flag, 0, winner, inliers}
void hs_orb_ransac(const int* good4, int n, int ds, int* counts2000, int* est5, double* warp6) {
    Y7TOrbEst e;
    memset(&e, 0, sizeof(e));
    e.n_good = n; e.flag = Y7T_ORB_OK; e.winner = -1;
    const bool have = hs_ransac((const Y7TOrbPair*)good4, ds, &e, counts2000, warp6);
    double st[6];
    y7t_orb_finish(0, 0, 0, &e, have, warp6, st);
    est5[0] = e.n_good; est5[1] = e.flag; est5[2] = e.n_first; est5[3] = e.winner; est5[4] = e.n_inliers;
}
int hs_orb_pick(int k, int c, int n) { return y7t_orb_pick(k, c, n); }
}
