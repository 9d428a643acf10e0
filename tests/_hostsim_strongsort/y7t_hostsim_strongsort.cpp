// tests/_hostsim_strongsort/y7t_hostsim_strongsort.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build (one "thread", nt = 1) of tests/_hostsim plus the StrongSORT workgroup program of yolov7-tracker_amd/csrc/y7t_track_strongsort.h:
// the plain forms of the frame's three launches (appearance distances, the step, the queued vector stores).  The product package never loads this library.
static int g_ss_stat[4] = {0};      // fused associations solved by the sparse component solver / densely after it declined / densely after a tie / densely (small problems)
#define Y7T_SS_STAT(k) (++g_ss_stat[k])
#include "../_hostsim/y7t_hostsim.cpp"
#include "../../yolov7-tracker_amd/csrc/y7t_track_strongsort.h"

extern "C" {
size_t hs_ss_feat_bytes(int cap_t, int cap_d, int dim) { return y7t_ss_layout(cap_t, cap_d, dim).total; }
void hs_ss_feat_init(void* fblob, int cap_t, int cap_d, int dim, double gamma) { y7t_ss_init(hs_ex(), fblob, cap_t, cap_d, dim, gamma); }
int hs_strongsort_step(void* blob, void* fblob, const float* dets, int n, const float* feats, double* out_rows, int out_cap, const double* warp) {
    int cnt = 0;
    const Y7TExec ex = hs_ex();
    Y7TTrkHdr* h = (Y7TTrkHdr*)blob;
    const Y7TTrk s = y7t_trk_bind(blob, h->cfg.cap_t, h->cfg.cap_d);
    const Y7TSs f = y7t_ss_bind(fblob);
    y7t_ss_appearance_plain(ex, s, f, dets, feats, n);
    y7t_tracker_step_strongsort(ex, blob, fblob, dets, n, feats, out_rows, out_cap, &cnt, warp);
    y7t_ss_store_pending(ex, f, feats);
    return cnt;
}
int hs_strongsort_predict(void* blob, double* out_rows, int out_cap) {      // update_without_detection: the program's predict-only form, no feature state
    int cnt = 0;
    y7t_tracker_step_strongsort(hs_ex(), blob, nullptr, nullptr, -1, nullptr, out_rows, out_cap, &cnt, nullptr);
    return cnt;
}
int hs_ss_feat_status(void* fblob) { return ((Y7TSsHdr*)fblob)->status; }
int hs_ss_stat(int k) { return g_ss_stat[k]; }
// the slot's vector (STrack.features[-1]); the byte offset of the vectors for host-side views
size_t hs_ss_vec_offset(int cap_t, int cap_d, int dim) { return y7t_ss_layout(cap_t, cap_d, dim).vec; }
// the pieces on their own
void hs_ss_cdist(const float* u, int nu, const float* v, int nv, int dim, double* out) {
    for (int i = 0; i < nu; ++i) for (int j = 0; j < nv; ++j) out[(size_t)i * nv + j] = y7t_ss_dist(u + (size_t)i * dim, v + (size_t)j * dim, dim);
}
void hs_ss_ema(float* vec, const float* raw, int dim) { y7t_ss_ema(vec, raw, dim); }
double hs_ss_fuse(double gamma, double iou_d, double app_d) { return y7t_ss_fuse(gamma, iou_d, app_d); }
}
