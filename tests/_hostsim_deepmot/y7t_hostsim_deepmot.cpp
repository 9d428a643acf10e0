// tests/_hostsim_deepmot/y7t_hostsim_deepmot.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build (one "thread", nt = 1) of tests/_hostsim plus DeepMOT's two workgroup programs of yolov7-tracker_amd/csrc/y7t_track_deepmot.h; the network
// between them is evaluated by the caller.  The product package never loads this library.
#include "../_hostsim/y7t_hostsim.cpp"
#include "../../yolov7-tracker_amd/csrc/y7t_track_deepmot.h"

extern "C" {
// -> rows << 16 | columns of the matrix the network is to run on (0: skipped); D holds it
int hs_deepmot_front(void* blob, const float* dets, int n, int img_h, int img_w, float* D, long long d_cap) {
    int hw[2] = {0, 0};
    y7t_deepmot_front(hs_ex(), blob, dets, n, img_h, img_w, D, d_cap, hw);
    return (hw[0] << 16) | hw[1];
}
int hs_deepmot_back(void* blob, const float* dets, const float* net_out, unsigned net_status, double* out_rows, int out_cap) {
    int cnt = 0;
    y7t_deepmot_back(hs_ex(), blob, dets, net_out, &net_status, out_rows, out_cap, &cnt);
    return cnt;
}
// one element of matching.ecu_iou_distance
double hs_dm_ecu_iou(const double* t_tlwh, const float* d_tlwh, double iou_d, int img_h, int img_w) { return y7t_dm_ecu_iou(t_tlwh, d_tlwh, iou_d, y7t_dm_norm_factor(img_h, img_w)); }
}
