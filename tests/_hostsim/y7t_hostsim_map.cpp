// tests/_hostsim/y7t_hostsim_map.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of yolov7-tracker_amd/csrc/y7t_map.h (-DY7T_HOSTSIM): the state blob of csrc/y7t_map.hip in host memory, y7t_map_image and y7t_map_curve -- the SAME
// bodies the device's workgroups run -- at nt = 1, and the radix sort as a serial pass per digit over the same keys and digits.  The product package never loads
// this library.
#include "../../yolov7-tracker_amd/csrc/y7t_map.h"
#include <string.h>
#include <vector>

extern "C" {
size_t hs_map_bytes(int cap, int nc) { return y7t_map_layout_of(cap, nc).total; }
void hs_map_layout(int cap, int nc, size_t* out4) {
    const Y7TMapLayout L = y7t_map_layout_of(cap, nc);
    out4[0] = L.nt; out4[1] = L.conf; out4[2] = L.cls; out4[3] = L.correct;
}
double hs_map_linspace01(int q, int n) { return y7t_map_linspace01(q, n); }
float hs_map_iou(const float* a, const float* b) { return y7t_map_iou(a, b); }
void hs_map_target_box(const float* t, float W, float H, const float* lb, float* b) { y7t_map_target_box(t, W, H, lb, b); }
void hs_map_scale_coords(float* b, const float* lb) { y7t_map_scale_coords(b, lb); }

void hs_map_init(char* obj, int cap, int nc) {
    const Y7TMapLayout L = y7t_map_layout_of(cap, nc);
    int* hdr = (int*)obj;
    memset(hdr, 0, 256);
    hdr[Y7T_MAP_H_CAP] = cap;
    hdr[Y7T_MAP_H_NC] = nc;
    memset(obj + L.nt, 0, (size_t)nc * 8);
    for (int q = 0; q < Y7T_MAP_GRID; ++q) ((double*)(obj + L.grid))[q] = y7t_map_linspace01(q, Y7T_MAP_GRID);
    for (int q = 0; q < Y7T_MAP_PX; ++q) ((double*)(obj + L.px))[q] = y7t_map_linspace01(q, Y7T_MAP_PX);
}

void hs_map_update(char* obj, const float* dets, const int* ndets, const int* keep, const float* cbox, int ncand, int cand_stride, int B, int max_det, const float* targets,
                   const int* toff, int img_h, int img_w, const float* lb, const float* iouv) {
    int* hdr = (int*)obj;
    const int cap = hdr[Y7T_MAP_H_CAP], nc = hdr[Y7T_MAP_H_NC];
    const Y7TMapLayout L = y7t_map_layout_of(cap, nc);
    long long total = 0;
    for (int b = 0; b < B; ++b) total += ndets[b] < 0 ? 0 : (ndets[b] > max_det ? max_det : ndets[b]);
    if (hdr[Y7T_MAP_H_ROWS] + total > cap) { hdr[Y7T_MAP_H_STATUS] |= Y7T_MAP_OVERFLOW; return; }
    std::vector<float> tb(Y7T_MAP_LANES * 4), tc(Y7T_MAP_LANES), pb((size_t)max_det * 4), bi(max_det);
    std::vector<int> bt(max_det);
    long long base = hdr[Y7T_MAP_H_ROWS];
    const Y7TMapExec ex = {0, 1};
    for (int b = 0; b < B; ++b) {
        const int P = ndets[b] < 0 ? 0 : (ndets[b] > max_det ? max_det : ndets[b]);
        if (P)
            y7t_map_image(ex, P, dets + (size_t)b * max_det * 6, keep + (size_t)b * max_det, cbox + (size_t)b * cand_stride * 4, ncand, targets + (size_t)toff[b] * 6,
                          toff[b + 1] - toff[b], (float)img_w, (float)img_h, lb + b * 5, iouv, tb.data(), tc.data(), pb.data(), bi.data(), bt.data(),
                          (float*)(obj + L.conf) + base, (int*)(obj + L.cls) + base, (int*)(obj + L.correct) + base);
        base += P;
    }
    long long* nt = (long long*)(obj + L.nt);
    for (int l = toff[0]; l < toff[B]; ++l)
        for (int c = 0; c < nc; ++c) nt[c] += targets[(size_t)l * 6 + 1] == (float)c ? 1 : 0;
    hdr[Y7T_MAP_H_ROWS] = (int)base;
    hdr[Y7T_MAP_H_SEEN] += B;
}

// -> ap (nc x 10), p, r (nc x 1000), nt (nc), classes (nc), info (4); order (rows): the sorted order as arrival indices, tpc (rows x 10): the inclusive counts
void hs_map_compute(char* obj, double* ap, double* p, double* r, long long* nt_out, int* classes, int* info, int* order, int* tpc) {
    int* hdr = (int*)obj;
    const int cap = hdr[Y7T_MAP_H_CAP], nc = hdr[Y7T_MAP_H_NC], n = hdr[Y7T_MAP_H_ROWS];
    const Y7TMapLayout L = y7t_map_layout_of(cap, nc);
    uint64_t *ka = (uint64_t*)(obj + L.key_a), *kb = (uint64_t*)(obj + L.key_b);
    uint32_t *ia = (uint32_t*)(obj + L.idx_a), *ib = (uint32_t*)(obj + L.idx_b);
    const float* conf = (const float*)(obj + L.conf);
    const int *cls = (const int*)(obj + L.cls), *cor = (const int*)(obj + L.correct);
    for (int i = 0; i < n; ++i) { ka[i] = y7t_map_key(cls[i], conf[i], nc); ia[i] = (uint32_t)i; }
    for (int pass = 0; pass < y7t_map_passes(nc); ++pass) {
        size_t cnt[257] = {0};
        for (int i = 0; i < n; ++i) ++cnt[y7t_map_digit(ka[i], pass) + 1];
        for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
        for (int i = 0; i < n; ++i) { const size_t o = cnt[y7t_map_digit(ka[i], pass)]++; kb[o] = ka[i]; ib[o] = ia[i]; }
        uint64_t* tk = ka; ka = kb; kb = tk;
        uint32_t* ti = ia; ia = ib; ib = ti;
    }
    float* sconf = (float*)(obj + L.sconf);
    int *scor = (int*)(obj + L.scorrect), *seg = (int*)(obj + L.seg);
    for (int i = 0; i < n; ++i) { sconf[i] = conf[ia[i]]; scor[i] = cor[ia[i]]; if (order) order[i] = (int)ia[i]; }
    for (int c = 0; c <= nc; ++c) {
        int lo = 0;
        while (lo < n && ka[lo] < ((uint64_t)c << 32)) ++lo;
        seg[c] = lo;
    }
    if (tpc)
        for (int c = 0; c < nc; ++c)
            for (int k = 0; k < Y7T_MAP_NIOU; ++k) {
                int run = 0;
                for (int i = seg[c]; i < seg[c + 1]; ++i) { run += (scor[i] >> k) & 1; tpc[(size_t)i * Y7T_MAP_NIOU + k] = run; }
            }
    const long long* nt = (const long long*)(obj + L.nt);
    std::vector<int> part(Y7T_MAP_LANES + 1);
    std::vector<double> pmax(Y7T_MAP_LANES), y(Y7T_MAP_GRID);
    const Y7TMapExec ex = {0, 1};
    int m = 0;
    for (int c = 0; c < nc; ++c) {
        for (int k = 0; k < Y7T_MAP_NIOU; ++k)
            y7t_map_curve(ex, sconf, scor, seg[c], seg[c + 1] - seg[c], nt[c], k, (const double*)(obj + L.grid), (const double*)(obj + L.px), part.data(), pmax.data(), y.data(),
                          ap + (size_t)c * Y7T_MAP_NIOU + k, p + (size_t)c * Y7T_MAP_PX, r + (size_t)c * Y7T_MAP_PX);
        nt_out[c] = nt[c];
        classes[c] = -1;
    }
    for (int c = 0; c < nc; ++c)
        if (nt[c] > 0) classes[m++] = c;
    info[0] = n; info[1] = hdr[Y7T_MAP_H_SEEN]; info[2] = hdr[Y7T_MAP_H_STATUS]; info[3] = m;
}
}
