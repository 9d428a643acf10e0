// tests/_hostsim/y7t_hostsim_jpegdec.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of yolov7-tracker_amd/csrc/y7t_jpegdec.h: one file through the launches of y7t_jpegdec_decode, a launch a loop over its workgroups and a workgroup a
// loop over its lanes, with the SAME lane, table, DC, block and pixel functions and the same memory layout.  What a barrier separates on the device is a loop of its
// own here (every lane reads its predecessor's exit before any lane of that round writes one).  The product package never loads this library.
#include "../../yolov7-tracker_amd/csrc/y7t_jpegdec.h"
#include <stddef.h>
#include <vector>

namespace {
struct Tables { Y7TJdHuff dc[3], ac[3]; };
void build_tables(const Y7TJdBytes& file, const Y7TJdDesc& d, const Y7TJdGeom& g, Tables* t) {
    for (int c = 0; c < g.comps; ++c) {
        y7t_jd_build_huff(file, d.dc_off[d.td[c] & 3], &t->dc[c]);
        y7t_jd_build_huff(file, d.ac_off[d.ta[c] & 3], &t->ac[c]);
    }
}
struct PlaneY { const unsigned char* p; int w; int operator()(int x, int y) const { return p[(size_t)y * w + x]; } };
struct PlaneC { const unsigned char* p[3]; int w; int operator()(int c, int x, int y) const { return p[c][(size_t)y * w + x]; } };
struct QTab { const Y7TJdBytes* file; uint32_t off; unsigned operator()(int k) const { return off ? (*file)(off + (uint32_t)k) : 1u; } };
}

extern "C" {
int hs_jpegdec_desc_bytes() { return (int)sizeof(Y7TJdDesc); }
int hs_jpegdec_subseq_min() { return Y7T_JD_SUBSEQ_MIN; }
int hs_jpegdec_nblocks(int H, int W, int sampling) { return y7t_jd_geom(H, W, sampling).nblocks; }
size_t hs_jpegdec_bytes(int H, int W, int sampling, size_t max_file_bytes, int subseq_bytes, int lanes) {
    Y7TJdLayout L;
    return y7t_jd_layout(y7t_jd_geom(H, W, sampling), 1, max_file_bytes, subseq_bytes, lanes, &L) ? L.total : 0;
}
// the offsets of the object's arrays (rounds, iters, descs, entry, exit, count, first, run_exit, run_entry, run_round, run_iters, coef, total): for a test that looks into a device object
int hs_jpegdec_layout(int H, int W, int sampling, size_t max_file_bytes, int subseq_bytes, int lanes, size_t* out) {
    Y7TJdLayout L;
    if (!y7t_jd_layout(y7t_jd_geom(H, W, sampling), 1, max_file_bytes, subseq_bytes, lanes, &L)) return -1;
    const size_t v[13] = {L.rounds, L.iters, L.descs, L.entry, L.exit, L.count, L.first, L.run_exit, L.run_entry, L.run_round, L.run_iters, L.coef, L.total};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
    return 0;
}

// file: the file's bytes (d->file_off is not used: the file starts at `file`); ws: hs_jpegdec_bytes(.., d->file_len, ..) bytes; diff / coef: nblocks x 64 int16 (or
// null) <- the coefficients with the DC as differences / as values; frame: H x W x 3; info: status, launches that found work, most rounds inside a workgroup,
// launches made, subsequences.  -> 0, or -1 for arguments the C ABI would refuse
int hs_jpegdec_decode(const unsigned char* file_bytes, const Y7TJdDesc* dp, int H, int W, int sampling, int subseq_bytes, int lanes, unsigned char* ws,
                      short* diff_out, short* coef_out, unsigned char* frame, int* info) {
    const Y7TJdDesc d = *dp;
    const Y7TJdGeom g = y7t_jd_geom(H, W, sampling);
    Y7TJdLayout L;
    if (!y7t_jd_layout(g, 1, d.file_len, subseq_bytes, lanes, &L)) return -1;
    if ((size_t)d.scan_off + d.scan_len > d.file_len) return -1;
    const Y7TJdBytes file = {file_bytes, d.file_len};
    const Y7TJdBytes scan = {file_bytes + d.scan_off, d.scan_len};
    const uint32_t S = (uint32_t)subseq_bytes, R = (uint32_t)lanes;
    const uint32_t nsub = (d.scan_len + S - 1) / S, nruns = (nsub + R - 1) / R;
    y7t_jd_state* entry = (y7t_jd_state*)(ws + L.entry);
    y7t_jd_state* exit_ = (y7t_jd_state*)(ws + L.exit);
    int* count = (int*)(ws + L.count);
    int* first = (int*)(ws + L.first);
    y7t_jd_state* run_exit = (y7t_jd_state*)(ws + L.run_exit);      // [2][L.nruns]
    y7t_jd_state* run_entry = (y7t_jd_state*)(ws + L.run_entry);
    int* run_round = (int*)(ws + L.run_round);
    int* run_iters = (int*)(ws + L.run_iters);
    short* coef = (short*)(ws + L.coef);
    Tables tab;
    build_tables(file, d, g, &tab);

    // ---- k_jd_sync, launch r = 0 .. nruns - 1 ----
    std::vector<y7t_jd_state> ex(R), want(R);
    for (uint32_t r = 0; r < nruns; ++r)
        for (uint32_t gi = 0; gi < nruns; ++gi) {
            const y7t_jd_state* prev = run_exit + ((r + 1) & 1) * L.nruns;
            y7t_jd_state* cur = run_exit + (r & 1) * L.nruns;
            const y7t_jd_state e = gi == 0 ? y7t_jd_pack(0, 0, 0) : (r == 0 ? y7t_jd_assumed(gi * R, S) : prev[gi - 1]);
            if (r > 0 && e == run_entry[gi]) { cur[gi] = prev[gi]; continue; }
            const uint32_t s0 = gi * R, n = nsub - s0 < R ? nsub - s0 : R;
            int iters = 0;
            for (;;) {
                bool any = false;
                for (uint32_t t = 0; t < n; ++t) {
                    if (iters == 0) want[t] = t == 0 ? e : (r == 0 ? y7t_jd_assumed(s0 + t, S) : entry[s0 + t]);
                    else want[t] = t == 0 ? e : ex[t - 1];
                }
                for (uint32_t t = 0; t < n; ++t) {
                    const bool fresh = iters == 0 && (r == 0 || (t == 0));
                    if (iters == 0 && !fresh) { ex[t] = exit_[s0 + t]; continue; }
                    if (!fresh && want[t] == entry[s0 + t]) continue;
                    int cnt, fl;
                    entry[s0 + t] = want[t];
                    ex[t] = y7t_jd_lane(scan, d.scan_len, g, tab.dc, tab.ac, d.restart_interval, want[t], 8u * (s0 + t + 1) * S, nullptr, 0, &cnt, &fl);
                    count[s0 + t] = cnt | fl << 24;
                    any = true;
                }
                ++iters;
                if (!any) break;
            }
            for (uint32_t t = 0; t < n; ++t) exit_[s0 + t] = ex[t];
            run_entry[gi] = e; cur[gi] = ex[n - 1]; run_round[gi] = (int)r; run_iters[gi] = iters;
        }

    // ---- k_jd_scan ----
    int total = 0, flags = 0, rounds = 0, iters = 0;
    for (uint32_t s = 0; s < nsub; ++s) { first[s] = total; total += count[s] & 0xFFFFFF; flags |= count[s] >> 24; }
    for (uint32_t gi = 0; gi < nruns; ++gi) { rounds = run_round[gi] + 1 > rounds ? run_round[gi] + 1 : rounds; iters = run_iters[gi] > iters ? run_iters[gi] : iters; }
    if (total != g.nblocks) flags |= Y7T_JD_E_COUNT;
    if (nsub) { const y7t_jd_state last = exit_[nsub - 1]; if (y7t_jd_state_b(last) || y7t_jd_state_z(last)) flags |= Y7T_JD_E_TRUNC; }
    info[0] = flags; info[1] = rounds; info[2] = iters; info[3] = (int)nruns; info[4] = (int)nsub;

    // ---- memset, k_jd_write ----
    memset(coef, 0, (size_t)g.nblocks * 128);
    for (uint32_t s = 0; s < nsub; ++s) {
        int cnt, fl;
        y7t_jd_lane(scan, d.scan_len, g, tab.dc, tab.ac, d.restart_interval, entry[s], 8u * (s + 1) * S, coef, first[s], &cnt, &fl);
        count[s] = cnt | fl << 24;
    }
    for (uint32_t s = 0; s < nsub; ++s) info[0] |= (count[s] >> 24) & Y7T_JD_E_RESTART;      // (k_jd_dc)
    if (diff_out) memcpy(diff_out, coef, (size_t)g.nblocks * 128);

    // ---- k_jd_dc: `lanes` threads, a contiguous share of the MCUs each ----
    {
        const int nm = g.mcols * g.mrows, T = lanes, per = (nm + T - 1) / T;
        std::vector<Y7TJdDcPart> part(T);
        Y7TJdDcPart zero = {{0, 0, 0}, 0};
        for (int t = 0; t < T; ++t) { const int m0 = t * per < nm ? t * per : nm, m1 = m0 + per < nm ? m0 + per : nm; part[t] = y7t_jd_dc_walk(g, d.restart_interval, coef, m0, m1, zero, false); }
        Y7TJdDcPart carry = zero;
        for (int t = 0; t < T; ++t) {
            const int m0 = t * per < nm ? t * per : nm, m1 = m0 + per < nm ? m0 + per : nm;
            y7t_jd_dc_walk(g, d.restart_interval, coef, m0, m1, carry, true);
            carry = y7t_jd_dc_join(carry, part[t]);
        }
    }
    if (coef_out) memcpy(coef_out, coef, (size_t)g.nblocks * 128);

    // ---- k_jd_pixels: whole planes here, tiles with their chroma context on the device ----
    const int pw = g.mcols * g.mw, ph = g.mrows * g.mh, cw = g.mcols * 8, ch = g.mrows * 8;
    std::vector<unsigned char> py((size_t)pw * ph), pc[3];
    for (int c = 0; c < g.comps; ++c) {
        const QTab q = {&file, d.dqt_off[d.tq[c] & 3]};
        const int bw = c == 0 ? pw / 8 : cw / 8, bh = c == 0 ? ph / 8 : ch / 8;
        if (c) pc[c].resize((size_t)cw * ch);
        unsigned char* plane = c == 0 ? py.data() : pc[c].data();
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx) {
                int v[64];
                y7t_jd_block(coef + (size_t)y7t_jd_block_index(g, c, bx, by) * 64, q, v);
                for (int i = 0; i < 64; ++i) plane[(size_t)(by * 8 + (i >> 3)) * (bw * 8) + bx * 8 + (i & 7)] = (unsigned char)v[i];
            }
    }
    const PlaneY Y = {py.data(), pw};
    const PlaneC C = {{nullptr, pc[1].data(), pc[2].data()}, cw};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) y7t_jd_pixel(g, Y, C, x, y, frame + ((size_t)y * W + x) * 3);
    return 0;
}
}
