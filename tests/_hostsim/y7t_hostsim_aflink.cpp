// tests/_hostsim/y7t_hostsim_aflink.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of the candidate stage of yolov7-tracker_amd/csrc/y7t_aflink.h: the gate, the row-major compaction and the pair transform of csrc/y7t_aflink.hip
// (k_afl_gate_count, k_afl_scan, k_afl_emit, k_afl_transform) run one item at a time with the SAME bodies, so that the pair list and the transformed blocks can be
// compared bit for bit with the NumPy restatement without a GPU.  The product package never loads this library.
#include "../../yolov7-tracker_amd/csrc/y7t_aflink.h"

extern "C" {
// -> pairs (max_pairs x 2), x1 / x2 (max_pairs x 90), count (all candidates), status (Y7T_AFL_OVERFLOW when count > max_pairs)
void hs_afl_candidates(const double* rows, const int* off, int n, double t0, double t1, double s, int max_pairs, int* pairs, float* x1, float* x2, int* count,
                       int* status) {
    int run = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (!y7t_afl_gate(rows, off, i, j, t0, t1, s)) continue;
            if (run < max_pairs) { pairs[2 * run] = i; pairs[2 * run + 1] = j; }
            ++run;
        }
    *count = run;
    *status = run > max_pairs ? Y7T_AFL_OVERFLOW : 0;
    const int m = run < max_pairs ? run : max_pairs;
    for (int p = 0; p < m; ++p) {
        const int trk[2] = {pairs[2 * p], pairs[2 * p + 1]};
        for (int c = 0; c < 3; ++c) {
            double mn = 0.0, mx = 0.0;
            for (int row = 0; row < 60; ++row) {
                const double v = y7t_afl_block_at(rows, off, trk[row / 30], row / 30, row % 30, c);
                if (row == 0 || v < mn) mn = v;
                if (row == 0 || v > mx) mx = v;
            }
            double sub, div;
            y7t_afl_norm(mn, mx, &sub, &div);
            for (int row = 0; row < 60; ++row) {
                const double v = y7t_afl_block_at(rows, off, trk[row / 30], row / 30, row % 30, c);
                (row < 30 ? x1 : x2)[(size_t)p * 90 + (row % 30) * 3 + c] = y7t_afl_apply(v, sub, div);
            }
        }
    }
}
int hs_afl_chunk(void) { return Y7T_AFL_CHUNK; }
int hs_afl_head_pairs(void) { return Y7T_AFL_HEAD_PAIRS; }
}
