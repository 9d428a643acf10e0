// tests/_hostsim/y7t_hostsim_gsi.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of yolov7-tracker_amd/csrc/y7t_gsi.h: the interpolation arithmetic of csrc/y7t_gsi.hip (k_gsi_count, k_gsi_scan, k_gsi_write) run one row at a
// time, and the per-track smoother y7t_gsi_track -- the SAME body the device's workgroups run -- at nt = 1, the matrix instruction replaced by the same sixteen
// products summed in the same k order (y7t_gsi_tile).  Tracks of up to 128 rows use the LDS row stride, longer ones the pool's, like the device.  The product
// package never loads this library.
#include "../../yolov7-tracker_amd/csrc/y7t_gsi.h"
#include <vector>

extern "C" {
// -> runs_out (max_rows x 5), off_out (n + 1), src_out (max_rows), count, status
void hs_gsi_interpolate(const double* runs, const int* off, int n, int interval, int max_rows, int max_len, double* runs_out, int* off_out, int* src_out, int* count,
                        int* status) {
    long long pos = 0;
    int st = 0;
    off_out[0] = 0;
    for (int k = 0; k < n; ++k) {
        const long long first = pos;
        for (int r = off[k]; r < off[k + 1]; ++r) {
            const double* a = runs + (size_t)r * Y7T_GSI_COLS;
            const double* b = a + Y7T_GSI_COLS;
            const int fill = r + 1 < off[k + 1] ? y7t_gsi_fill(a[0], b[0], interval) : 0;
            for (int i = 0; i <= fill; ++i, ++pos) {
                if (pos >= max_rows) continue;
                double* d = runs_out + (size_t)pos * Y7T_GSI_COLS;
                if (i == 0) {
                    for (int c = 0; c < Y7T_GSI_COLS; ++c) d[c] = a[c];
                } else {
                    d[0] = a[0] + (double)i;
                    for (int c = 1; c < Y7T_GSI_COLS; ++c) d[c] = y7t_gsi_lerp(a[c], b[c], b[0] - a[0], (double)i);
                }
                src_out[pos] = r;
            }
        }
        if (pos - first > max_len) st |= Y7T_GSI_LEN_OVERFLOW;
        off_out[k + 1] = (int)pos;
    }
    if (pos > max_rows) st |= Y7T_GSI_ROWS_OVERFLOW;
    *count = (int)pos;
    *status = st;
}

// -> out (rows x 4), status (n)
void hs_gsi_smooth(const double* runs, const int* off, const double* len_scale, int n, int longest, double reg, double* out, int* status) {
    for (int k = 0; k < n; ++k) {
        const int r0 = off[k], len = off[k + 1] - r0;
        for (int e = 0; e < len * 4; ++e) out[(size_t)r0 * 4 + e] = runs[(size_t)(r0 + (e >> 2)) * Y7T_GSI_COLS + 1 + (e & 3)];
        status[k] = len < 1 ? 0 : (len > longest ? Y7T_GSI_TOO_LONG : Y7T_GSI_PENDING);
        if (len < 1 || len > longest || len > Y7T_GSI_MAX_LEN) continue;
        const int np = y7t_gsi_pad(len);
        const size_t ld = y7t_gsi_class(len) == 0 ? Y7T_GSI_LDS_LEN + Y7T_GSI_LDS_PAD : np;
        std::vector<double> A((size_t)np * ld), Y((size_t)np * 4), t(np), D(272);
        const Y7TGsiExec ex = {0, 1, 0, 1, 0, 1};
        status[k] = y7t_gsi_track(ex, A.data(), ld, Y.data(), t.data(), D.data(), runs + (size_t)r0 * Y7T_GSI_COLS, len, len_scale[k], reg, out + (size_t)r0 * 4);
    }
}
int hs_gsi_lds_len(void) { return Y7T_GSI_LDS_LEN; }
int hs_gsi_max_len(void) { return Y7T_GSI_MAX_LEN; }
}
