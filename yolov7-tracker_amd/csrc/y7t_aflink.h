// y7t_aflink.h -- the appearance-free link model of StrongSORT++ (the reference ships its network, tracker/reid_models/AFLink.py: class PostLinker): the constants
// of the device kernels (csrc/y7t_aflink.hip) and the candidate gate and the pair transform stated once, for those kernels and for the CPU build of the same
// bodies (tests/_hostsim/aflink.py).  DESIGN.md section 4 "AFLink" is the specification and tests/aflink_np.py its NumPy restatement.  Every operation here is a
// comparison or ONE correctly rounded float64 operation (subtract, multiply, add, sqrt, divide, the cast to float32), so the three agree bit for bit; the file is
// compiled with -ffp-contract=off on both sides and says so itself where a product feeds a sum.  Portable text: no HIP header is needed.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define Y7T_AFL_HD __host__ __device__ inline
#else
#define Y7T_AFL_HD static inline
#endif
#if defined(__clang__)
#define Y7T_AFL_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define Y7T_AFL_NO_CONTRACT
#endif

#ifndef Y7T_AFL_CHUNK_PAIRS
#define Y7T_AFL_CHUNK_PAIRS 2048      // (a -D of the build may override it: profiles/aflink_timing.txt compares 512, 1024 and 2048)
#endif
enum {
    Y7T_AFL_LEN = 30,                  // rows of a tracklet the network sees
    Y7T_AFL_BLOCK = 90,                // floats of one (30, 3) block
    Y7T_AFL_CHUNK = Y7T_AFL_CHUNK_PAIRS,   // pairs per chunk: the network runs layer by layer over a chunk (two ping-pong activation buffers of 36 KiB a pair)
    Y7T_AFL_HEAD_PAIRS = 8,            // pairs per workgroup of the pooling + classifier kernel
    Y7T_AFL_NUM_WEIGHTS = 1075266,     // float tensors of PostLinker().state_dict(), packed
    Y7T_AFL_MAX_TRACKLETS = 32768,     // N * N candidates are counted in 32-bit integers
    Y7T_AFL_OVERFLOW = 1,              // status bit: more candidates than max_pairs
};

// the gate of the ordered pair (i, j): i ends (last frame fi, last position bi) before j begins (first frame fj, first position bj)
//   thrT0 <= fj - fi < thrT1  and not  thrS < sqrt(dx * dx + dy * dy)
Y7T_AFL_HD bool y7t_afl_gate(const double* rows, const int* off, int i, int j, double t0, double t1, double s) {
    Y7T_AFL_NO_CONTRACT
    if (i == j || off[i + 1] <= off[i] || off[j + 1] <= off[j]) return false;
    const double* a = rows + (size_t)(off[i + 1] - 1) * 3;
    const double* b = rows + (size_t)off[j] * 3;
    const double dt = b[0] - a[0];
    if (!(t0 <= dt && dt < t1)) return false;
    const double dx = a[1] - b[1], dy = a[2] - b[2];
    const double xx = dx * dx, yy = dy * dy;
    const double d = sqrt(xx + yy);
    return !(s < d);
}

// element (r, c) of a tracklet's (30, 3) block: the FORMER keeps its last 30 rows, padded with zero rows in front; the LATTER its first 30, padded behind
Y7T_AFL_HD double y7t_afl_block_at(const double* rows, const int* off, int trk, int latter, int r, int c) {
    const int n = off[trk + 1] - off[trk];
    int src;
    if (latter) src = r < n ? r : -1;
    else src = n >= Y7T_AFL_LEN ? n - Y7T_AFL_LEN + r : (r >= Y7T_AFL_LEN - n ? r - (Y7T_AFL_LEN - n) : -1);
    return src < 0 ? 0.0 : rows[(size_t)(off[trk] + src) * 3 + c];
}

// min_ and max_ of a column over the 60 rows -> subtractor = (max_ + min_) / 2, divisor = (max_ - min_) / 2 + 1e-5
Y7T_AFL_HD void y7t_afl_norm(double mn, double mx, double* sub, double* div) {
    Y7T_AFL_NO_CONTRACT
    const double s = mx + mn, d = mx - mn;
    const double h = d / 2.0;
    *sub = s / 2.0;
    *div = h + 1e-5;
}
Y7T_AFL_HD float y7t_afl_apply(double x, double sub, double div) {
    Y7T_AFL_NO_CONTRACT
    const double d = x - sub;
    return (float)(d / div);
}
