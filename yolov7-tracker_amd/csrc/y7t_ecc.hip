// y7t_ecc.hip -- the ECC camera-motion estimate on the device (csrc/y7t_ecc.h states the arithmetic; DESIGN.md section 4 "GMC / ECC").
//
// Launch scheme.  y7t_ecc_align enqueues: one single-thread launch that writes the start state; max_iters + 1 launches of k_ecc_iter; one single-thread launch
// that writes the 2x3 warp and the status.  Launch k of k_ecc_iter first combines the slabs of partial sums that launch k - 1 left (every workgroup, in the same
// order, so all hold the same new parameters: the launch boundary is the grid-wide barrier), solves the 3x3 system, tests OpenCV's loop condition and, unless the
// estimate is finished, runs its pass over the template grid with the new parameters and leaves its own slabs.  The state header and the slabs are double
// buffered (k & 1), so no workgroup of launch k reads what another workgroup of launch k writes.  A launch that finds the estimate finished copies the header
// forward and returns at once.  The host reads NOTHING back between the launches -- no sample of the `done` word either: apply_device keeps the tracker's frame
// asynchronous, and a finished launch costs a few microseconds where a host read costs a stream synchronise.  No float atomics, no graph capture.
#include "y7t_common.h"
#include "y7t_ecc.h"

static inline hipStream_t S(y7t_stream s) { return (hipStream_t)s; }

// -- prepare: one launch, 32 x 8 output pixels per workgroup; I of the tile and its one-pixel halo in LDS, the gradients from there -------------------------
enum { PT_W = 32, PT_H = 8, PT_LW = PT_W + 2, PT_LH = PT_H + 2 };

__global__ __launch_bounds__(256) void k_ecc_prepare(const uint8_t* __restrict__ bgr, int H, int W, int ds, int h, int w, Y7TEccPix* __restrict__ plane) {
    __shared__ float sI[PT_LH][PT_LW + 1];
    const int tid = threadIdx.x, tx0 = blockIdx.x * PT_W, ty0 = blockIdx.y * PT_H;
    for (int i = tid; i < PT_LH * PT_LW; i += 256) {
        const int r = i / PT_LW, c = i - r * PT_LW;
        const int y = y7t_ecc_reflect101(ty0 - 1 + r, h), x = y7t_ecc_reflect101(tx0 - 1 + c, w);
        sI[r][c] = y7t_ecc_plane_I(bgr, H, W, ds, h, w, y, x);
    }
    __syncthreads();
    const int lx = tid & (PT_W - 1), ly = tid / PT_W, x = tx0 + lx, y = ty0 + ly;
    if (x < w && y < h) {
        Y7TEccPix o;
        o.I = sI[ly + 1][lx + 1];
        o.gx = 0.5f * (sI[ly + 1][lx + 2] - sI[ly + 1][lx]);
        o.gy = 0.5f * (sI[ly + 2][lx + 1] - sI[ly][lx + 1]);
        o.pad = 0.0f;
        plane[(size_t)y * w + x] = o;
    }
}

// -- iterate ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ void k_ecc_start(void* ws, double th, double tx, double ty, double eps) { y7t_ecc_start(y7t_ecc_hdr(ws, 0), th, tx, ty, eps); }

// solve_prev: combine + solve the slabs of launch k - 1 first (every launch but the first)
__global__ __launch_bounds__(Y7T_ECC_THREADS) void k_ecc_iter(const Y7TEccPix* __restrict__ tmpl, const Y7TEccPix* __restrict__ img, int h, int w, int nwg,
                                                              long long chunk, int k, int solve_prev, int max_iters, double eps, void* ws) {
    __shared__ double sS[Y7T_ECC_SLAB];
    __shared__ Y7TEccHdr sH;
    __shared__ Y7TEccWarpF sWp;
    __shared__ double sW[Y7T_ECC_NWAVE][Y7T_ECC_NSUM];
    __shared__ double sP[Y7T_ECC_CGROUPS][Y7T_ECC_NSUM];
    const int tid = threadIdx.x;
    const Y7TEccHdr* prev = y7t_ecc_hdr(ws, k - 1);
    Y7TEccHdr* cur = y7t_ecc_hdr(ws, k);
    if (prev->flag) {      // finished in an earlier launch (the same answer in every work-item of the grid: launch k - 1 wrote it)
        if (blockIdx.x == 0 && tid == 0) *cur = *prev;
        return;
    }
    if (solve_prev) {      // the slab combine in the order of y7t_ecc_combine: group g = tid / 32 sums slabs g, g + 32, ... for value j = tid % 32
        const double* sl = y7t_ecc_slabs(ws, h, w, k - 1);
        const int j = tid & 31, g = tid >> 5;
        if (j < Y7T_ECC_NSUM) {
            double part = 0.0;
            for (int s = g; s < nwg; s += Y7T_ECC_CGROUPS) part += sl[(size_t)s * Y7T_ECC_SLAB + j];
            sP[g][j] = part;
        }
        __syncthreads();
        if (tid < Y7T_ECC_NSUM) {
            double a = 0.0;
            for (int gg = 0; gg < Y7T_ECC_CGROUPS; ++gg) a += sP[gg][tid];
            sS[tid] = a;
        }
    }
    __syncthreads();
    if (tid == 0) {
        Y7TEccHdr hd = *prev;
        if (solve_prev) y7t_ecc_solve(sS, &hd);
        y7t_ecc_check(&hd, max_iters, eps);
        sH = hd;
        sWp = y7t_ecc_warp_f32(hd.p);      // (once per workgroup: the sine / cosine series is float64)
        if (blockIdx.x == 0) *cur = hd;
    }
    __syncthreads();
    if (sH.flag) return;
    const Y7TEccWarpF wp = sWp;
    double acc[Y7T_ECC_NSUM];
#pragma unroll
    for (int i = 0; i < Y7T_ECC_NSUM; ++i) acc[i] = 0.0;
    const long long npix = (long long)h * w, lo = (long long)blockIdx.x * chunk, hi = lo + chunk < npix ? lo + chunk : npix;
    for (long long i = lo + tid; i < hi; i += Y7T_ECC_THREADS) {
        const int y = (int)(i / w), x = (int)(i - (long long)y * w);
        y7t_ecc_pixel(img, tmpl, h, w, x, y, wp, acc);
    }
    // within the wave by shuffles, across the waves through LDS (lane 0 of each wave writes its 21 values: no two lanes of one instruction, no bank conflict)
#pragma unroll
    for (int i = 0; i < Y7T_ECC_NSUM; ++i) {
#pragma unroll
        for (int off = Y7T_ECC_WAVE / 2; off >= 1; off >>= 1) acc[i] += __shfl_down(acc[i], off, Y7T_ECC_WAVE);
    }
    if ((tid & (Y7T_ECC_WAVE - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < Y7T_ECC_NSUM; ++i) sW[tid / Y7T_ECC_WAVE][i] = acc[i];
    }
    __syncthreads();
    if (tid < Y7T_ECC_SLAB) {
        double a = 0.0;
        if (tid < Y7T_ECC_NSUM)
            for (int wv = 0; wv < Y7T_ECC_NWAVE; ++wv) a += sW[wv][tid];
        y7t_ecc_slabs(ws, h, w, k)[(size_t)blockIdx.x * Y7T_ECC_SLAB + tid] = a;
    }
}

__global__ void k_ecc_finish(const void* ws, int k, double* warp6, double* status4) { y7t_ecc_finish(y7t_ecc_hdr((void*)ws, k), warp6, status4); }

__global__ void k_ecc_sums_out(const void* ws, int h, int w, int nwg, int k, double* sums) {
    if (threadIdx.x == 0) y7t_ecc_combine(y7t_ecc_slabs((void*)ws, h, w, k), nwg, sums);
}

// -- C ABI -----------------------------------------------------------------------------------------------------------------------------------------------
static int plane_dims_ok(int h, int w) { return h >= 2 && w >= 2 && (long long)h * w <= (1ll << 30); }

extern "C" int y7t_ecc_prepare_u8(const uint8_t* bgr, int H, int W, int downscale, void* plane_out, y7t_stream stream) {
    Y7T_ARG_CHECK(bgr && plane_out && downscale >= 1 && H >= 1 && W >= 1);
    const int h = H / downscale, w = W / downscale;
    Y7T_ARG_CHECK(plane_dims_ok(h, w));
    y7t_note_kernel("k_ecc_prepare");
    hipLaunchKernelGGL(k_ecc_prepare, dim3((w + PT_W - 1) / PT_W, (h + PT_H - 1) / PT_H), dim3(256), 0, S(stream), bgr, H, W, downscale, h, w, (Y7TEccPix*)plane_out);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_ecc_workspace_bytes(int h, int w, size_t* out) {
    Y7T_ARG_CHECK(out && plane_dims_ok(h, w));
    *out = y7t_ecc_ws_bytes(h, w);
    return 0;
}

extern "C" int y7t_ecc_align(const void* tmpl_plane, const void* img_plane, int h, int w, int motion, int max_iters, double eps, void* workspace,
                             double* warp_out6_f64, double* status_out, y7t_stream stream) {
    Y7T_ARG_CHECK(motion == Y7T_ECC_MOTION_EUCLIDEAN);
    Y7T_ARG_CHECK(tmpl_plane && img_plane && workspace && warp_out6_f64 && status_out && plane_dims_ok(h, w));
    Y7T_ARG_CHECK(max_iters >= 0 && max_iters <= 10000 && eps == eps);
    Y7T_ARG_CHECK(((uintptr_t)tmpl_plane & 15) == 0 && ((uintptr_t)img_plane & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    const int nwg = y7t_ecc_num_wg(h, w);
    const long long chunk = y7t_ecc_chunk(h, w);
    hipLaunchKernelGGL(k_ecc_start, dim3(1), dim3(1), 0, S(stream), workspace, 0.0, 0.0, 0.0, eps);
    y7t_note_kernel("k_ecc_iter");
    for (int k = 1; k <= max_iters + 1; ++k)
        hipLaunchKernelGGL(k_ecc_iter, dim3(nwg), dim3(Y7T_ECC_THREADS), 0, S(stream), (const Y7TEccPix*)tmpl_plane, (const Y7TEccPix*)img_plane, h, w, nwg, chunk, k,
                           k > 1 ? 1 : 0, max_iters, eps, workspace);
    hipLaunchKernelGGL(k_ecc_finish, dim3(1), dim3(1), 0, S(stream), (const void*)workspace, max_iters + 1, warp_out6_f64, status_out);
    Y7T_LAUNCH_CHECK();
    return 0;
}

extern "C" int y7t_ecc_iteration_sums_f64(const void* tmpl_plane, const void* img_plane, int h, int w, double theta, double tx, double ty, void* workspace,
                                          double* sums_out21_f64, y7t_stream stream) {
    Y7T_ARG_CHECK(tmpl_plane && img_plane && workspace && sums_out21_f64 && plane_dims_ok(h, w));
    Y7T_ARG_CHECK(((uintptr_t)tmpl_plane & 15) == 0 && ((uintptr_t)img_plane & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    const int nwg = y7t_ecc_num_wg(h, w);
    hipLaunchKernelGGL(k_ecc_start, dim3(1), dim3(1), 0, S(stream), workspace, theta, tx, ty, -1.0);
    hipLaunchKernelGGL(k_ecc_iter, dim3(nwg), dim3(Y7T_ECC_THREADS), 0, S(stream), (const Y7TEccPix*)tmpl_plane, (const Y7TEccPix*)img_plane, h, w, nwg,
                       y7t_ecc_chunk(h, w), 1, 0, 1, -1.0, workspace);
    hipLaunchKernelGGL(k_ecc_sums_out, dim3(1), dim3(64), 0, S(stream), (const void*)workspace, h, w, nwg, 1, sums_out21_f64);
    Y7T_LAUNCH_CHECK();
    return 0;
}
