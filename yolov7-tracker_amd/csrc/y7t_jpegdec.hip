// y7t_jpegdec.hip -- baseline JPEG files to BGR frames on the device, as gfx950 kernels (csrc/y7t_jpegdec.h states the arithmetic; DESIGN.md section 4 "JPEG
// decoding" is the specification and tests/jpegdec_np.py its NumPy restatement).  Integer arithmetic decides every bit and every pixel; no atomics, no flags between
// workgroups, no read-back: a kernel boundary is the only hand-over between workgroups, results are bit-identical from call to call and a file's do not depend on
// the rest of the batch.
//
//   k_jd_sync     launch r of `nruns` (the runs of the batch's longest scan).  The scan is cut into subsequences of subseq_bytes stuffed bytes, a lane each; a
//                 workgroup owns a run of 256.  A lane decodes from an assumed state and records where and in which state it left; a lane whose predecessor left
//                 in another state than the lane entered decodes again, until the run agrees with its own entry (<= lanes + 1 rounds).  Launch 0 does that for every
//                 run; launch r > 0 reads the exit launch r - 1 left for the run before, and returns at once where it is the entry the run already used.  After
//                 launch r the runs 0 .. r are final, so `nruns` launches suffice whatever the stream.  A restart marker resets the state, so runs agree sooner.
//   k_jd_scan     a workgroup per file: the exclusive sum of the lanes' block counts places every lane's first block; the file's status word and round counts
//   k_jd_write    the lanes once more from their final entry states, storing the coefficients (the buffer was cleared: only non-zero ones are stored)
//   k_jd_dc       a workgroup per file: the write pass's restart-marker findings into the status word; the DC differences -> values, a segmented inclusive sum per component in scan order, from 0 again at every restart interval
//   k_jd_pixels   a workgroup per tile of 8 x 4 MCUs: a thread per block (the tile's and, where chroma is subsampled, a ring of chroma blocks around it) does
//                 dequantisation and the inverse DCT into the LDS, then 4 pixels a thread: chroma upsampling, colour, BGR bytes straight into the frame
#include "y7t_jpegdec.h"
#include "y7t_common.h"
#include <mutex>
#include <unordered_map>
#include <vector>

enum { kLanes = Y7T_JD_LANES, kTX = 8, kTY = 4, kLumaPitch = kTX * 16, kChromaPitch = kTX * 8 + 16, kChromaRows = kTY * 8 + 16 };

struct JdArgs {
    Y7TJdGeom g;
    Y7TJdLayout L;
    const unsigned char* files;
    char* obj;
    int S, max_batch;
};

struct JdFile {      // a file's slices of the object
    Y7TJdDesc d;
    uint32_t nsub, nruns;
    y7t_jd_state *entry, *exit_, *run_exit[2], *run_entry;
    int *count, *first, *run_round, *run_iters;
    short* coef;
};
__device__ inline JdFile jd_file(const JdArgs& a, int b) {
    JdFile f;
    f.d = ((const Y7TJdDesc*)(a.obj + a.L.descs))[b];
    f.nsub = (f.d.scan_len + (uint32_t)a.S - 1) / (uint32_t)a.S;
    if (f.nsub > a.L.nsub) f.nsub = a.L.nsub;
    f.nruns = (f.nsub + kLanes - 1) / kLanes;
    const size_t so = (size_t)b * a.L.nsub, ro = (size_t)b * a.L.nruns;
    f.entry = (y7t_jd_state*)(a.obj + a.L.entry) + so;
    f.exit_ = (y7t_jd_state*)(a.obj + a.L.exit) + so;
    f.count = (int*)(a.obj + a.L.count) + so;
    f.first = (int*)(a.obj + a.L.first) + so;
    f.run_exit[0] = (y7t_jd_state*)(a.obj + a.L.run_exit) + ro;
    f.run_exit[1] = f.run_exit[0] + (size_t)a.max_batch * a.L.nruns;
    f.run_entry = (y7t_jd_state*)(a.obj + a.L.run_entry) + ro;
    f.run_round = (int*)(a.obj + a.L.run_round) + ro;
    f.run_iters = (int*)(a.obj + a.L.run_iters) + ro;
    f.coef = (short*)(a.obj + a.L.coef) + (size_t)b * a.g.nblocks * 64;
    return f;
}
__device__ inline void jd_tables(const JdArgs& a, const Y7TJdDesc& d, Y7TJdHuff* dc, Y7TJdHuff* ac) {      // a thread per table; the caller's barrier follows
    const Y7TJdBytes file = {a.files + d.file_off, d.file_len};
    const int t = threadIdx.x;
    if (t < 2 * a.g.comps) {
        const int c = t >> 1;
        if (t & 1) y7t_jd_build_huff(file, d.ac_off[d.ta[c] & 3], &ac[c]);
        else y7t_jd_build_huff(file, d.dc_off[d.td[c] & 3], &dc[c]);
    }
}

__global__ void __launch_bounds__(kLanes) k_jd_sync(JdArgs a, int r) {
    __shared__ Y7TJdHuff dc[3], ac[3];
    __shared__ y7t_jd_state ex[kLanes];
    const int tid = threadIdx.x;
    const uint32_t gi = blockIdx.x;
    const JdFile f = jd_file(a, blockIdx.y);
    if (gi >= f.nruns) return;
    const uint32_t S = (uint32_t)a.S;
    const y7t_jd_state* prev = f.run_exit[(r + 1) & 1];
    y7t_jd_state* cur = f.run_exit[r & 1];
    const y7t_jd_state e = gi == 0 ? y7t_jd_pack(0, 0, 0) : (r == 0 ? y7t_jd_assumed(gi * kLanes, S) : prev[gi - 1]);
    if (r > 0 && e == f.run_entry[gi]) {      // nothing left to do (the condition is the workgroup's): the exit moves on to this launch's buffer
        if (tid == 0) cur[gi] = prev[gi];
        return;
    }
    jd_tables(a, f.d, dc, ac);
    __syncthreads();
    const Y7TJdBytes scan = {a.files + f.d.file_off + f.d.scan_off, f.d.scan_len};
    const uint32_t s0 = gi * kLanes, n = f.nsub - s0 < kLanes ? f.nsub - s0 : kLanes, s = s0 + (uint32_t)tid;
    const bool active = (uint32_t)tid < n;
    y7t_jd_state my_entry = 0, my_exit = 0;
    int word = 0, cnt, fl;
    if (active) {
        if (r == 0 || tid == 0) {
            my_entry = tid == 0 ? e : y7t_jd_assumed(s, S);
            my_exit = y7t_jd_lane(scan, f.d.scan_len, a.g, dc, ac, f.d.restart_interval, my_entry, 8u * (s + 1) * S, nullptr, 0, &cnt, &fl);
            word = cnt | fl << 24;
        } else { my_entry = f.entry[s]; my_exit = f.exit_[s]; word = f.count[s]; }
    }
    ex[tid] = my_exit;
    int iters = 1;
    for (;;) {
        __syncthreads();
        const y7t_jd_state want = tid == 0 ? e : ex[tid - 1];
        __syncthreads();      // (every lane has read its predecessor's exit before one is written)
        const bool again = active && want != my_entry;
        if (again) {
            my_entry = want;
            my_exit = y7t_jd_lane(scan, f.d.scan_len, a.g, dc, ac, f.d.restart_interval, my_entry, 8u * (s + 1) * S, nullptr, 0, &cnt, &fl);
            word = cnt | fl << 24;
            ex[tid] = my_exit;
        }
        ++iters;
        if (!__syncthreads_or(again)) break;
    }
    if (active) { f.entry[s] = my_entry; f.exit_[s] = my_exit; f.count[s] = word; }
    if ((uint32_t)tid == n - 1) cur[gi] = my_exit;
    if (tid == 0) { f.run_entry[gi] = e; f.run_round[gi] = r; f.run_iters[gi] = iters; }
}

__global__ void __launch_bounds__(kLanes) k_jd_scan(JdArgs a, int* __restrict__ status) {
    __shared__ int sc[kLanes], fls[kLanes];
    const int tid = threadIdx.x, b = blockIdx.x;
    const JdFile f = jd_file(a, b);
    const uint32_t per = (f.nsub + kLanes - 1) / kLanes;
    const uint32_t lo = min((uint32_t)tid * per, f.nsub), hi = min(lo + per, f.nsub);
    int sum = 0, fl = 0;
    for (uint32_t s = lo; s < hi; ++s) { const int w = f.count[s]; sum += w & 0xFFFFFF; fl |= w >> 24; }
    sc[tid] = sum; fls[tid] = fl;
    __syncthreads();
    for (int w = 1; w < kLanes; w <<= 1) {
        const int v = tid >= w ? sc[tid - w] : 0, g2 = tid >= w ? fls[tid - w] : 0;
        __syncthreads();
        sc[tid] += v; fls[tid] |= g2;
        __syncthreads();
    }
    int at = sc[tid] - sum;
    for (uint32_t s = lo; s < hi; ++s) { f.first[s] = at; at += f.count[s] & 0xFFFFFF; }
    if (tid == 0) {
        int flags = fls[kLanes - 1], rounds = 0, iters = 0;
        if (sc[kLanes - 1] != a.g.nblocks) flags |= Y7T_JD_E_COUNT;
        if (f.nsub) { const y7t_jd_state last = f.exit_[f.nsub - 1]; if (y7t_jd_state_b(last) || y7t_jd_state_z(last)) flags |= Y7T_JD_E_TRUNC; }
        for (uint32_t gi = 0; gi < f.nruns; ++gi) { rounds = max(rounds, f.run_round[gi] + 1); iters = max(iters, f.run_iters[gi]); }
        status[b] = flags;
        ((int*)(a.obj + a.L.rounds))[b] = rounds;
        ((int*)(a.obj + a.L.iters))[b] = iters;
    }
}

__global__ void __launch_bounds__(kLanes) k_jd_write(JdArgs a) {
    __shared__ Y7TJdHuff dc[3], ac[3];
    const JdFile f = jd_file(a, blockIdx.y);
    if (blockIdx.x >= f.nruns) return;
    jd_tables(a, f.d, dc, ac);
    __syncthreads();
    const uint32_t s = blockIdx.x * kLanes + threadIdx.x;
    if (s >= f.nsub) return;
    const Y7TJdBytes scan = {a.files + f.d.file_off + f.d.scan_off, f.d.scan_len};
    int cnt, fl;
    y7t_jd_lane(scan, f.d.scan_len, a.g, dc, ac, f.d.restart_interval, f.entry[s], 8u * (s + 1) * (uint32_t)a.S, f.coef, f.first[s], &cnt, &fl);
    f.count[s] = cnt | fl << 24;      // (this pass knows every block's index: it alone can hold the restart markers against the restart interval; k_jd_dc collects)
}

__global__ void __launch_bounds__(kLanes) k_jd_dc(JdArgs a, int* __restrict__ status) {
    __shared__ Y7TJdDcPart part[kLanes];
    const int tid = threadIdx.x;
    const JdFile f = jd_file(a, blockIdx.x);
    const int nm = a.g.mcols * a.g.mrows, per = (nm + kLanes - 1) / kLanes;
    const int m0 = min(tid * per, nm), m1 = min(m0 + per, nm);
    int misplaced = 0;
    for (uint32_t s = tid; s < f.nsub; s += kLanes) misplaced |= (f.count[s] >> 24) & Y7T_JD_E_RESTART;
    misplaced = __syncthreads_or(misplaced);
    if (tid == 0 && misplaced) status[blockIdx.x] |= Y7T_JD_E_RESTART;      // (k_jd_scan wrote the word in an earlier launch; this thread alone touches it here)
    const Y7TJdDcPart zero = {{0u, 0u, 0u}, 0};
    part[tid] = y7t_jd_dc_walk(a.g, f.d.restart_interval, f.coef, m0, m1, zero, false);
    __syncthreads();
    for (int w = 1; w < kLanes; w <<= 1) {
        Y7TJdDcPart v = part[tid];
        if (tid >= w) v = y7t_jd_dc_join(part[tid - w], v);
        __syncthreads();
        part[tid] = v;
        __syncthreads();
    }
    y7t_jd_dc_walk(a.g, f.d.restart_interval, f.coef, m0, m1, tid ? part[tid - 1] : zero, true);
}

struct LdsY { const unsigned char* p; int x0, y0; __device__ int operator()(int x, int y) const { return p[(y - y0) * kLumaPitch + (x - x0)]; } };
struct LdsC { const unsigned char* p; int x0, y0; __device__ int operator()(int c, int x, int y) const { return p[(c - 1) * (kChromaPitch * kChromaRows) + (y - y0 + 8) * kChromaPitch + (x - x0 + 8)]; } };
struct LdsQ { const unsigned char* p; __device__ unsigned operator()(int k) const { return p[k]; } };

__global__ void __launch_bounds__(256) k_jd_pixels(JdArgs a, unsigned char* __restrict__ frames) {
    __shared__ unsigned ly[kLumaPitch * kTY * 16 / 4];
    __shared__ unsigned lc[2 * kChromaPitch * kChromaRows / 4];
    __shared__ unsigned char q[3][64];
    const Y7TJdGeom g = a.g;
    const int tid = threadIdx.x, b = blockIdx.z, mx0 = blockIdx.x * kTX, my0 = blockIdx.y * kTY;
    const Y7TJdDesc d = ((const Y7TJdDesc*)(a.obj + a.L.descs))[b];
    const short* coef = (const short*)(a.obj + a.L.coef) + (size_t)b * g.nblocks * 64;
    if (tid < 64 * g.comps) {
        const Y7TJdBytes file = {a.files + d.file_off, d.file_len};
        const uint32_t off = d.dqt_off[d.tq[tid >> 6] & 3];
        q[tid >> 6][tid & 63] = off ? (unsigned char)file(off + (uint32_t)(tid & 63)) : 1;
    }
    __syncthreads();
    const int nlx = kTX * g.hs, nl = nlx * kTY * g.vs;
    const int hx = g.hs == 2 ? 1 : 0, hy = g.vs == 2 ? 1 : 0, ncx = kTX + 2 * hx, nc = g.comps == 3 ? ncx * (kTY + 2 * hy) : 0;
    for (int it = tid; it < nl + 2 * nc; it += 256) {
        int c, bx, by;
        unsigned* dst;
        if (it < nl) {
            c = 0; bx = mx0 * g.hs + it % nlx; by = my0 * g.vs + it / nlx;
            if (bx >= g.mcols * g.hs || by >= g.mrows * g.vs) continue;
            dst = ly + ((it / nlx) * 8 * kLumaPitch + (it % nlx) * 8) / 4;
        } else {
            const int j = it - nl, k = j % nc;
            c = 1 + j / nc; bx = mx0 - hx + k % ncx; by = my0 - hy + k / ncx;
            if (bx < 0 || by < 0 || bx >= g.mcols || by >= g.mrows) continue;
            dst = lc + ((c - 1) * (kChromaPitch * kChromaRows) + ((by - my0) * 8 + 8) * kChromaPitch + (bx - mx0) * 8 + 8) / 4;
        }
        const int4* src = (const int4*)(coef + (size_t)y7t_jd_block_index(g, c, bx, by) * 64);
        short cf[64];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int4 v = src[i];
            cf[8 * i] = (short)v.x; cf[8 * i + 1] = (short)(v.x >> 16); cf[8 * i + 2] = (short)v.y; cf[8 * i + 3] = (short)(v.y >> 16);
            cf[8 * i + 4] = (short)v.z; cf[8 * i + 5] = (short)(v.z >> 16); cf[8 * i + 6] = (short)v.w; cf[8 * i + 7] = (short)(v.w >> 16);
        }
        int v[64];
        const LdsQ qc = {q[c]};
        y7t_jd_block(cf, qc, v);
        const int pitch = (c == 0 ? kLumaPitch : kChromaPitch) / 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dst[i * pitch] = (unsigned)v[8 * i] | (unsigned)v[8 * i + 1] << 8 | (unsigned)v[8 * i + 2] << 16 | (unsigned)v[8 * i + 3] << 24;
            dst[i * pitch + 1] = (unsigned)v[8 * i + 4] | (unsigned)v[8 * i + 5] << 8 | (unsigned)v[8 * i + 6] << 16 | (unsigned)v[8 * i + 7] << 24;
        }
    }
    __syncthreads();
    const int x0 = mx0 * g.mw, y0 = my0 * g.mh, tw4 = kTX * g.mw / 4, th = kTY * g.mh;
    const LdsY Y = {(const unsigned char*)ly, x0, y0};
    const LdsC C = {(const unsigned char*)lc, mx0 * 8, my0 * 8};
    const bool wide = (g.W & 3) == 0;      // (then the 12 bytes of 4 pixels are dword aligned, and x + 3 < W whenever x < W)
    for (int u = tid; u < tw4 * th; u += 256) {
        const int y = y0 + u / tw4, x = x0 + (u % tw4) * 4;
        if (y >= g.H || x >= g.W) continue;
        const int npx = min(4, g.W - x);
        unsigned char px[12];
        for (int i = 0; i < npx; ++i) y7t_jd_pixel(g, Y, C, x + i, y, px + 3 * i);
        unsigned char* o = frames + (((size_t)b * g.H + y) * g.W + x) * 3;
        if (npx == 4 && wide) {
            unsigned w3[3] = {0, 0, 0};
            for (int i = 0; i < 12; ++i) w3[i >> 2] |= (unsigned)px[i] << (8 * (i & 3));
            unsigned* o4 = (unsigned*)o;
            o4[0] = w3[0]; o4[1] = w3[1]; o4[2] = w3[2];
        } else {
            for (int i = 0; i < 3 * npx; ++i) o[i] = px[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct JdInfo { Y7TJdGeom g; Y7TJdLayout L; int S, max_batch; size_t max_file_bytes; std::vector<Y7TJdDesc> staging; };
static std::mutex g_jd_mu;
static std::unordered_map<const void*, JdInfo> g_jds;

static bool jd_setup(int H, int W, int components, int sampling, int max_batch, size_t max_file_bytes, int subseq_bytes, JdInfo* info) {
    if (H < 1 || W < 1 || H > Y7T_JPEGDEC_MAX_SIDE || W > Y7T_JPEGDEC_MAX_SIDE || sampling < 0 || sampling > Y7T_JD_GRAY) return false;
    if (components != (sampling == Y7T_JD_GRAY ? 1 : 3)) return false;
    info->S = subseq_bytes == 0 ? Y7T_JPEGDEC_SUBSEQ_DEFAULT : subseq_bytes;
    info->g = y7t_jd_geom(H, W, sampling);
    info->max_batch = max_batch; info->max_file_bytes = max_file_bytes;
    return y7t_jd_layout(info->g, max_batch, max_file_bytes, info->S, kLanes, &info->L);
}

extern "C" size_t y7t_jpegdec_bytes(int H, int W, int components, int sampling, int max_batch, size_t max_file_bytes, int subseq_bytes) {
    JdInfo info;
    return jd_setup(H, W, components, sampling, max_batch, max_file_bytes, subseq_bytes, &info) ? info.L.total : 0;
}

extern "C" int y7t_jpegdec_init(void* obj, size_t bytes, int H, int W, int components, int sampling, int max_batch, size_t max_file_bytes, int subseq_bytes,
                                y7t_stream stream) {
    Y7T_ARG_CHECK(obj && ((uintptr_t)obj & 255) == 0);
    JdInfo info;
    Y7T_ARG_CHECK(jd_setup(H, W, components, sampling, max_batch, max_file_bytes, subseq_bytes, &info));
    Y7T_ARG_CHECK(bytes >= info.L.total);
    Y7T_HIP_CHECK(hipMemsetAsync(obj, 0, info.L.descs, (hipStream_t)stream));      // (the round counts read 0 before the first call)
    std::lock_guard<std::mutex> l(g_jd_mu);
    g_jds[obj] = std::move(info);
    return 0;
}

extern "C" int y7t_jpegdec_release(void* obj) {
    std::lock_guard<std::mutex> l(g_jd_mu);
    g_jds.erase(obj);
    return 0;
}

extern "C" int y7t_jpegdec_decode(void* obj, const uint8_t* files, const y7t_jpegdec_desc* descs, int B, uint8_t* frames, int* status, y7t_stream stream) {
    static_assert(sizeof(Y7TJdDesc) == sizeof(y7t_jpegdec_desc) && sizeof(Y7TJdDesc) == 80, "the per-file record of include/y7t.h");
    std::lock_guard<std::mutex> l(g_jd_mu);      // (the staged records are the object's: one call at a time stages them)
    auto it = g_jds.find(obj);
    if (it == g_jds.end()) { y7t_set_error("this address holds no JPEG decoder (y7t_jpegdec_init)"); return Y7T_E_STATE; }
    JdInfo& info = it->second;
    Y7T_ARG_CHECK(B >= 0);
    if (B > info.max_batch) { y7t_set_error("y7t_jpegdec_decode: %d files exceed this decoder's capacity (max_batch = %d)", B, info.max_batch); return Y7T_E_CAPACITY; }
    if (B == 0) return 0;
    Y7T_ARG_CHECK(files && descs && frames && status && ((uintptr_t)frames & 3) == 0 && ((uintptr_t)status & 3) == 0);
    uint32_t longest = 0;
    for (int b = 0; b < B; ++b) {
        const Y7TJdDesc& d = ((const Y7TJdDesc*)descs)[b];
        if (d.file_len > info.max_file_bytes) {
            y7t_set_error("y7t_jpegdec_decode: file %d has %u bytes, this decoder takes %zu (max_file_bytes)", b, d.file_len, info.max_file_bytes);
            return Y7T_E_CAPACITY;
        }
        Y7T_ARG_CHECK(d.file_len >= 1 && (size_t)d.scan_off + d.scan_len <= d.file_len);
        for (int c = 0; c < 4; ++c) Y7T_ARG_CHECK(d.tq[c] < 4 && d.td[c] < 4 && d.ta[c] < 4);
        longest = d.scan_len > longest ? d.scan_len : longest;
    }
    // the records are copied from pageable memory: hipMemcpyAsync stages such a source before it returns (it is asynchronous only for pinned memory), which is what
    // lets the caller, and the next call's assign below, reuse the memory at once
    info.staging.assign((const Y7TJdDesc*)descs, (const Y7TJdDesc*)descs + B);
    hipStream_t st = (hipStream_t)stream;
    JdArgs a = {info.g, info.L, files, (char*)obj, info.S, info.max_batch};
    Y7T_HIP_CHECK(hipMemcpyAsync(a.obj + info.L.descs, info.staging.data(), (size_t)B * sizeof(Y7TJdDesc), hipMemcpyHostToDevice, st));
    Y7T_HIP_CHECK(hipMemsetAsync(a.obj + info.L.coef, 0, (size_t)B * info.g.nblocks * 128, st));
    const uint32_t nsub = (longest + (uint32_t)info.S - 1) / (uint32_t)info.S;
    const int nruns = (int)((nsub + kLanes - 1) / kLanes) > 1 ? (int)((nsub + kLanes - 1) / kLanes) : 1;
    for (int r = 0; r < nruns; ++r) {
        hipLaunchKernelGGL(k_jd_sync, dim3(nruns, B), dim3(kLanes), 0, st, a, r);
        Y7T_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_jd_scan, dim3(B), dim3(kLanes), 0, st, a, status);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jd_write, dim3(nruns, B), dim3(kLanes), 0, st, a);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jd_dc, dim3(B), dim3(kLanes), 0, st, a, status);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jd_pixels, dim3((info.g.mcols + kTX - 1) / kTX, (info.g.mrows + kTY - 1) / kTY, B), dim3(256), 0, st, a, frames);
    Y7T_LAUNCH_CHECK();
    return 0;
}
