// y7t_render.hip -- annotated frames on the device, as gfx950 kernels: the overlay of tracker/track.py's plot_img and a baseline JPEG encoder for what it returns
// (csrc/y7t_render.h states the arithmetic; DESIGN.md section 4 "Rendering" is the specification and tests/render_np.py its NumPy restatement).  Integer arithmetic
// decides every pixel and every bit; no global atomics; results are bit-identical from call to call and a frame's do not depend on its neighbours in the batch.
//
//   k_render_draw    a workgroup per 32 x 32 tile: the tracks whose primitives touch the tile are listed in the LDS 256 candidates at a time (a list per chunk, the
//                    chunks in track order: no cap), every pixel then takes the last primitive of the list that covers it.  Frames whose width is a multiple of 4
//                    move as dwords, 4 pixels a thread.
//   k_jpeg_blocks    a workgroup per 32 (4:2:0) or 64 (4:4:4) MCUs of an MCU row: the pixels go through the LDS as the dwords they arrive in, a thread per block
//                    does colour conversion, the 2 x 2 chroma mean, the DCT, quantisation and zigzag -> 64 int16 and a word (last non-zero index, bits of the AC code)
//   k_jpeg_entropy   a workgroup per MCU row, 256 blocks at a time with a carried bit offset: a scan of the blocks' bit lengths places every block, a thread forms its
//                    block's code words and ORs them into the LDS (y7t_render.h: Y7TJpegSink), a second scan over the 0xFF bytes places the stuffed bytes in the
//                    row's slot in HBM (sized for the worst case: no overflow path)
//   k_jpeg_pack      a workgroup per MCU row: the sum of the lengths before it places its segment and the marker after it in the batch's one contiguous image
#include "y7t_render.h"
#include "y7t_common.h"
#include <mutex>
#include <unordered_map>
#include <vector>

// ---------------------------------------------------------------------------------------------
// overlay
// ---------------------------------------------------------------------------------------------
enum { kTile = 32, kChunk = 256 };

// rank of this thread among the threads of the workgroup (256) with `flag`, in thread order, and their number; wcnt: 4 ints of LDS.  Two barriers.
__device__ inline int wg_rank(bool flag, int* wcnt, int* total) {
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();      // (the previous round's readers are done with wcnt)
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; ++w) { const int c = wcnt[w]; before += w < wave ? c : 0; all += c; }
    *total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(256) k_render_draw(const unsigned char* __restrict__ in, int H, int W, const Y7TRenderTrack* __restrict__ tracks,
                                                     const int* __restrict__ offsets, unsigned char* __restrict__ out) {
    __shared__ Y7TRenderPrim list[kChunk];
    __shared__ int wcnt[4];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
    const int tx1 = min(tx0 + kTile, W) - 1, ty1 = min(ty0 + kTile, H) - 1;
    const int py = ty0 + (tid >> 3), px0 = tx0 + (tid & 7) * 4;
    const bool row_in = py < H;
    const bool wide = (W & 3) == 0;      // (then px0 + 3 < W whenever px0 < W, and the 12 bytes of the 4 pixels are dword aligned)
    const size_t base = (((size_t)b * H + (row_in ? py : 0)) * W + px0) * 3;
    unsigned char c[4][3];
    const int npx = !row_in ? 0 : (px0 + 4 <= W ? 4 : (px0 < W ? W - px0 : 0));
    if (npx == 4 && wide) {
        const unsigned* p = (const unsigned*)(in + base);
        const unsigned v[3] = {p[0], p[1], p[2]};
        for (int i = 0; i < 12; ++i) c[i / 3][i % 3] = (unsigned char)(v[i >> 2] >> (8 * (i & 3)));
    } else {
        for (int i = 0; i < npx; ++i)
            for (int k = 0; k < 3; ++k) c[i][k] = in[base + 3 * i + k];
    }
    const int lo = offsets[b], hi = offsets[b + 1];
    for (int c0 = lo; c0 < hi; c0 += kChunk) {      // (lo and hi are the workgroup's: every barrier is reached by all of it)
        Y7TRenderPrim p;
        bool touch = false;
        if (c0 + tid < hi) {
            p = y7t_render_prim(tracks[c0 + tid]);
            touch = y7t_render_touches(p, tx0, ty0, tx1, ty1);
        }
        int n;
        const int r = wg_rank(touch, wcnt, &n);
        if (touch) list[r] = p;
        __syncthreads();
        for (int i = 0; i < npx; ++i)
            for (int k = n - 1; k >= 0; --k)
                if (y7t_render_hit(list[k], px0 + i, py, c[i])) break;
    }
    if (npx == 4 && wide) {
        unsigned v[3] = {0, 0, 0};
        for (int i = 0; i < 12; ++i) v[i >> 2] |= (unsigned)c[i / 3][i % 3] << (8 * (i & 3));
        unsigned* p = (unsigned*)(out + base);
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    } else {
        for (int i = 0; i < npx; ++i)
            for (int k = 0; k < 3; ++k) out[base + 3 * i + k] = c[i][k];
    }
}

extern "C" int y7t_render_draw(const uint8_t* frames, int B, int H, int W, const void* tracks, const int* offsets, uint8_t* out, y7t_stream stream) {
    Y7T_ARG_CHECK(B >= 0 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535);
    if (B == 0) return 0;
    Y7T_ARG_CHECK(frames && out && offsets && frames != out && B <= 65535);
    Y7T_ARG_CHECK(((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)tracks & 3) == 0);
    static_assert(sizeof(Y7TRenderTrack) == 48, "the packed track row of include/y7t.h");
    hipLaunchKernelGGL(k_render_draw, dim3((W + kTile - 1) / kTile, (H + kTile - 1) / kTile, B), dim3(256), 0, (hipStream_t)stream, frames, H, W,
                       (const Y7TRenderTrack*)tracks, offsets, out);
    Y7T_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// JPEG
// ---------------------------------------------------------------------------------------------
enum { kBlkThreads = 192, kStripCols = 512, kPitchW = (kStripCols * 3 + 8) / 4, kEntBlocks = 256, kEntWords = kEntBlocks * Y7T_JPEG_BLOCK_BYTES / 4 + 4 };

// the strip's pixels as the LDS holds them: row r at r * kPitchW words, its first pixel `shift` bytes in (the dwords were loaded from aligned addresses)
struct LdsPx {
    const unsigned char* lds;
    int s0, dshift, ncols, nrows;      // the first row's shift, the shift's step a row (W * 3 mod 4), the columns and rows of the frame inside the strip
    __device__ unsigned operator()(int x, int y) const {
        x = x < ncols ? x : ncols - 1;
        y = y < nrows ? y : nrows - 1;
        const unsigned char* p = lds + y * (kPitchW * 4) + ((s0 + y * dshift) & 3) + 3 * x;
        return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
    }
};

__global__ void __launch_bounds__(kBlkThreads) k_jpeg_blocks(const unsigned char* __restrict__ frames, size_t total_bytes, Y7TJpegGeom g, const Y7TJpegTables* __restrict__ tab,
                                                             short* __restrict__ coef, unsigned* __restrict__ meta) {
    __shared__ unsigned lds[16 * kPitchW];
    const int tid = threadIdx.x, b = blockIdx.z, mrow = blockIdx.y;
    const int mpw = kStripCols / g.mw;      // MCUs of a workgroup
    const int m0 = blockIdx.x * mpw, x0 = m0 * g.mw, y0 = mrow * g.mh;
    const int ncols = min((int)kStripCols, g.W - x0), nrows = min(g.mh, g.H - y0);
    const size_t row0 = (((size_t)b * g.H + y0) * g.W + x0) * 3, rstep = (size_t)g.W * 3;
    const int ndw = (3 + ncols * 3 + 3) / 4;      // (<= kPitchW: a row's bytes from the aligned address below its first)
    for (int e = tid; e < nrows * ndw; e += kBlkThreads) {
        const int r = e / ndw, k = e - r * ndw;
        const size_t start = row0 + r * rstep, a = (start & ~(size_t)3) + 4 * (size_t)k;
        unsigned v = 0;
        if (a + 4 <= total_bytes) v = *(const unsigned*)(frames + a);
        else for (int i = 0; i < 4; ++i) if (a + i < total_bytes) v |= (unsigned)frames[a + i] << (8 * i);      // (the last dword of the batch, when it is not whole)
        lds[r * kPitchW + k] = v;
    }
    __syncthreads();
    const int m = m0 + tid / g.bpm, k = tid % g.bpm;
    if (tid >= mpw * g.bpm || m >= g.mcols) return;
    const LdsPx px = {(const unsigned char*)lds, (int)(row0 & 3), (int)(rstep & 3), ncols, nrows};
    const int comp = y7t_jpeg_block_comp(g.sub, k);
    const bool avg = g.sub == Y7T_JPEG_420 && comp > 0;
    const int bx = (m - m0) * g.mw + ((g.sub == Y7T_JPEG_420 && comp == 0) ? (k & 1) * 8 : 0), by = (g.sub == Y7T_JPEG_420 && comp == 0) ? (k >> 1) * 8 : 0;
    short zz[64];
    int last, bits;
    y7t_jpeg_block(px, comp, bx, by, avg, tab->q[comp ? 1 : 0], tab->ac[comp ? 1 : 0], zz, &last, &bits);
    const size_t blk = ((size_t)b * g.mrows + mrow) * g.row_blocks + (size_t)m * g.bpm + k;
    int4* o = (int4*)(coef + blk * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int4 v;
        v.x = (zz[8 * i] & 0xffff) | (int)((unsigned)zz[8 * i + 1] << 16); v.y = (zz[8 * i + 2] & 0xffff) | (int)((unsigned)zz[8 * i + 3] << 16);
        v.z = (zz[8 * i + 4] & 0xffff) | (int)((unsigned)zz[8 * i + 5] << 16); v.w = (zz[8 * i + 6] & 0xffff) | (int)((unsigned)zz[8 * i + 7] << 16);
        o[i] = v;
    }
    meta[blk] = (unsigned)last | (unsigned)bits << 8;
}

__global__ void __launch_bounds__(256) k_jpeg_entropy(Y7TJpegGeom g, const Y7TJpegTables* __restrict__ tab, const short* __restrict__ coef, const unsigned* __restrict__ meta,
                                                      unsigned char* __restrict__ slots, size_t slot_bytes, int* __restrict__ seglen) {
    __shared__ unsigned buf[kEntWords];
    __shared__ int sc[256];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, mrow = blockIdx.x, b = blockIdx.y;
    const size_t seg = (size_t)b * g.mrows + mrow, blk0 = seg * g.row_blocks;
    unsigned char* slot = slots + seg * slot_bytes;
    int carry_bits = 0;
    unsigned carry_word = 0;
    size_t outpos = 0;
    for (int c0 = 0; c0 < g.row_blocks; c0 += kEntBlocks) {      // (the trip count is the workgroup's)
        const int nb = min((int)kEntBlocks, g.row_blocks - c0), j = c0 + tid;
        const bool act = tid < nb, final = c0 + kEntBlocks >= g.row_blocks;
        int last = 0, diff = 0, bits = 0, cls = 0;
        if (act) {
            const unsigned mt = meta[blk0 + j];
            const int k = j % g.bpm, back = y7t_jpeg_block_prev(g.sub, k);
            cls = y7t_jpeg_block_comp(g.sub, k) ? 1 : 0;
            last = (int)(mt & 63);
            const bool has = back == 1 || j >= g.bpm;      // (the row's first MCU predicts from 0; Y1 .. Y3 of 4:2:0 from the block before them)
            diff = (int)coef[(blk0 + j) * 64] - (has ? (int)coef[(blk0 + j - back) * 64] : 0);
            bits = (int)(mt >> 8) + y7t_jpeg_dc_bits(diff, tab->dc[cls]);
        }
        sc[tid] = bits;
        __syncthreads();
        for (int w = 1; w < 256; w <<= 1) {
            const int v = tid >= w ? sc[tid - w] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int start = carry_bits + sc[tid] - bits;
        int end = carry_bits + sc[255];
        const int pad = final ? (8 - (end & 7)) & 7 : 0;      // the row's last byte is filled with 1-bits
        const int pad_at = end;
        end += pad;
        for (int w = tid; w <= (end >> 5) && w < kEntWords; w += 256) buf[w] = w == 0 ? carry_word : 0u;
        __syncthreads();
        if (act) {
            Y7TJpegSink s = {buf, (unsigned)start, 0u};
            y7t_jpeg_emit_block(s, coef + (blk0 + j) * 64, last, diff, tab->dc[cls], tab->ac[cls]);
            y7t_jpeg_flush(s);
        }
        if (tid == 0 && pad) {
            Y7TJpegSink s = {buf, (unsigned)pad_at, 0u};
            y7t_jpeg_put(s, (1u << pad) - 1u, pad);
            y7t_jpeg_flush(s);
        }
        __syncthreads();
        const int nbytes = end >> 3;
        for (int base = 0; base < nbytes; base += 256) {
            const int i = base + tid;
            const bool valid = i < nbytes;
            const unsigned v = valid ? (buf[i >> 2] >> (24 - 8 * (i & 3))) & 255u : 0u;
            int nff;
            const int before = wg_rank(valid && v == 255u, wcnt, &nff);
            if (valid) {
                slot[outpos + i - base + before] = (unsigned char)v;
                if (v == 255u) slot[outpos + i - base + before + 1] = 0;
            }
            outpos += min(256, nbytes - base) + nff;
        }
        carry_bits = end & 7;
        carry_word = carry_bits ? (buf[nbytes >> 2] >> (24 - 8 * (nbytes & 3)) & 255u) << 24 : 0u;
        __syncthreads();      // (the buffer is read to the end before the next chunk clears it)
    }
    if (tid == 0) seglen[seg] = (int)outpos;
}

__global__ void __launch_bounds__(256) k_jpeg_pack(Y7TJpegGeom g, const unsigned char* __restrict__ header, int hdr_len, const unsigned char* __restrict__ slots,
                                                   size_t slot_bytes, const int* __restrict__ seglen, unsigned char* __restrict__ out, int* __restrict__ lens) {
    __shared__ long long red[256];
    const int tid = threadIdx.x, mrow = blockIdx.x, b = blockIdx.y;
    const int seg = b * g.mrows + mrow;
    long long s = 0;
    for (int i = tid; i < seg; i += 256) s += seglen[i];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const int n = seglen[seg];
    // the frames before this one: header, segments, a marker after every segment (RSTm between the rows, EOI after the last)
    const size_t at = (size_t)red[0] + (size_t)b * ((size_t)hdr_len + 2 * (size_t)g.mrows) + (size_t)hdr_len + 2 * (size_t)mrow;
    if (mrow == 0) for (int i = tid; i < hdr_len; i += 256) out[at - hdr_len + i] = header[i];
    const unsigned char* src = slots + (size_t)seg * slot_bytes;
    unsigned char* dst = out + at;
    const int head = min(n, (int)((4 - ((uintptr_t)dst & 3)) & 3)), ndw = (n - head) >> 2;
    if (tid < head) dst[tid] = src[tid];
    for (int d = tid; d < ndw; d += 256) {
        const unsigned char* p = src + head + 4 * d;
        *(unsigned*)(dst + head + 4 * d) = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
    }
    for (int i = head + 4 * ndw + tid; i < n; i += 256) dst[i] = src[i];
    if (tid == 0) {
        const bool lastrow = mrow == g.mrows - 1;
        dst[n] = 0xFF;
        dst[n + 1] = (unsigned char)(lastrow ? 0xD9 : 0xD0 + (mrow & 7));
        if (lastrow) lens[b + 1] = (int)(at + n + 2);
        if (seg == 0) lens[0] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
struct JpegLayout { size_t tab, header, coef, meta, seglen, slots, total, out; };
struct JpegInfo { Y7TJpegGeom g; int quality, max_batch, hdr_len; JpegLayout L; std::vector<unsigned char> staging; };
static std::mutex g_jpeg_mu;
static std::unordered_map<const void*, JpegInfo> g_jpegs;

static bool jpeg_caps_ok(int H, int W, int sub, int max_batch) {
    return H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (sub == Y7T_JPEG_420 || sub == Y7T_JPEG_444) && max_batch >= 1 && max_batch <= 65535;
}
static bool jpeg_layout(int H, int W, int sub, int max_batch, JpegLayout* L) {
    if (!jpeg_caps_ok(H, W, sub, max_batch)) return false;
    const Y7TJpegGeom g = y7t_jpeg_geom(H, W, sub);
    const size_t segs = (size_t)max_batch * g.mrows, blocks = segs * g.row_blocks;
    size_t o = 256;
    L->tab = o; o = al256(o + sizeof(Y7TJpegTables));
    L->header = o; o = al256(o + Y7T_JPEG_HEADER_MAX);
    L->coef = o; o = al256(o + blocks * 128);
    L->meta = o; o = al256(o + blocks * 4);
    L->seglen = o; o = al256(o + segs * 4);
    L->slots = o; o = al256(o + segs * y7t_jpeg_slot_bytes(g));
    L->total = o;
    L->out = al256((size_t)max_batch * y7t_jpeg_file_max(g));
    return L->out < ((size_t)1 << 31);      // (the offsets of the batch's image are int32)
}

extern "C" size_t y7t_jpeg_bytes(int H, int W, int subsampling, int max_batch, size_t* out_bytes) {
    JpegLayout L;
    if (!jpeg_layout(H, W, subsampling, max_batch, &L)) return 0;
    if (out_bytes) *out_bytes = L.out;
    return L.total;
}

extern "C" int y7t_jpeg_init(void* obj, size_t bytes, int H, int W, int quality, int subsampling, int max_batch, y7t_stream stream) {
    Y7T_ARG_CHECK(obj && ((uintptr_t)obj & 255) == 0);
    Y7T_ARG_CHECK(quality >= 1 && quality <= 100);
    JpegInfo info;
    Y7T_ARG_CHECK(jpeg_layout(H, W, subsampling, max_batch, &info.L));
    Y7T_ARG_CHECK(bytes >= info.L.total);
    info.g = y7t_jpeg_geom(H, W, subsampling);
    info.quality = quality; info.max_batch = max_batch;
    info.staging.assign(info.L.coef, 0);      // the tables and the header, as they lie in the object
    Y7TJpegTables* t = (Y7TJpegTables*)(info.staging.data() + info.L.tab);
    y7t_jpeg_make_tables(quality, t);
    info.hdr_len = y7t_jpeg_header(info.g, *t, info.staging.data() + info.L.header);
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    JpegInfo& kept = g_jpegs[obj] = std::move(info);      // (the staging bytes outlive the copy)
    Y7T_HIP_CHECK(hipMemcpyAsync(obj, kept.staging.data(), kept.L.coef, hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int y7t_jpeg_release(void* obj) {
    std::lock_guard<std::mutex> l(g_jpeg_mu);
    g_jpegs.erase(obj);
    return 0;
}

extern "C" int y7t_jpeg_encode(void* obj, const uint8_t* frames, int B, uint8_t* out, size_t out_bytes, int* lens, y7t_stream stream) {
    Y7TJpegGeom g;
    JpegLayout L;
    int hdr_len, max_batch;
    {
        std::lock_guard<std::mutex> l(g_jpeg_mu);
        auto it = g_jpegs.find(obj);
        if (it == g_jpegs.end()) { y7t_set_error("this address holds no JPEG encoder (y7t_jpeg_init)"); return Y7T_E_STATE; }
        g = it->second.g; L = it->second.L; hdr_len = it->second.hdr_len; max_batch = it->second.max_batch;
    }
    Y7T_ARG_CHECK(B >= 0 && lens);
    if (B > max_batch) { y7t_set_error("y7t_jpeg_encode: %d frames exceed this encoder's capacity (max_batch = %d)", B, max_batch); return Y7T_E_CAPACITY; }
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) { Y7T_HIP_CHECK(hipMemsetAsync(lens, 0, 4, st)); return 0; }
    Y7T_ARG_CHECK(frames && out && ((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 3) == 0);
    Y7T_ARG_CHECK(out_bytes >= (size_t)B * y7t_jpeg_file_max(g));
    char* base = (char*)obj;
    const Y7TJpegTables* tab = (const Y7TJpegTables*)(base + L.tab);
    short* coef = (short*)(base + L.coef);
    unsigned* meta = (unsigned*)(base + L.meta);
    int* seglen = (int*)(base + L.seglen);
    unsigned char* slots = (unsigned char*)(base + L.slots);
    const size_t slot_bytes = y7t_jpeg_slot_bytes(g);
    const int mpw = kStripCols / g.mw;
    hipLaunchKernelGGL(k_jpeg_blocks, dim3((g.mcols + mpw - 1) / mpw, g.mrows, B), dim3(kBlkThreads), 0, st, frames, (size_t)B * g.H * g.W * 3, g, tab, coef, meta);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jpeg_entropy, dim3(g.mrows, B), dim3(256), 0, st, g, tab, coef, meta, slots, slot_bytes, seglen);
    Y7T_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jpeg_pack, dim3(g.mrows, B), dim3(256), 0, st, g, (const unsigned char*)(base + L.header), hdr_len, slots, slot_bytes, seglen, out, lens);
    Y7T_LAUNCH_CHECK();
    return 0;
}
