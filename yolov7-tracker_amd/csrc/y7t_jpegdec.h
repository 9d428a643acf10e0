// y7t_jpegdec.h -- the arithmetic of the baseline JPEG decoder, stated once for the device kernels (csrc/y7t_jpegdec.hip) and for the host build the tests compare
// them with (tests/_hostsim/y7t_hostsim_jpegdec.cpp).  DESIGN.md section 4 "JPEG decoding" is the specification and tests/jpegdec_np.py its NumPy restatement.
// Everything is integer arithmetic.  Every function works on what it is given and is harmless on any input: a read of the file goes through a reader that clamps
// the index to the file, the zig-zag index stays below 64, a table index below 256; sums and products that a crafted stream could drive out of 32 bits wrap (they
// are formed as unsigned), which no well-formed stream reaches.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define Y7T_JHD __host__ __device__
#else
#define Y7T_JHD
#endif

// sampling (include/y7t.h: Y7T_JPEGDEC_*)
#define Y7T_JD_444 0
#define Y7T_JD_422 1
#define Y7T_JD_420 2
#define Y7T_JD_GRAY 3
// bits of a file's status word (include/y7t.h)
#define Y7T_JD_E_CODE 1       /* a bit pattern that is no code of its table, or a symbol baseline coding does not have */
#define Y7T_JD_E_TRUNC 2      /* the scan ended, or a marker stood, inside an MCU */
#define Y7T_JD_E_COUNT 4      /* the scan held more or fewer blocks than the frame has */
#define Y7T_JD_E_RANGE 8      /* a run of zeros led past coefficient 63 */
#define Y7T_JD_E_RESTART 16   /* a restart marker where the restart interval puts none, or none where it puts one */
#define Y7T_JD_SUBSEQ_MIN 16
#define Y7T_JD_SUBSEQ_MAX 4096
#define Y7T_JD_LANES 256      /* subsequences of a workgroup's run */
#define Y7T_JD_MAX_FILE (1u << 28)

// the per-file record the host parser writes (include/y7t.h: y7t_jpegdec_desc, 80 bytes); offsets other than file_off count from the file's first byte
struct Y7TJdDesc {
    uint32_t file_off, file_len;      // the file inside the batch's buffer
    uint32_t scan_off, scan_len;      // the entropy-coded bytes after the SOS header (up to the last EOI, or the end of the file)
    uint32_t restart_interval;        // MCUs; 0: none
    uint32_t dqt_off[4];              // by table id: the table's 64 bytes (zig-zag order); 0: not defined
    uint32_t dc_off[4], ac_off[4];    // by table id: BITS (16 bytes) with HUFFVAL after them; 0: not defined
    uint8_t tq[4], td[4], ta[4];      // by component: its table ids
};

struct Y7TJdGeom { int H, W, comps, hs, vs, mw, mh, mcols, mrows, bpm, nblocks, dw, dh; };
Y7T_JHD inline Y7TJdGeom y7t_jd_geom(int H, int W, int sampling) {
    Y7TJdGeom g;
    g.H = H; g.W = W;
    g.comps = sampling == Y7T_JD_GRAY ? 1 : 3;
    g.hs = (sampling == Y7T_JD_422 || sampling == Y7T_JD_420) ? 2 : 1;
    g.vs = sampling == Y7T_JD_420 ? 2 : 1;
    g.mw = 8 * g.hs; g.mh = 8 * g.vs;
    g.mcols = (W + g.mw - 1) / g.mw; g.mrows = (H + g.mh - 1) / g.mh;
    g.bpm = g.comps == 1 ? 1 : g.hs * g.vs + 2;
    g.nblocks = g.mcols * g.mrows * g.bpm;
    g.dw = (W + g.hs - 1) / g.hs; g.dh = (H + g.vs - 1) / g.vs;      // the chroma components' real extent
    return g;
}
// block k of an MCU -> its component
Y7T_JHD inline int y7t_jd_block_comp(const Y7TJdGeom& g, int k) { const int nl = g.comps == 1 ? 1 : g.hs * g.vs; return k < nl ? 0 : k - nl + 1; }
// block (bx, by) of component c's block grid -> its index in scan order
Y7T_JHD inline int y7t_jd_block_index(const Y7TJdGeom& g, int c, int bx, int by) {
    if (c == 0) return ((by / g.vs) * g.mcols + bx / g.hs) * g.bpm + (by % g.vs) * g.hs + bx % g.hs;
    return (by * g.mcols + bx) * g.bpm + g.hs * g.vs + c - 1;
}

Y7T_JHD constexpr int y7t_jd_zig(int k) {      // zig-zag position k -> natural index
    constexpr unsigned char z[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k & 63];
}

// a reader of a byte range: every index is clamped to the range (an empty range reads 0)
struct Y7TJdBytes {
    const unsigned char* p;
    uint32_t n;
    Y7T_JHD unsigned operator()(uint32_t i) const { return n ? p[i < n ? i : n - 1] : 0u; }
};

// ---------------------------------------------------------------------------------------------
// Huffman tables (Annex C / F.2.2.3): code lengths 1 .. 16, lim[L] the first 16-bit left-aligned pattern that is NOT a code of length <= L
// ---------------------------------------------------------------------------------------------
struct Y7TJdHuff { int lim[17], base[17]; unsigned char vals[256]; };
template <class Rd>
Y7T_JHD inline void y7t_jd_build_huff(const Rd& file, uint32_t off, Y7TJdHuff* h) {
    unsigned code = 0;
    int k = 0;
    h->lim[0] = 0; h->base[0] = 0;
    for (int L = 1; L <= 16; ++L) {
        const int n = off ? (int)file(off + L - 1) : 0;
        h->base[L] = k - (int)code;
        code += (unsigned)n; k += n;
        const unsigned lim = code << (16 - L);
        h->lim[L] = (int)(lim > 65536u ? 65536u : lim);      // (a table with more codes than its lengths hold: a malformed file)
        code <<= 1;
        if (code > 131072u) code = 131072u;
    }
    if (k > 256) k = 256;
    for (int i = 0; i < 256; ++i) h->vals[i] = (off && i < k) ? (unsigned char)file(off + 16 + i) : 0;
}
// the 16 bits that follow -> symbol and length; no code: length 17
Y7T_JHD inline int y7t_jd_lookup(const Y7TJdHuff& h, int bits16, int* len) {
    for (int L = 1; L <= 16; ++L)
        if (bits16 < h.lim[L]) { *len = L; return h.vals[(h.base[L] + (bits16 >> (16 - L))) & 255]; }
    *len = 17;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// entropy decoding of a subsequence
// ---------------------------------------------------------------------------------------------
// A decoder's state between two symbols: the bit of the scan (stuffed bytes: 0xFF00 counts 16 bits) at which the next symbol starts, the block inside the MCU and
// the zig-zag index; after the last bit of a byte the position is the next byte's first bit even where that byte is a stuffed zero (it is skipped when bits are
// needed).  Packed: p | b << 32 | z << 40.
typedef unsigned long long y7t_jd_state;
Y7T_JHD inline y7t_jd_state y7t_jd_pack(uint32_t p, int b, int z) { return (y7t_jd_state)p | (y7t_jd_state)(b & 15) << 32 | (y7t_jd_state)(z & 63) << 40; }
Y7T_JHD inline uint32_t y7t_jd_state_p(y7t_jd_state s) { return (uint32_t)s; }
Y7T_JHD inline int y7t_jd_state_b(y7t_jd_state s) { return (int)(s >> 32) & 15; }
Y7T_JHD inline int y7t_jd_state_z(y7t_jd_state s) { return (int)(s >> 40) & 63; }

// 40 bits of data from stuffed byte i on: stuffed zeros skipped (bit k of skips: one stood before data byte k), zeros from a marker or the scan's end on
// (avail: the bits before it, 40 if none; mark: the stuffed index of the marker's 0xFF, or the scan's length)
// Every byte is read into a named value before it is tested (keep it so: the device compiler is sensitive to the form of this loop).
struct Y7TJdWin { unsigned long long w; int avail; unsigned skips; uint32_t mark; };
template <class Rd>
Y7T_JHD inline Y7TJdWin y7t_jd_window(const Rd& scan, uint32_t scan_len, uint32_t i) {
    Y7TJdWin r;
    r.w = 0; r.avail = 40; r.skips = 0; r.mark = scan_len;
    uint32_t j = i;
    bool open = true;
    for (int k = 0; k < 5; ++k) {
        unsigned c = 0;
        if (open) {
            const unsigned here = j < scan_len ? scan(j) : 1u, before = j > 0 ? scan(j - 1) : 0u;
            if (here == 0u && before == 0xFFu) { ++j; r.skips |= 1u << k; }
            if (j >= scan_len) { open = false; r.avail = 8 * k; r.mark = scan_len; }
            else {
                const unsigned cur = scan(j), next = j + 1 < scan_len ? scan(j + 1) : 0xD9u;
                if (cur == 0xFFu && next != 0u) { open = false; r.avail = 8 * k; r.mark = j; }
                else { c = cur; ++j; }
            }
        }
        r.w = r.w << 8 | c;
    }
    return r;
}
// the position t bits (t <= 39) after the first bit of the window that starts at stuffed byte i
Y7T_JHD inline uint32_t y7t_jd_advance(const Y7TJdWin& win, uint32_t i, int t) {
    const int k = t >> 3, r = t & 7;
    const unsigned m = r ? (1u << (k + 1)) - 1u : (1u << k) - 1u;
    unsigned s = win.skips & m, n = 0;
    for (; s; s &= s - 1) ++n;
    return 8u * (i + (uint32_t)k + n) + (uint32_t)r;
}
// at an MCU boundary: do only 1-bits (or nothing) stand before the next byte boundary, and RSTm behind it?  -> the position after the marker, or 0
template <class Rd>
Y7T_JHD inline uint32_t y7t_jd_at_restart(const Rd& scan, uint32_t scan_len, uint32_t p) {
    uint32_t i = (p + 7) >> 3;
    if (i + 2 >= scan_len) return 0;
    const int pad = (int)(8 * i - p);
    if (pad && (i == 0 || (scan(i - 1) & ((1u << pad) - 1u)) != (1u << pad) - 1u)) return 0;
    if (i > 0 && scan(i) == 0u && scan(i - 1) == 0xFFu) ++i;      // (the byte before the marker was 0xFF: its stuffed zero)
    if (scan(i) != 0xFFu || (scan(i + 1) & 0xF8u) != 0xD0u) return 0;
    return 8 * (i + 2);
}

// One lane: the symbols that start in [entry, end_bit) of one scan, from the state `entry`.  -> the state at which the first symbol at or after end_bit starts (the
// scan's end: 8 * scan_len, b = z = 0); *count: the blocks completed; *flags: Y7T_JD_E_*.  coef != nullptr: the coefficients are stored (natural order, int16, the DC
// as the difference the stream holds) from block `first` on, a block index at or above g.nblocks dropped.
template <class Rd>
Y7T_JHD inline y7t_jd_state y7t_jd_lane(const Rd& scan, uint32_t scan_len, const Y7TJdGeom& g, const Y7TJdHuff* dc, const Y7TJdHuff* ac, uint32_t ri,
                                         y7t_jd_state entry, uint32_t end_bit, short* coef, int first, int* count, int* flags) {
    uint32_t p = y7t_jd_state_p(entry);
    int b = y7t_jd_state_b(entry), z = y7t_jd_state_z(entry), n = 0, fl = 0;
    if (b >= g.bpm) b = 0;
    const uint32_t total = 8u * scan_len;
    if (end_bit > total) end_bit = total;
    while (p < end_bit) {
        if (ri && b == 0 && z == 0) {
            const uint32_t q = y7t_jd_at_restart(scan, scan_len, p);
            if (q) { p = q; continue; }
            if (coef) {      // (the pass that knows its block index) an MCU starts right behind RSTm exactly where the restart interval says so
                const bool behind = (p & 7) == 0 && p >= 16 && scan((p >> 3) - 2) == 0xFFu && (scan((p >> 3) - 1) & 0xF8u) == 0xD0u;
                const bool due = first + n > 0 && (uint32_t)(first + n) % (ri * (uint32_t)g.bpm) == 0;
                if (first + n < g.nblocks && behind != due) fl |= Y7T_JD_E_RESTART;
            }
        }
        const uint32_t i = p >> 3;
        const int o = (int)(p & 7);
        const Y7TJdWin win = y7t_jd_window(scan, scan_len, i);
        const int c = y7t_jd_block_comp(g, b);
        int len;
        const int sym = y7t_jd_lookup(z == 0 ? dc[c] : ac[c], (int)(win.w >> (24 - o)) & 0xFFFF, &len);
        int use, size, run = 0, bad = 0;      // (bad: counted only once the symbol is known to lie before the scan's end)
        bool eob = false;
        if (len > 16) { bad = Y7T_JD_E_CODE; len = 16; }
        if (z == 0) { size = sym; if (size > 11) { size = 11; bad = Y7T_JD_E_CODE; } }
        else {
            size = sym & 15; run = sym >> 4;
            if (size > 11) { size = 11; bad = Y7T_JD_E_CODE; }
            if (size == 0) { if (run == 15) run = 16; else { eob = true; if (run) bad = Y7T_JD_E_CODE; } }
        }
        use = len + size;
        if (o + use > win.avail) {      // the symbol runs into a marker or the scan's end
            if (b || z) fl |= Y7T_JD_E_TRUNC;
            if (win.mark + 1 < scan_len && (scan(win.mark + 1) & 0xF8u) == 0xD0u) { p = 8 * (win.mark + 2); b = 0; z = 0; continue; }      // RSTm: start over behind it
            p = total; b = 0; z = 0;
            break;
        }
        fl |= bad;
        int v = (int)(win.w >> (40 - o - use)) & ((1 << size) - 1);
        if (size && v < (1 << (size - 1))) v -= (1 << size) - 1;
        if (z == 0) {
            if (coef && first + n < g.nblocks) coef[(size_t)(first + n) * 64] = (short)v;
            z = 1;
        } else if (eob) z = 64;
        else {
            z += run;
            if (size) {
                if (z > 63) { fl |= Y7T_JD_E_RANGE; z = 63; }
                if (coef && first + n < g.nblocks) coef[(size_t)(first + n) * 64 + y7t_jd_zig(z)] = (short)v;
                ++z;
            } else if (z > 64) fl |= Y7T_JD_E_RANGE;
        }
        if (z >= 64) { z = 0; ++n; if (++b >= g.bpm) b = 0; }
        p = y7t_jd_advance(win, i, o + use);
    }
    *count = n; *flags = fl;
    return y7t_jd_pack(p, b, z);
}
// the state a lane assumes before it has seen its predecessor's
Y7T_JHD inline y7t_jd_state y7t_jd_assumed(uint32_t subseq, uint32_t subseq_bytes) { return y7t_jd_pack(8u * subseq * subseq_bytes, 0, 0); }

// ---------------------------------------------------------------------------------------------
// the DC values: a running sum per component in scan order, from 0 again after every restart interval.  One thread's share [m0, m1) of the MCUs in two steps:
// y7t_jd_dc_sum -> per component the sum of its differences since the last reset (and whether there was one), then, given the sums carried in, y7t_jd_dc_apply
// ---------------------------------------------------------------------------------------------
struct Y7TJdDcPart { unsigned sum[3]; int reset; };
Y7T_JHD inline Y7TJdDcPart y7t_jd_dc_join(const Y7TJdDcPart& a, const Y7TJdDcPart& b) {      // a's MCUs, then b's
    Y7TJdDcPart r;
    for (int c = 0; c < 3; ++c) r.sum[c] = b.reset ? b.sum[c] : a.sum[c] + b.sum[c];
    r.reset = a.reset | b.reset;
    return r;
}
Y7T_JHD inline Y7TJdDcPart y7t_jd_dc_walk(const Y7TJdGeom& g, uint32_t ri, short* coef, int m0, int m1, Y7TJdDcPart carry, bool store) {
    Y7TJdDcPart r = carry;
    if (!store) { r.sum[0] = r.sum[1] = r.sum[2] = 0; r.reset = 0; }
    for (int m = m0; m < m1; ++m) {
        if (ri && m % (int)ri == 0) { r.sum[0] = r.sum[1] = r.sum[2] = 0; r.reset = 1; }
        for (int k = 0; k < g.bpm; ++k) {
            const int c = y7t_jd_block_comp(g, k);
            short* d = coef + ((size_t)m * g.bpm + k) * 64;
            r.sum[c] += (unsigned)(int)*d;
            if (store) *d = (short)r.sum[c];
        }
    }
    return r;
}

// ---------------------------------------------------------------------------------------------
// inverse DCT: Loeffler, Ligtenberg and Moschytz, 13-bit constants, the inverse of y7t_jpeg_fdct (csrc/y7t_render.h)
// ---------------------------------------------------------------------------------------------
#define Y7T_JM(a, c) ((int)((unsigned)(a) * (unsigned)(c)))
#define Y7T_JA(a, b) ((int)((unsigned)(a) + (unsigned)(b)))
#define Y7T_JS(a, b) ((int)((unsigned)(a) - (unsigned)(b)))
Y7T_JHD inline void y7t_jd_idct_1d(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7, int sh) {
    const int z1 = Y7T_JM(Y7T_JA(d2, d6), 4433);
    const int t2 = Y7T_JA(z1, Y7T_JM(d6, -15137)), t3 = Y7T_JA(z1, Y7T_JM(d2, 6270));
    const int t0 = Y7T_JM(Y7T_JA(d0, d4), 8192), t1 = Y7T_JM(Y7T_JS(d0, d4), 8192);
    const int e0 = Y7T_JA(t0, t3), e3 = Y7T_JS(t0, t3), e1 = Y7T_JA(t1, t2), e2 = Y7T_JS(t1, t2);
    const int z5 = Y7T_JM(Y7T_JA(Y7T_JA(d7, d3), Y7T_JA(d5, d1)), 9633);
    const int y1 = Y7T_JM(Y7T_JA(d7, d1), -7373), y2 = Y7T_JM(Y7T_JA(d5, d3), -20995);
    const int y3 = Y7T_JA(Y7T_JM(Y7T_JA(d7, d3), -16069), z5), y4 = Y7T_JA(Y7T_JM(Y7T_JA(d5, d1), -3196), z5);
    const int o0 = Y7T_JA(Y7T_JM(d7, 2446), Y7T_JA(y1, y3)), o1 = Y7T_JA(Y7T_JM(d5, 16819), Y7T_JA(y2, y4));
    const int o2 = Y7T_JA(Y7T_JM(d3, 25172), Y7T_JA(y2, y3)), o3 = Y7T_JA(Y7T_JM(d1, 12299), Y7T_JA(y1, y4));
    const int rnd = 1 << (sh - 1);
    d0 = Y7T_JA(Y7T_JA(e0, o3), rnd) >> sh; d7 = Y7T_JA(Y7T_JS(e0, o3), rnd) >> sh;
    d1 = Y7T_JA(Y7T_JA(e1, o2), rnd) >> sh; d6 = Y7T_JA(Y7T_JS(e1, o2), rnd) >> sh;
    d2 = Y7T_JA(Y7T_JA(e2, o1), rnd) >> sh; d5 = Y7T_JA(Y7T_JS(e2, o1), rnd) >> sh;
    d3 = Y7T_JA(Y7T_JA(e3, o0), rnd) >> sh; d4 = Y7T_JA(Y7T_JS(e3, o0), rnd) >> sh;
}
// d: the dequantised coefficients, natural order -> the samples 0 .. 255
Y7T_JHD inline void y7t_jd_idct(int* d) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) y7t_jd_idct_1d(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c], 11);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 8; ++r) y7t_jd_idct_1d(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4], d[8 * r + 5], d[8 * r + 6], d[8 * r + 7], 18);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 64; ++i) { const int v = Y7T_JA(d[i], 128); d[i] = v < 0 ? 0 : (v > 255 ? 255 : v); }
}
// one block: coef (natural order) times the quantiser (q(k): the table's entry at zig-zag position k) -> 64 samples
template <class Q>
Y7T_JHD inline void y7t_jd_block(const short* coef, const Q& q, int* d) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 64; ++k) d[y7t_jd_zig(k)] = (int)coef[y7t_jd_zig(k)] * (int)q(k);
    y7t_jd_idct(d);
}

// ---------------------------------------------------------------------------------------------
// a pixel: chroma upsampling (libjpeg's "fancy" triangle filters) and YCbCr -> B, G, R.  Y(x, y) and C(c, x, y) (c = 1, 2; component coordinates) -> 0 .. 255
// ---------------------------------------------------------------------------------------------
Y7T_JHD inline int y7t_jd_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
template <class Cs>
Y7T_JHD inline int y7t_jd_chroma(const Y7TJdGeom& g, const Cs& C, int c, int x, int y) {
    if (g.hs == 1) return C(c, x, y);
    const int cx = x >> 1;
    if (g.vs == 1) {
        if (g.dw <= 2) return C(c, cx, y);
        const int p = C(c, cx, y);
        return (x & 1) ? (3 * p + C(c, y7t_jd_clampi(cx + 1, g.dw - 1), y) + 2) >> 2 : (3 * p + C(c, y7t_jd_clampi(cx - 1, g.dw - 1), y) + 1) >> 2;
    }
    const int cy = y >> 1;
    if (g.dw <= 2) return C(c, cx, cy);
    const int r1 = y7t_jd_clampi((y & 1) ? cy + 1 : cy - 1, g.dh - 1);
    const int xn = y7t_jd_clampi((x & 1) ? cx + 1 : cx - 1, g.dw - 1);
    const int s0 = 3 * C(c, cx, cy) + C(c, cx, r1), s1 = 3 * C(c, xn, cy) + C(c, xn, r1);
    return (3 * s0 + s1 + ((x & 1) ? 7 : 8)) >> 4;
}
template <class Ys, class Cs>
Y7T_JHD inline void y7t_jd_pixel(const Y7TJdGeom& g, const Ys& Y, const Cs& C, int x, int y, unsigned char* bgr) {
    const int yy = Y(x, y);
    if (g.comps == 1) { bgr[0] = bgr[1] = bgr[2] = (unsigned char)yy; return; }
    const int cb = y7t_jd_chroma(g, C, 1, x, y) - 128, cr = y7t_jd_chroma(g, C, 2, x, y) - 128;
    const int r = yy + ((91881 * cr + 32768) >> 16), gg = yy + ((-22554 * cb - 46802 * cr + 32768) >> 16), b = yy + ((116130 * cb + 32768) >> 16);
    bgr[0] = (unsigned char)y7t_jd_clampi(b, 255); bgr[1] = (unsigned char)y7t_jd_clampi(gg, 255); bgr[2] = (unsigned char)y7t_jd_clampi(r, 255);
}

// ---------------------------------------------------------------------------------------------
// the decoder object's memory (host only): per file nsub subsequence records and nruns run records, sized for max_file_bytes
// ---------------------------------------------------------------------------------------------
struct Y7TJdLayout { size_t rounds, iters, descs, entry, exit, count, first, run_exit, run_entry, run_round, run_iters, coef, total; uint32_t nsub, nruns; };
inline bool y7t_jd_layout(const Y7TJdGeom& g, int max_batch, size_t max_file_bytes, int subseq_bytes, int lanes, Y7TJdLayout* L) {
    if (lanes < 1 || max_batch < 1 || max_batch > 65535 || max_file_bytes < 1 || max_file_bytes > Y7T_JD_MAX_FILE) return false;
    if (subseq_bytes < Y7T_JD_SUBSEQ_MIN || subseq_bytes > Y7T_JD_SUBSEQ_MAX || (subseq_bytes & 3)) return false;
    L->nsub = (uint32_t)((max_file_bytes + subseq_bytes - 1) / subseq_bytes);
    L->nruns = (L->nsub + (uint32_t)lanes - 1) / (uint32_t)lanes;
    const size_t B = (size_t)max_batch, ns = B * L->nsub, nr = B * L->nruns;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 256;
    L->rounds = o; o = al(o + B * 4);
    L->iters = o; o = al(o + B * 4);
    L->descs = o; o = al(o + B * sizeof(Y7TJdDesc));
    L->entry = o; o = al(o + ns * 8);
    L->exit = o; o = al(o + ns * 8);
    L->count = o; o = al(o + ns * 4);
    L->first = o; o = al(o + ns * 4);
    L->run_exit = o; o = al(o + 2 * nr * 8);
    L->run_entry = o; o = al(o + nr * 8);
    L->run_round = o; o = al(o + nr * 4);
    L->run_iters = o; o = al(o + nr * 4);
    L->coef = o; o = al(o + B * (size_t)g.nblocks * 128);
    L->total = o;
    return true;
}
