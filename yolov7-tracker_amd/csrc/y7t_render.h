// y7t_render.h -- the arithmetic of the annotated-frame path, stated once for the device kernels (csrc/y7t_render.hip) and for the host build the tests compare them
// with (tests/_hostsim/y7t_hostsim_render.cpp): the overlay's geometry and the baseline JPEG encoder.  DESIGN.md section 4 "Rendering" is the specification and
// tests/render_np.py its NumPy restatement.  Everything that decides a pixel or a bit is integer arithmetic; the one floating-point step, a box's corners, is the
// float64 sum and truncation of the reference's Python expression.  No state, no allocation: every function works on what it is given.
#pragma once
#include <stdint.h>
#include <string.h>
#include "y7t_font.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define Y7T_RHD __host__ __device__
#else
#define Y7T_RHD
#endif

// ---------------------------------------------------------------------------------------------
// overlay
// ---------------------------------------------------------------------------------------------
#define Y7T_RENDER_LABEL 24
// one row of the packed track table (48 bytes): tlwh as the tracker reports it, the id the colour comes from, the label the host assembled
struct Y7TRenderTrack { float x, y, w, h; int id; int len; unsigned char label[Y7T_RENDER_LABEL]; };
// what a track draws: the rectangle's 1-pixel outline [xa, xb] x [ya, yb] (thickened by 1), the text origin (tx, ty) = the baseline's left end, the colour
struct Y7TRenderPrim { int xa, ya, xb, yb, tx, ty, len; unsigned char bgr[3], live; unsigned char label[Y7T_RENDER_LABEL]; };

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ static const unsigned char y7t_font_rows[Y7T_FONT_COUNT][Y7T_FONT_H] = Y7T_FONT_ROWS;
#else
static const unsigned char y7t_font_rows[Y7T_FONT_COUNT][Y7T_FONT_H] = Y7T_FONT_ROWS;
#endif

// int(v) of Python for a float64: toward zero; beyond +-2^30 the corner is clamped there (a frame is far smaller), NaN drops the track
Y7T_RHD inline int y7t_render_trunc(double v) { return v >= 1073741824.0 ? 1073741824 : (v <= -1073741824.0 ? -1073741824 : (int)v); }
Y7T_RHD inline int y7t_render_pymod255(long long v) { const long long m = v % 255; return (int)(m < 0 ? m + 255 : m); }

Y7T_RHD inline Y7TRenderPrim y7t_render_prim(const Y7TRenderTrack& t) {
    Y7TRenderPrim p;
    const double x = t.x, y = t.y, w = t.w, h = t.h;
    p.live = (x == x && y == y && w == w && h == h) ? 1 : 0;
    const int x1 = y7t_render_trunc(x), y1 = y7t_render_trunc(y), x2 = y7t_render_trunc(x + w), y2 = y7t_render_trunc(y + h);
    p.xa = x1 < x2 ? x1 : x2; p.xb = x1 < x2 ? x2 : x1;
    p.ya = y1 < y2 ? y1 : y2; p.yb = y1 < y2 ? y2 : y1;
    p.tx = x1; p.ty = y1;
    p.len = t.len < 0 ? 0 : (t.len > Y7T_RENDER_LABEL ? Y7T_RENDER_LABEL : t.len);
    const long long idx = 3LL * (long long)t.id;      // get_color: the tuple is handed to cv2 as (B, G, R)
    p.bgr[0] = (unsigned char)y7t_render_pymod255(37 * idx);
    p.bgr[1] = (unsigned char)y7t_render_pymod255(17 * idx);
    p.bgr[2] = (unsigned char)y7t_render_pymod255(29 * idx);
    for (int i = 0; i < Y7T_RENDER_LABEL; ++i) p.label[i] = i < p.len ? t.label[i] : 0;
    return p;
}

// does any primitive of p touch the pixel rectangle [x0, x1] x [y0, y1]?  (conservative: the text's whole cell row, the rectangle's ring)
Y7T_RHD inline bool y7t_render_touches(const Y7TRenderPrim& p, int x0, int y0, int x1, int y1) {
    if (!p.live) return false;
    const bool ring = p.xa - 1 <= x1 && p.xb + 1 >= x0 && p.ya - 1 <= y1 && p.yb + 1 >= y0 &&
                      !(x0 >= p.xa + 2 && x1 <= p.xb - 2 && y0 >= p.ya + 2 && y1 <= p.yb - 2);
    const int top = p.ty - Y7T_FONT_BASE;
    const bool text = p.len > 0 && p.tx <= x1 && p.tx + Y7T_FONT_W * p.len - 1 >= x0 && top <= y1 && top + Y7T_FONT_H - 1 >= y0;
    return ring || text;
}

// the pixel (px, py) under the two primitives of one track, the text (drawn second) first -> true and the colour when one of them covers it
Y7T_RHD inline bool y7t_render_hit(const Y7TRenderPrim& p, int px, int py, unsigned char* bgr) {
    if (!p.live) return false;
    const int dx = px - p.tx, dy = py - (p.ty - Y7T_FONT_BASE);
    if (dx >= 0 && dx < Y7T_FONT_W * p.len && dy >= 0 && dy < Y7T_FONT_H) {
        const int ch = (int)p.label[dx >> 3] - Y7T_FONT_FIRST;
        if (ch >= 0 && ch < Y7T_FONT_COUNT && (y7t_font_rows[ch][dy] & (0x80 >> (dx & 7)))) {
            bgr[0] = 255; bgr[1] = 164; bgr[2] = 0;
            return true;
        }
    }
    if (px >= p.xa - 1 && px <= p.xb + 1 && py >= p.ya - 1 && py <= p.yb + 1 &&
        !(px >= p.xa + 2 && px <= p.xb - 2 && py >= p.ya + 2 && py <= p.yb - 2)) {
        bgr[0] = p.bgr[0]; bgr[1] = p.bgr[1]; bgr[2] = p.bgr[2];
        return true;
    }
    return false;
}

// ---------------------------------------------------------------------------------------------
// baseline JPEG
// ---------------------------------------------------------------------------------------------
#define Y7T_JPEG_420 0
#define Y7T_JPEG_444 1
#define Y7T_JPEG_BLOCK_BYTES 216      /* >= the longest code of a block: 22 bits of DC and 63 x 26 of AC = 1660 bits = 207.5 bytes */
#define Y7T_JPEG_HEADER_MAX 1024

struct Y7TJpegHuff { unsigned short code[256]; unsigned char size[256]; };
// q: the two quantisation tables in natural (row-major) order; dc / ac [0] luminance, [1] chrominance
struct Y7TJpegTables { unsigned short q[2][64]; Y7TJpegHuff dc[2], ac[2]; };

Y7T_RHD constexpr int y7t_jpeg_zig(int k) {      // zigzag position k -> natural index
    constexpr unsigned char z[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k];
}

// component c (0 Y, 1 Cb, 2 Cr) of a pixel: 16-bit fixed point, round to nearest, clamped to 0 .. 255.  A tie goes up for Y and down for Cb and Cr (+ 32767):
// the saturated colours sit on chroma ties (yellow: Cb = 0.5), and down is the side from which a decoder returns them exactly
Y7T_RHD inline int y7t_jpeg_ycc(int r, int g, int b, int c) {
    int v;
    if (c == 0) v = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    else if (c == 1) v = ((-11059 * r - 21709 * g + 32768 * b + 32767) >> 16) + 128;
    else v = ((32768 * r - 27439 * g - 5329 * b + 32767) >> 16) + 128;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the accurate-integer forward DCT of Loeffler, Ligtenberg and Moschytz: 13-bit constants, 2 extra bits kept between the passes; d (natural order) -> 8 x its DCT
Y7T_RHD inline int y7t_jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
Y7T_RHD inline void y7t_jpeg_fdct_1d(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7, int pass) {
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
    const int sh = pass == 0 ? 11 : 15;      // CONST_BITS -+ PASS1_BITS
    if (pass == 0) { d0 = (e0 + e1) * 4; d4 = (e0 - e1) * 4; }
    else { d0 = y7t_jpeg_descale(e0 + e1, 2); d4 = y7t_jpeg_descale(e0 - e1, 2); }
    const int z = (e2 + e3) * 4433;
    d2 = y7t_jpeg_descale(z + e3 * 6270, sh);
    d6 = y7t_jpeg_descale(z - e2 * 15137, sh);
    const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    d7 = y7t_jpeg_descale(t4 * 2446 + z1 + z3, sh);
    d5 = y7t_jpeg_descale(t5 * 16819 + z2 + z4, sh);
    d3 = y7t_jpeg_descale(t6 * 25172 + z2 + z3, sh);
    d1 = y7t_jpeg_descale(t7 * 12299 + z1 + z4, sh);
}
Y7T_RHD inline void y7t_jpeg_fdct(int* d) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 8; ++r) y7t_jpeg_fdct_1d(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4], d[8 * r + 5], d[8 * r + 6], d[8 * r + 7], 0);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) y7t_jpeg_fdct_1d(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c], 1);
}

// a coefficient of y7t_jpeg_fdct (8 x the DCT) over its quantiser: integer division, half away from zero; the DC within -1024 .. 1023, the rest within +-1023
Y7T_RHD inline int y7t_jpeg_quant(int v, int q, bool dc) {
    const int q8 = q * 8, a = v < 0 ? -v : v;
    int m = (a + (q8 >> 1)) / q8;
    if (m > 1023) m = (dc && v < 0 && m >= 1024) ? 1024 : 1023;
    return v < 0 ? -m : m;
}

Y7T_RHD inline int y7t_jpeg_nbits(int a) { int n = 0; while (a) { ++n; a >>= 1; } return n; }      // a >= 0: the category of a magnitude

// One block.  px(x, y) -> the pixel as b | g << 8 | r << 16, x and y in the caller's frame of reference (it replicates the frame's last column and row beyond them);
// (x0, y0): the block's first pixel; avg: a chroma block of 4:2:0, every sample the mean of 2 x 2 pixels from (x0, y0) on.  -> zz[64] in zigzag order, the index
// of the last non-zero coefficient (0 if none after the DC) and the bits its AC code takes.
template <class Px>
Y7T_RHD inline void y7t_jpeg_block(const Px& px, int comp, int x0, int y0, bool avg, const unsigned short* q, const Y7TJpegHuff& ac, short* zz, int* last_out, int* ac_bits_out) {
    int d[64];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 64; ++i) {
        const int x = i & 7, y = i >> 3;
        int v;
        if (!avg) {
            const unsigned p = px(x0 + x, y0 + y);
            v = y7t_jpeg_ycc((int)(p >> 16 & 255), (int)(p >> 8 & 255), (int)(p & 255), comp);
        } else {
            int s = 2;
            for (int j = 0; j < 4; ++j) {
                const unsigned p = px(x0 + 2 * x + (j & 1), y0 + 2 * y + (j >> 1));
                s += y7t_jpeg_ycc((int)(p >> 16 & 255), (int)(p >> 8 & 255), (int)(p & 255), comp);
            }
            v = s >> 2;
        }
        d[i] = v - 128;
    }
    y7t_jpeg_fdct(d);
    int last = 0, bits = 0, run = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 64; ++k) {
        const int n = y7t_jpeg_zig(k);
        const int v = y7t_jpeg_quant(d[n], q[n], k == 0);
        zz[k] = (short)v;
        if (k == 0) continue;
        if (v == 0) { ++run; continue; }
        last = k;
        bits += (run >> 4) * ac.size[0xF0];
        const int cat = y7t_jpeg_nbits(v < 0 ? -v : v);
        bits += ac.size[((run & 15) << 4) | cat] + cat;
        run = 0;
    }
    if (last < 63) bits += ac.size[0];
    *last_out = last;
    *ac_bits_out = bits;
}

Y7T_RHD inline int y7t_jpeg_dc_bits(int diff, const Y7TJpegHuff& dc) { const int cat = y7t_jpeg_nbits(diff < 0 ? -diff : diff); return dc.size[cat] + cat; }

// The bit sink: the stream as 32-bit words, the stream's first bit the word's bit 31.  A thread gathers the bits of the word it is in and ORs the word into the
// buffer when it leaves it; two blocks share at most the word their boundary falls in, OR commutes, so the buffer (zero before) does not depend on the order.
struct Y7TJpegSink { unsigned* buf; unsigned pos, acc; };
Y7T_RHD inline void y7t_jpeg_sink_or(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (v) atomicOr(p, v);      // (LDS)
#else
    *p |= v;
#endif
}
Y7T_RHD inline void y7t_jpeg_put(Y7TJpegSink& s, unsigned v, int n) {      // the low n bits of v, 0 <= n <= 27
    if (n == 0) return;
    v &= (1u << n) - 1u;
    const int room = 32 - (int)(s.pos & 31);
    if (n < room) {
        s.acc |= v << (room - n);
    } else {
        s.acc |= v >> (n - room);
        y7t_jpeg_sink_or(s.buf + (s.pos >> 5), s.acc);
        s.acc = n > room ? v << (32 - (n - room)) : 0u;
    }
    s.pos += n;
}
Y7T_RHD inline void y7t_jpeg_flush(Y7TJpegSink& s) { if (s.pos & 31) y7t_jpeg_sink_or(s.buf + (s.pos >> 5), s.acc); s.acc = 0; }

// the code of one block: the DC difference, then (run, size) symbols with ZRL for runs over 15, then EOB unless the last coefficient is not zero
Y7T_RHD inline void y7t_jpeg_emit_block(Y7TJpegSink& s, const short* zz, int last, int diff, const Y7TJpegHuff& dc, const Y7TJpegHuff& ac) {
    int cat = y7t_jpeg_nbits(diff < 0 ? -diff : diff);
    y7t_jpeg_put(s, ((unsigned)dc.code[cat] << cat) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u)), dc.size[cat] + cat);
    int run = 0;
    for (int k = 1; k <= last; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) y7t_jpeg_put(s, ac.code[0xF0], ac.size[0xF0]);
        cat = y7t_jpeg_nbits(v < 0 ? -v : v);
        const int sym = (run << 4) | cat;
        y7t_jpeg_put(s, ((unsigned)ac.code[sym] << cat) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u)), ac.size[sym] + cat);
        run = 0;
    }
    if (last < 63) y7t_jpeg_put(s, ac.code[0], ac.size[0]);
}

// the frame's geometry in MCUs
struct Y7TJpegGeom { int H, W, sub, mw, mh, mcols, mrows, bpm, row_blocks; };
Y7T_RHD inline Y7TJpegGeom y7t_jpeg_geom(int H, int W, int sub) {
    Y7TJpegGeom g;
    g.H = H; g.W = W; g.sub = sub;
    g.mw = g.mh = sub == Y7T_JPEG_420 ? 16 : 8;
    g.mcols = (W + g.mw - 1) / g.mw; g.mrows = (H + g.mh - 1) / g.mh;
    g.bpm = sub == Y7T_JPEG_420 ? 6 : 3;
    g.row_blocks = g.mcols * g.bpm;
    return g;
}
// block k of an MCU: its component, its first pixel inside the MCU, and the block of the row (relative to it) that holds its DC predictor
Y7T_RHD inline int y7t_jpeg_block_comp(int sub, int k) { return sub == Y7T_JPEG_420 ? (k < 4 ? 0 : k - 3) : k; }
Y7T_RHD inline int y7t_jpeg_block_prev(int sub, int k) { return sub == Y7T_JPEG_420 ? (k == 0 ? 3 : (k < 4 ? 1 : 6)) : 3; }      // blocks back
// bytes of a row's segment slot: every block at its longest, every byte stuffed
Y7T_RHD inline size_t y7t_jpeg_slot_bytes(const Y7TJpegGeom& g) { return ((size_t)g.row_blocks * Y7T_JPEG_BLOCK_BYTES * 2 + 16 + 15) & ~(size_t)15; }
// bytes of a frame's file at most: header, every slot, the markers between and after them
inline size_t y7t_jpeg_file_max(const Y7TJpegGeom& g) { return Y7T_JPEG_HEADER_MAX + (size_t)g.mrows * (y7t_jpeg_slot_bytes(g) + 2) + 2; }

// ---- host only: the tables and the header ----
// Annex K of ITU-T T.81: the example quantisation tables and the typical Huffman tables (BITS, HUFFVAL)
static const unsigned char y7t_jpeg_k1[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
static const unsigned char y7t_jpeg_dc_bits_k3[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const unsigned char y7t_jpeg_ac_bits_k5[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const unsigned char y7t_jpeg_ac_vals_k5[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// Annex C: the codes of a table from its BITS and HUFFVAL
inline void y7t_jpeg_derive(const unsigned char* bits, const unsigned char* vals, Y7TJpegHuff* h) {
    memset(h, 0, sizeof(*h));
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k) { h->code[vals[k]] = (unsigned short)code++; h->size[vals[k]] = (unsigned char)len; }
        code <<= 1;
    }
}
// the IJG scaling of the Annex K tables, baseline (1 .. 255)
inline void y7t_jpeg_make_tables(int quality, Y7TJpegTables* t) {
    const int ql = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int s = ql < 50 ? 5000 / ql : 200 - 2 * ql;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            int v = ((int)y7t_jpeg_k1[c][i] * s + 50) / 100;
            t->q[c][i] = (unsigned short)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    static const unsigned char dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (int c = 0; c < 2; ++c) {
        y7t_jpeg_derive(y7t_jpeg_dc_bits_k3[c], dc_vals, &t->dc[c]);
        y7t_jpeg_derive(y7t_jpeg_ac_bits_k5[c], y7t_jpeg_ac_vals_k5[c], &t->ac[c]);
    }
}
// SOI, APP0 (JFIF 1.01, no density), DQT x 2, SOF0, DHT x 4, DRI (one MCU row), SOS -> bytes written (<= Y7T_JPEG_HEADER_MAX)
inline int y7t_jpeg_header(const Y7TJpegGeom& g, const Y7TJpegTables& t, unsigned char* o) {
    int n = 0;
    auto b = [&](int v) { o[n++] = (unsigned char)v; };
    auto w = [&](int v) { b(v >> 8); b(v & 255); };
    w(0xFFD8);
    w(0xFFE0); w(16); b('J'); b('F'); b('I'); b('F'); b(0); w(0x0101); b(0); w(1); w(1); b(0); b(0);
    for (int c = 0; c < 2; ++c) {
        w(0xFFDB); w(67); b(c);
        for (int k = 0; k < 64; ++k) b(t.q[c][y7t_jpeg_zig(k)]);
    }
    w(0xFFC0); w(17); b(8); w(g.H); w(g.W); b(3);
    b(1); b(g.sub == Y7T_JPEG_420 ? 0x22 : 0x11); b(0);
    b(2); b(0x11); b(1);
    b(3); b(0x11); b(1);
    static const unsigned char dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (int cls = 0; cls < 2; ++cls)
        for (int c = 0; c < 2; ++c) {
            const unsigned char* bits = cls ? y7t_jpeg_ac_bits_k5[c] : y7t_jpeg_dc_bits_k3[c];
            const unsigned char* vals = cls ? y7t_jpeg_ac_vals_k5[c] : dc_vals;
            const int nv = cls ? 162 : 12;
            w(0xFFC4); w(19 + nv); b((cls << 4) | c);
            for (int i = 0; i < 16; ++i) b(bits[i]);
            for (int i = 0; i < nv; ++i) b(vals[i]);
        }
    w(0xFFDD); w(4); w(g.mcols);
    w(0xFFDA); w(12); b(3); b(1); b(0x00); b(2); b(0x11); b(3); b(0x11); b(0); b(63); b(0);
    return n;
}
