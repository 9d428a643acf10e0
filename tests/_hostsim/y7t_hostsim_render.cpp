// tests/_hostsim/y7t_hostsim_render.cpp -- TEST INFRASTRUCTURE ONLY.
// The CPU build of yolov7-tracker_amd/csrc/y7t_render.h: the overlay one pixel at a time against every track of its frame, last to first (the device lists the tracks
// per tile; the per-track test is the SAME function), and the JPEG encoder one block at a time with the SAME block, code and header functions, a whole MCU row into
// one bit buffer (the device takes 256 blocks at a time with a carried bit offset).  The product package never loads this library.
#include "../../yolov7-tracker_amd/csrc/y7t_render.h"
#include <stddef.h>
#include <vector>

extern "C" {
void hs_render_draw(const unsigned char* in, int B, int H, int W, const Y7TRenderTrack* tracks, const int* offsets, unsigned char* out) {
    for (int b = 0; b < B; ++b) {
        std::vector<Y7TRenderPrim> prims;
        for (int t = offsets[b]; t < offsets[b + 1]; ++t) prims.push_back(y7t_render_prim(tracks[t]));
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t at = (((size_t)b * H + y) * W + x) * 3;
                unsigned char c[3] = {in[at], in[at + 1], in[at + 2]};
                for (int k = (int)prims.size() - 1; k >= 0; --k)
                    if (y7t_render_hit(prims[k], x, y, c)) break;
                out[at] = c[0]; out[at + 1] = c[1]; out[at + 2] = c[2];
            }
    }
}

struct FramePx {
    const unsigned char* f;
    int H, W;
    unsigned operator()(int x, int y) const {
        x = x < W ? x : W - 1;
        y = y < H ? y : H - 1;
        const unsigned char* p = f + ((size_t)y * W + x) * 3;
        return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
    }
};

size_t hs_jpeg_file_max(int H, int W, int sub) { return y7t_jpeg_file_max(y7t_jpeg_geom(H, W, sub)); }

// one (H, W, 3) BGR frame -> the file's bytes in out (hs_jpeg_file_max of room); returns their number
size_t hs_jpeg_encode(const unsigned char* frame, int H, int W, int quality, int sub, unsigned char* out) {
    const Y7TJpegGeom g = y7t_jpeg_geom(H, W, sub);
    Y7TJpegTables tab;
    y7t_jpeg_make_tables(quality, &tab);
    size_t n = (size_t)y7t_jpeg_header(g, tab, out);
    const FramePx px = {frame, H, W};
    std::vector<short> coef((size_t)g.row_blocks * 64);
    std::vector<int> last(g.row_blocks), acb(g.row_blocks);
    std::vector<unsigned> buf((size_t)g.row_blocks * Y7T_JPEG_BLOCK_BYTES / 4 + 4);
    for (int mrow = 0; mrow < g.mrows; ++mrow) {
        for (int j = 0; j < g.row_blocks; ++j) {
            const int m = j / g.bpm, k = j % g.bpm, comp = y7t_jpeg_block_comp(sub, k);
            const bool luma420 = sub == Y7T_JPEG_420 && comp == 0;
            y7t_jpeg_block(px, comp, m * g.mw + (luma420 ? (k & 1) * 8 : 0), mrow * g.mh + (luma420 ? (k >> 1) * 8 : 0), sub == Y7T_JPEG_420 && comp > 0,
                           tab.q[comp ? 1 : 0], tab.ac[comp ? 1 : 0], &coef[(size_t)j * 64], &last[j], &acb[j]);
        }
        std::fill(buf.begin(), buf.end(), 0u);
        Y7TJpegSink s = {buf.data(), 0u, 0u};
        for (int j = 0; j < g.row_blocks; ++j) {
            const int k = j % g.bpm, cls = y7t_jpeg_block_comp(sub, k) ? 1 : 0, back = y7t_jpeg_block_prev(sub, k);
            const int diff = coef[(size_t)j * 64] - ((back == 1 || j >= g.bpm) ? coef[(size_t)(j - back) * 64] : 0);
            const unsigned before = s.pos;
            y7t_jpeg_emit_block(s, &coef[(size_t)j * 64], last[j], diff, tab.dc[cls], tab.ac[cls]);
            if ((int)(s.pos - before) != acb[j] + y7t_jpeg_dc_bits(diff, tab.dc[cls])) return 0;      // (the length the device's scan uses is the length of the code)
        }
        const int pad = (8 - (int)(s.pos & 7)) & 7;
        y7t_jpeg_put(s, (1u << pad) - 1u, pad);
        y7t_jpeg_flush(s);
        for (unsigned i = 0; i < s.pos >> 3; ++i) {
            const unsigned v = buf[i >> 2] >> (24 - 8 * (i & 3)) & 255u;
            out[n++] = (unsigned char)v;
            if (v == 255u) out[n++] = 0;
        }
        out[n++] = 0xFF;
        out[n++] = (unsigned char)(mrow == g.mrows - 1 ? 0xD9 : 0xD0 + (mrow & 7));
    }
    return n;
}
}
