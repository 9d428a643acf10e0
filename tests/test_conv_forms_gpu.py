"""GPU: every product form of the convolution kernels alone, by name, on a plan of one op (y7t_det_create / y7t_det_forward_ops / y7t_det_forward_fused over an arena the
test owns: the Arena / Plan harness of tests/test_membound_gpu.py), at the smallest shape that reaches the form.  Reference and bar: tests/conv_ref.py (float64 of the fp16
values; tests/teacher_forced.py::conv_tolerance, no new number); tests/test_conv_ref_cpu.py shows what the instrument catches.

Every case
  * asserts y7t_last_kernel() exactly -- the expected name is written by hand from the dispatch code (csrc/y7t_conv.hip::conv_dispatch and the launchers); where the name
    does not tell the form (p8: persistent or one tile per workgroup; the tile-counter kernels: fewer / exactly 2 / more chunks per workgroup) the launcher's rule is
    restated on torch.cuda.get_device_properties(0).multi_processor_count and asserted;
  * may not WRITE outside its output slice: the arena (guard buffers in front of the first and behind the last buffer, the 256-byte gaps, the channels outside the slices,
    the input buffers) is compared bit for bit with a snapshot taken before the run;
  * may not READ what it has no business reading: the gaps around the input buffers, the channels outside the input slice and the never-stored upsampled channel range of
    a concat buffer hold NaN, and the output must hold none;
  * runs three times on the same plan: bit-identical outputs (the tile counters hand themselves back), each inside the bar;
  * prints one MARGIN line: kernel, case, worst err / tol (profiles/conv_forms_margins.txt keeps the listing of one run).
Inputs normal(0, 1) fp16, weights normal / sqrt(K) (rows Cout .. Cout_pad zero), biases normal(0, 0.5).  Cases above 20 000 output pixels compare every pixel of the first
and the last pixel tile of each image plus a seeded tenth (or less, as listed) of the rest; the NaN, write and run-to-run checks always cover the whole tensor."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests.post_scenes import unpack_candidates
from tests.test_membound_gpu import Arena, Plan
from tests.util import layer_cout_pad, pack_w
from yolov7_tracker_amd.detector.layout import WeightLayout as WL

pytestmark = pytest.mark.gpu

E_ARG = -1
SEEN = set()

# every product instantiation this file pins, written by hand from the launchers' y7t_note_kernel calls
PRODUCT_FORMS = {
    "igemm<128,128,64,2>", "igemm<128,64,64,2>", "igemm<128,64,32,2> ragged-K", "igemm<128,64,64,2> ragged-K", "igemm<128,64,32,2> 1x1 splitK", "igemm<128,64,64,2> splitK",
    "igemm<128,64,32,2> 1x1", "igemm<256,128,32,2> ragged-K", "igemm<256,64,32,2> ragged-K",
    "igemm<128,128,32,2> 1x1 upsample-on-read", "igemm<128,64,32,2> 1x1 upsample-on-read", "p8<256,256,64> 1x1 upsample-on-read", "p8<256,256,64> 1x1",
    "ws64<16,16> dyn", "ws128<4,16> dyn", "ws128_s2<2,16> dyn", "ws_s2<2,32>", "ws_s2<2,32> + 1x1",
    "patch<16,16,128>", "patch<32,8,128>", "patch<16,16,64>", "patch<32,8,64>", "patch_mt<16,16,4>", "patch_mt<32,8,4>",
    "patch_strip<20,64>", "patch_strip<20,128>", "patch_strip<40,64>", "patch_strip<40,128>",
    "igemm<128,64,32,4> 1x1 detect-decode", "igemm<128,64,32,2> 1x1 detect-decode",
}


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ harness
def conv_op(in_buf, in_ld, in_coff, H, W, Cin, out_buf, out_ld, out_coff, out_f32, Cout, Cout_pad, k, s, act, korder, w_off=0, bias_off=0, up=None, detect_level=-1):
    from yolov7_tracker_amd.detector import graph
    op = np.zeros((), graph.OP_DTYPE)
    p = k // 2
    op["type"], op["in_buf"], op["in_ld"], op["in_coff"], op["H"], op["W"], op["Cin"] = 0, in_buf, in_ld, in_coff, H, W, Cin
    op["out_buf"], op["out_ld"], op["out_coff"], op["out_f32"] = out_buf, out_ld, out_coff, out_f32
    op["Ho"], op["Wo"], op["Cout"], op["Cout_pad"] = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, Cout, Cout_pad
    op["KH"], op["KW"], op["stride"], op["pad"], op["K"], op["K_pad"] = k, k, s, p, k * k * Cin, (k * k * Cin + 63) // 64 * 64
    op["act"], op["korder"], op["detect_level"], op["w_off"], op["bias_off"] = act, int(korder), detect_level, w_off, bias_off
    if up is not None:
        op["up_buf"], op["up_ld"], op["up_coff"], op["up_c0"], op["up_C"] = up
    return op


def _span(arena, i):
    H, W, ld = arena.shapes[i]
    o = arena.offsets[i] // 2
    return o, o + arena.B * H * W * ld


def poison_reads(arena, bufs):
    """NaN into the input buffers `bufs` and into the gaps in front of and behind them (the caller then writes the slices the op reads)"""
    for i in bufs:
        a, b = _span(arena, i)
        nxt = arena.offsets[i + 1] // 2 if i + 1 < len(arena.offsets) else arena.mem.numel()
        arena.mem[a - 128:nxt] = float("nan")


def bits(t):
    """the bit patterns (NaN-safe, any dtype)"""
    return t.contiguous().view(torch.int16)


class Case:
    """one conv op (or the twin pair in one op) on its own plan.  Buffers: 0 guard | 1 input | 2 half-resolution source (4 x 4 dummy without `up`) | 3 output | 4 guard"""

    def __init__(self, L, label, B, H, W, Cin, Cout, k, s, act, korder, in_ld=None, in_coff=0, out_ld=None, out_coff=0, out_f32=0, up=None, up_ld=None, up_coff=0, twin=False,
                 detect_level=-1, seed=None):
        self.L, self.label, self.B, self.H, self.W, self.Cin, self.Cout, self.k, self.s, self.act = L, label, B, H, W, Cin, Cout, k, s, act
        self.korder, self.in_coff, self.out_coff, self.out_f32, self.up, self.up_coff, self.twin = WL(korder), in_coff, out_coff, out_f32, up, up_coff, twin
        self.in_ld, self.out_ld = in_ld or Cin, out_ld or Cout
        p = k // 2
        self.Ho, self.Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.M, self.K = B * self.Ho * self.Wo, k * k * Cin
        rng = np.random.default_rng(zlib.crc32(repr((label, B, H, W, Cin, Cout, k, s, act, int(korder))).encode()) if seed is None else seed)
        self.rng = rng
        self.up_ld = up_ld or (up[1] if up else 8)
        lo_shape = (H // 2, W // 2, self.up_ld) if up else (4, 4, 8)
        self.arena = Arena([(8, 8, 64), (H, W, self.in_ld), lo_shape, (self.Ho, self.Wo, self.out_ld * (2 if out_f32 else 1)), (8, 8, 64)], B)
        poison_reads(self.arena, [1, 2] if up else [1])
        # what the op reads
        self.x = rng.normal(0, 1, (B, H, W, Cin)).astype(np.float16)
        xin = torch.from_numpy(self.x).cuda()
        if up:
            c0, C = up
            self.lo = rng.normal(0, 1, (B, H // 2, W // 2, C)).astype(np.float16)
            self.arena.view(2)[..., up_coff:up_coff + C] = torch.from_numpy(self.lo).cuda()
            xin[..., c0:c0 + C] = float("nan")                                          # never stored at full resolution
        self.arena.view(1)[..., in_coff:in_coff + Cin] = xin
        # weights and biases
        cout_pad = layer_cout_pad(Cout, self.korder)
        if self.korder == WL.PANEL_1X1 and Cout % 128 == 0:
            cout_pad = Cout
        self.Wt = (rng.normal(0, 1, (Cout, Cin, k, k)) / np.sqrt(self.K)).astype(np.float16)
        self.bias = rng.normal(0, 0.5, Cout).astype(np.float32)
        self.cout_pad = cout_pad
        self._pack()
        self.op = conv_op(1, self.in_ld, in_coff, H, W, Cin, 3, self.out_ld, out_coff, out_f32, Cout, cout_pad, k, s, act, self.korder,
                          up=(2, self.up_ld, up_coff) + tuple(up) if up else None, detect_level=detect_level)

    def _pack(self):
        wp = pack_w(self.Wt.astype(np.float32), self.Cin, self.cout_pad, self.korder).ravel()
        bp = np.zeros(self.cout_pad, np.float32)
        bp[:self.Cout] = self.bias
        if self.twin:
            from yolov7_tracker_amd.detector import weights
            self.W2 = (self.rng.normal(0, 1, (128, 128, 1, 1)) / np.sqrt(128)).astype(np.float16)
            self.b2 = self.rng.normal(0, 0.5, 128).astype(np.float32)
            wp = np.concatenate([wp, weights.pack_ws_s2_tail(self.W2.reshape(128, 128)).ravel()])
            bp = np.concatenate([bp, self.b2])
        self.arena.dummy_w, self.arena.dummy_b = torch.from_numpy(np.ascontiguousarray(wp)).cuda(), torch.from_numpy(bp).cuda()

    def out_view(self):
        v = self.arena.view(3)
        return v.view(torch.float32) if self.out_f32 else v

    def reference(self, rows):
        x = self.x.astype(np.float64)
        if self.up:
            x = cr.concat_input(self.x, 0, self.Cin, (self.lo, 0) + tuple(self.up))
        if self.twin:
            ref, absum = cr.twin_ref(x, self.Wt, self.bias, self.W2, self.b2, self.act, rows)
            return ref, absum, cr.tolerance(ref, absum, 128, 2.0 ** -11), 128
        ref, absum = cr.conv_ref(x, self.Wt, self.bias, self.k, self.s, self.act, rows)
        return ref, absum, cr.tolerance(ref, absum, self.K), self.K

    def run(self, kernel, rows=None, runs=3):
        """three forwards; -> worst err / tol.  rows: the pixel indices that are compared with float64 (None: all)"""
        snap = self.arena.mem.clone()
        plan = Plan(self.L, [self.op], self.arena)
        outs = []
        try:
            for _ in range(runs):
                self.arena.mem.copy_(snap)                    # the output slice holds the sentinel again: a forward that stores nothing cannot pass on the last one's values
                rc, name = plan.run()
                assert rc == 0, (rc, self.L.y7t_last_error())
                assert name == kernel, "%s ran %r, the dispatch code says %r" % (self.label, name, kernel)
                outs.append(self.out_slice().clone())
        finally:
            plan.close()
        for o in outs[1:]:
            assert torch.equal(bits(o), bits(outs[0])), "%s: runs differ" % self.label
        assert not bool(torch.isnan(outs[0]).any()), "%s: %d NaN in the output (the kernel read a position it must not read)" % (self.label, int(torch.isnan(outs[0]).sum()))
        self.assert_only_the_output_slice_changed(snap)
        return self.check_values(outs[0], kernel, rows)

    def out_slice(self):
        return self.out_view()[..., self.out_coff:self.out_coff + self.Cout]

    def assert_only_the_output_slice_changed(self, snap):
        """nothing but the output slice has changed against the snapshot `snap` of the arena"""
        after = self.arena.mem.clone()
        a, b = _span(self.arena, 3)
        av, sv = after[a:b].view(self.B, self.Ho, self.Wo, -1), snap[a:b].view(self.B, self.Ho, self.Wo, -1)
        f = 2 if self.out_f32 else 1
        av[..., f * self.out_coff:f * (self.out_coff + self.Cout)] = sv[..., f * self.out_coff:f * (self.out_coff + self.Cout)]
        changed = int((bits(after) != bits(snap)).sum())
        assert changed == 0, "%s: %d fp16 positions outside the output slice were written" % (self.label, changed)

    def check_values(self, out, kernel, rows=None, note=""):
        """the values of one forward (a clone of the output slice) against float64 at the bar; prints the MARGIN line.  -> worst err / tol"""
        ref, absum, tol, K = self.reference(rows)
        got = out.reshape(self.M, self.Cout)
        got = (got if rows is None else got[torch.from_numpy(rows).cuda()]).double().cpu().numpy()
        ratio = cr.worst_ratio(got, ref, tol)
        extra = ""
        if self.out_f32:
            extra = "   fp32-only bound: %.3g" % cr.worst_ratio(got, ref, cr.f32_bound(ref, absum, K, self.act))
        print("\nMARGIN %-44s %-86s %.3f%s%s%s" % (kernel, self.label, ratio, extra, "" if rows is None else "   (%d of %d pixels)" % (len(rows), self.M), note))
        assert ratio <= 1.0, "%s: worst err / tol %.3g" % (self.label, ratio)
        SEEN.add(kernel)
        return ratio


def some_rows(c, tile, fraction=0.1):
    """(above 8 images: 16 pixels at both ends of every image instead of a whole tile; the launch's last pixel tile is always whole)"""
    if c.M <= 20000:
        return None
    rows = cr.pixel_rows(c.B, c.Ho, c.Wo, min(tile if c.B <= 8 else 16, c.Ho * c.Wo), 7, fraction)
    return np.union1d(rows, np.arange((c.M - 1) // tile * tile, c.M))


# ------------------------------------------------------------------------------------------------ 1. k_conv_igemm, plain
# B, H, W, Cin, Cout, k, s, act, korder, in_ld, in_coff, out_ld, out_coff, out_f32
IGEMM_CASES = [
    # 3x3 with uniform taps and NO split-K: 64 pixel tiles x 4 channel tiles = 256 tiles (launch_conv_ut splits below 256), not narrow (64 * 4 is not < 256)
    ("uniform taps, no split-K, TAP_MAJOR", "igemm<128,128,64,2>", (2, 128, 128, 64, 512, 3, 2, 1, WL.TAP_MAJOR, 64, 0, 512, 0, 0)),
    ("uniform taps, no split-K, LINE_MAJOR odometer from step 0", "igemm<128,128,64,2>", (2, 128, 128, 192, 512, 3, 2, 1, WL.LINE_MAJOR, 256, 64, 640, 128, 0)),
    # the narrow rule: tm = 100; 100 * 2 = 200 < 256 <= 100 * 4 = 400
    ("narrow rule on a layer that allows 128-wide tiles", "igemm<128,64,64,2>", (8, 80, 80, 128, 256, 3, 2, 1, WL.LINE_MAJOR, 128, 0, 256, 0, 0)),
    # ragged K
    ("ragged K, 1x1 Cin 40", "igemm<128,64,32,2> ragged-K", (2, 9, 13, 40, 64, 1, 1, 2, WL.TAP_MAJOR, 64, 16, 96, 32, 0)),
    ("ragged K, 3x3 s2 Cin 8 (K = 72: tiny's first layer)", "igemm<128,64,64,2> ragged-K", (2, 21, 27, 8, 32, 3, 2, 2, WL.TAP_MAJOR, 8, 0, 32, 0, 0)),
    ("ragged K, 3x3 Cin 16, ragged last pixel tile (M = 429)", "igemm<128,64,64,2> ragged-K", (3, 13, 11, 16, 64, 3, 1, 1, WL.TAP_MAJOR, 16, 0, 64, 0, 0)),
    # split-K (tiles < 256 and >= 8 K-steps) and k_splitk_reduce
    ("split-K, fp16 out Cout 44 ld 44 (half4 stores)", "igemm<128,64,32,2> 1x1 splitK", (2, 10, 14, 512, 44, 1, 1, 1, WL.TAP_MAJOR, 512, 0, 44, 0, 0)),
    ("split-K, fp16 out Cout 46 ld 48 (the n + 3 >= Cout tail)", "igemm<128,64,32,2> 1x1 splitK", (2, 10, 14, 512, 46, 1, 1, 2, WL.TAP_MAJOR, 512, 0, 48, 0, 0)),
    ("split-K, fp32 out Cout 45", "igemm<128,64,32,2> 1x1 splitK", (2, 10, 14, 256, 45, 1, 1, 0, WL.TAP_MAJOR, 256, 0, 45, 0, 1)),
    # 27 K-steps in 6 splits of 5: splits start at steps 5, 10, 20, 25 -- inside a (kh, chunk, kw) group of three
    ("split-K, LINE_MAJOR s2 Cin 192, splits start inside a group", "igemm<128,64,64,2> splitK", (1, 33, 31, 192, 64, 3, 2, 1, WL.LINE_MAJOR, 256, 64, 64, 0, 0)),
    # the direct fp16 epilogue (Cout % 8 != 0) without split-K: 2 K-steps
    ("direct fp16 epilogue, Cout 20 in ld 24 at 4, M = 300", "igemm<128,64,32,2> 1x1", (3, 10, 10, 64, 20, 1, 1, 1, WL.TAP_MAJOR, 64, 0, 24, 4, 0)),
    # the 256-pixel tiles: (M / 256) * (Cout_pad / BN) >= 2048
    ("256-pixel tiles, s2 Cin 8 -> 1024, M = 131072", "igemm<256,128,32,2> ragged-K", (2, 512, 512, 8, 1024, 3, 2, 1, WL.TAP_MAJOR, 8, 0, 1024, 0, 0)),
    ("256-pixel tiles, stem-like Cin 16 -> 64, M = 2048 * 256", "igemm<256,64,32,2> ragged-K", (2, 512, 512, 16, 64, 3, 1, 1, WL.TAP_MAJOR, 16, 0, 64, 0, 0)),
]


@pytest.mark.parametrize("label,kernel,case", IGEMM_CASES, ids=[c[0] for c in IGEMM_CASES])
def test_igemm_plain(L, label, kernel, case):
    B, H, W, Cin, Cout, k, s, act, korder, in_ld, in_coff, out_ld, out_coff, out_f32 = case
    c = Case(L, "%s %s" % (label, case[:8]), B, H, W, Cin, Cout, k, s, act, korder, in_ld, in_coff, out_ld, out_coff, out_f32)
    c.run(kernel, some_rows(c, 256))


# ------------------------------------------------------------------------------------------------ 2. upsample-on-read
# (up_c0, up_C) in a concat of 192 channels: first, inside and last; 32 (mod 64) wherever the position allows (the launcher admits multiples of 32, w6 only uses 64)
UP_RANGES = [(0, 32), (32, 96), (96, 96)]


@pytest.mark.parametrize("korder", [WL.TAP_MAJOR, WL.PANEL_1X1], ids=["TAP_MAJOR", "PANEL_1X1"])
@pytest.mark.parametrize("Cout,kernel", [(128, "igemm<128,128,32,2> 1x1 upsample-on-read"), (64, "igemm<128,64,32,2> 1x1 upsample-on-read")])
@pytest.mark.parametrize("up", UP_RANGES, ids=["first", "inside", "last"])
def test_igemm_upsample_on_read(L, up, Cout, kernel, korder):
    c = Case(L, "up [%d, %d) of 192 -> %d %s, source at 32 of a wider buffer" % (up[0], up[0] + up[1], Cout, WL(korder).name), 2, 10, 14, 192, Cout, 1, 1, 1 + (up[0] == 32),
             korder, in_ld=208, in_coff=8, out_ld=Cout + 32, out_coff=16, up=up, up_ld=up[1] + 40, up_coff=32)
    c.run(kernel)


@pytest.mark.parametrize("what", ["odd H", "up_c0 % 32", "PANEL_1X1_N64"])
def test_upsample_on_read_refusals(L, what):
    H = 9 if what == "odd H" else 10
    up = (16, 64) if what == "up_c0 % 32" else (32, 64)
    korder = WL.PANEL_1X1_N64 if what == "PANEL_1X1_N64" else WL.TAP_MAJOR
    c = Case(L, what, 2, H, 14, 192, 64, 1, 1, 1, korder, up=up, up_ld=72, up_coff=8)
    snap = c.arena.mem.clone()
    plan = Plan(L, [c.op], c.arena)
    try:
        rc, _ = plan.run()
    finally:
        plan.close()
    assert rc == E_ARG, (what, rc)
    assert torch.equal(bits(c.arena.mem), bits(snap))


def p8_form(M, Cin, cout_pad, ncu):
    """csrc/y7t_conv_p8.hip::y7t_conv_p8_launch: the persistent form (in a plan: on the tile counter) where a workgroup gets >= 2 tiles and Cin / 64 is even"""
    ntn = cout_pad // 256
    grid, gp = -(-M // 256) * ntn, ncu // ntn * ntn
    return "persistent" if (Cin // 64) % 2 == 0 and gp > 0 and grid >= 2 * gp else "one tile per workgroup"


@pytest.mark.parametrize("form", ["one tile per workgroup", "persistent"])
@pytest.mark.parametrize("up", [(0, 64), (64, 128), (128, 64)], ids=["first", "inside", "last"])
def test_p8_upsample_on_read(L, ncu, up, form):
    B = 2 if form == "one tile per workgroup" else -(-(2 * ncu * 256 + 1) // 140)      # 10 x 14 maps: >= 2 * gp_ + 1 pixel tiles of one channel tile
    Cin = 192 if form != "persistent" else 256                                       # (the persistent form needs an even number of K-tiles)
    assert p8_form(B * 140, Cin, 256, ncu) == form
    c = Case(L, "p8 %s, up [%d, %d) of %d -> 256, B %d" % (form, up[0], up[0] + up[1], Cin, B), B, 10, 14, Cin, 256, 1, 1, 1, WL.P8, in_ld=Cin + 16, in_coff=8, out_ld=288,
             out_coff=16, up=up, up_ld=up[1] + 40, up_coff=32)
    assert c.M % 256 != 0
    c.run("p8<256,256,64> 1x1 upsample-on-read", None if c.M <= 20000 else cr.pixel_rows(1, c.M, 1, 256, 7, 0.02))


# ------------------------------------------------------------------------------------------------ 3. tile-counter forms
def dyn_case(L, ncu, which, korder, s, Cin, Cout, TH, TW, n_nt, act):
    """-> (Case, rows to compare).  TH x TW OUTPUT tiles, 2 tiles per chunk, grid = min(chunks * n_nt, ncu) workgroups of which grid / n_nt share a counter: chunks 0 and 1 of a workgroup are
    static, every later one comes from the counter"""
    assert ncu % 4 == 0
    wgs = ncu // n_nt                                                               # workgroups per counter on a full grid
    if which == "fewer chunks than workgroups":
        B, ty, tx = 1, 2, 3
    elif which == "exactly 2 chunks per workgroup":
        B, ty, tx = 4, 1, wgs                                                         # 4 * wgs tiles = 2 * wgs chunks
    else:                                                                             # more than 2 * wgs + 1 chunks, an odd number of tiles, an odd number per row, B = 3
        B, tx = 3, 13 if n_nt > 1 else next(n for n in range(1, 999, 2) if 3 * n * n > 4 * wgs + 2)
        ty = tx if n_nt == 1 else next(n for n in range(1, 999, 2) if 3 * 13 * n > 4 * wgs + 2)
    tiles = B * ty * tx
    chunks = -(-tiles // 2)
    grid_c = min(chunks * n_nt, ncu) // n_nt
    assert {"fewer chunks than workgroups": chunks < wgs, "exactly 2 chunks per workgroup": chunks == 2 * grid_c and grid_c == wgs,
            "more chunks, odd tile count": chunks > 2 * grid_c + 1 and tiles % 2 == 1 and tx % 2 == 1}[which], (which, tiles, chunks, grid_c)
    H, W = ty * TH * s, tx * TW * s
    c = Case(L, "%s: %d tiles, %d chunks, %d workgroups per counter; B %d %dx%d act %d" % (which, tiles, chunks, grid_c, B, H, W, act), B, H, W, Cin, Cout, 3, s, act, korder,
             in_ld=Cin + 64, in_coff=64, out_ld=Cout + 128, out_coff=128)
    return c, some_rows(c, TH * TW * 2, 0.03)


def _dyn_case(L, ncu, kernel, which, korder, s, Cin, Cout, TH, TW, n_nt, act):
    c, rows = dyn_case(L, ncu, which, korder, s, Cin, Cout, TH, TW, n_nt, act)
    c.run(kernel, rows)


# the three tile-counter kernels of _dyn_case: kernel -> (korder, stride, Cin, Cout, TH, TW, counters, activation of regime i)
DYN_FORMS = {"ws64<16,16> dyn": (WL.WS64, 1, 64, 64, 16, 16, 1, lambda i: i), "ws128<4,16> dyn": (WL.WS128, 1, 128, 256, 4, 16, 2, lambda i: i),
             "ws128_s2<2,16> dyn": (WL.WS128, 2, 128, 256, 2, 16, 2, lambda i: (i + 1) % 3)}


DYN_WHICH = ["fewer chunks than workgroups", "exactly 2 chunks per workgroup", "more chunks, odd tile count"]


@pytest.mark.parametrize("act,which", enumerate(DYN_WHICH), ids=DYN_WHICH)
def test_ws64_on_the_tile_counter(L, ncu, which, act):
    _dyn_case(L, ncu, "ws64<16,16> dyn", which, WL.WS64, 1, 64, 64, 16, 16, 1, act)


@pytest.mark.parametrize("act,which", enumerate(DYN_WHICH), ids=DYN_WHICH)
def test_ws128_on_two_tile_counters(L, ncu, which, act):
    _dyn_case(L, ncu, "ws128<4,16> dyn", which, WL.WS128, 1, 128, 256, 4, 16, 2, act)


@pytest.mark.parametrize("act,which", enumerate(DYN_WHICH), ids=DYN_WHICH)
def test_ws128_stride2_on_two_tile_counters(L, ncu, which, act):
    _dyn_case(L, ncu, "ws128_s2<2,16> dyn", which, WL.WS128, 2, 128, 256, 2, 16, 2, (act + 1) % 3)


def p8_plan_case(L, ncu, Cin, Cout, form):
    """-> (Case, rows to compare)"""
    ntn = Cout // 256
    tm = -(-2 * (ncu // ntn * ntn) // ntn)                                            # pixel tiles for grid >= 2 * gp_
    B = -(-((tm - 1) * 256 + 1) // 77)                                                # 7 x 11 maps
    assert p8_form(B * 77, Cin, Cout, ncu) == form and (B * 77) % 256 != 0             # ... and a ragged last pixel tile
    c = Case(L, "p8 %s: %d pixel tiles x %d channel tiles on %d CUs, %d -> %d" % (form, -(-B * 77 // 256), ntn, ncu, Cin, Cout), B, 7, 11, Cin, Cout, 1, 1, 1 + (ntn == 1), WL.P8,
             in_ld=Cin + 64, in_coff=64, out_ld=Cout + 64, out_coff=32 if ntn == 1 else 0)
    return c, cr.pixel_rows(1, c.M, 1, 256, 7, 0.02)


@pytest.mark.parametrize("Cin,Cout,form", [(128, 256, "persistent"), (128, 768, "persistent"), (192, 768, "one tile per workgroup")],
                         ids=["one channel tile", "three channel tiles", "odd Cin / 64 stays on one tile per workgroup"])
def test_p8_in_a_plan(L, ncu, Cin, Cout, form):
    c, rows = p8_plan_case(L, ncu, Cin, Cout, form)
    c.run("p8<256,256,64> 1x1", rows)


# ------------------------------------------------------------------------------------------------ 4. ws_s2 and its twin form in a plan
@pytest.mark.parametrize("twin", [False, True], ids=["ws_s2", "ws_s2 + 1x1"])
@pytest.mark.parametrize("which", ["one tile", "more tiles than workgroups"])
def test_ws_s2_in_a_plan(L, ncu, which, twin):
    c, rows = ws_s2_case(L, ncu, which, twin)
    c.run("ws_s2<2,32> + 1x1" if twin else "ws_s2<2,32>", rows)


def ws_s2_case(L, ncu, which, twin):
    """-> (Case, rows to compare)"""
    B, H, W = (1, 4, 64) if which == "one tile" else (3, 4 * next(n for n in range(1, 999, 2) if 3 * 3 * n > ncu), 192)      # 2 x 32 output tiles: 3 per row, an odd number
    tiles = B * (H // 4) * (W // 64)
    assert tiles == 1 or tiles > ncu
    c = Case(L, "%s: %d tiles on %d CUs, B %d %dx%d" % (which, tiles, ncu, B, H, W), B, H, W, 64, 128, 3, 2, 1 + (which == "one tile"), WL.WS_S2_TWIN if twin else WL.WS_S2,
             in_ld=128, in_coff=64, out_ld=256, out_coff=128, twin=twin)
    return c, some_rows(c, 64, 0.1)


# ------------------------------------------------------------------------------------------------ 5. the patch family
# PATCH / PATCH_N64 layout ops (a plan cannot force the patch kernel: the layout sends the op there); ragged right and bottom tiles
PATCH_CASES = [
    # 15 x 34: 16 x 16 tiles are 66 % useful, 32 x 8 tiles 50 %; 19 x 27: 50 % against 67 %
    ("patch<16,16,128>", (2, 15, 34, 64, 128, 1, WL.PATCH)),
    ("patch<32,8,128>", (2, 19, 27, 128, 128, 2, WL.PATCH)),
    ("patch<16,16,64>", (2, 15, 34, 192, 64, 1, WL.PATCH)),
    ("patch<32,8,64>", (2, 19, 27, 64, 64, 1, WL.PATCH)),
    # multi-tile workgroups: 64-row panels and tiles * (Cout_pad / 64) >= 8192; 114 images of 3 x 3 tiles = 1026 tiles (not a multiple of 4) x 8 panels
    ("patch_mt<16,16,4>", (114, 47, 47, 64, 512, 1, WL.PATCH_N64)),
    ("patch_mt<32,8,4>", (114, 21, 93, 64, 512, 2, WL.PATCH_N64)),
    # dense strips: 420 and 720 positions (two and three workgroups, the last one ragged)
    ("patch_strip<20,64>", (3, 7, 20, 64, 64, 1, WL.PATCH)),
    ("patch_strip<20,128>", (3, 7, 20, 128, 128, 2, WL.PATCH)),
    ("patch_strip<40,64>", (2, 9, 40, 128, 64, 1, WL.PATCH)),
    ("patch_strip<40,128>", (2, 9, 40, 64, 256, 1, WL.PATCH)),
]


@pytest.mark.parametrize("kernel,case", PATCH_CASES, ids=[c[0] for c in PATCH_CASES])
def test_patch_family(L, kernel, case):
    B, H, W, Cin, Cout, act, korder = case
    if kernel.startswith("patch_mt"):
        tw, th = (16, 16) if "16,16" in kernel else (32, 8)
        tiles = B * -(-H // th) * -(-W // tw)
        assert tiles % 4 and tiles * (Cout // 64) >= 8192
    c = Case(L, "%s %s" % (WL(korder).name, case[:6]), B, H, W, Cin, Cout, 3, 1, act, korder, in_ld=Cin + 64, in_coff=64, out_ld=Cout + 64, out_coff=32)
    c.run(kernel, some_rows(c, 256, 0.01))


# ------------------------------------------------------------------------------------------------ 6. the fused Detect epilogue
ANCHORS = [[(12.0, 16.0), (19.0, 36.0), (40.0, 28.0)], [(36.0, 75.0), (76.0, 55.0), (72.0, 146.0)]]
WS_FILL = 0xA5


class DetectPlan:
    """Detect 1x1 convs (one per level) on a plan: plain (fp32 heads, then y7t_det_postprocess' decode pass) and fused (y7t_det_forward_fused).  levels: [(ny, nx, stride)].
    The objectness weights take input channel 0 with weight 1: images listed in `empty` hold -24 there (objectness logit - 24: no candidate), all others 0."""

    def __init__(self, L, B, levels, Cin, no, korder, obj_bias, empty=(), seed=0):
        self.L, self.B, self.levels, self.Cin, self.no, self.Cout = L, B, levels, Cin, no, 3 * no
        rng = np.random.default_rng(seed)
        shapes = [(8, 8, 64)]
        for ny, nx, _ in levels:
            shapes += [(ny, nx, Cin), (ny, nx, 2 * self.Cout)]
        self.arena = Arena(shapes + [(8, 8, 64)], B)
        poison_reads(self.arena, [1 + 2 * l for l in range(len(levels))])
        ops, ws, bs = [], [], []
        self.x, self.Wt, self.bias = [], [], []
        for l, (ny, nx, _) in enumerate(levels):
            x = rng.normal(0, 1, (B, ny, nx, Cin)).astype(np.float16)
            x[..., 0] = 0
            x[list(empty), ..., 0] = -24
            Wt = (rng.normal(0, 1, (self.Cout, Cin, 1, 1)) / np.sqrt(Cin)).astype(np.float16)
            Wt[4::no, 0] = 1
            bias = rng.normal(0, 0.5, self.Cout).astype(np.float32)
            bias[4::no] += obj_bias
            self.arena.view(1 + 2 * l)[...] = torch.from_numpy(x).cuda()
            bp = np.zeros(64, np.float32)
            bp[:self.Cout] = bias
            ops.append(conv_op(1 + 2 * l, Cin, 0, ny, nx, Cin, 2 + 2 * l, self.Cout, 0, 1, self.Cout, 64, 1, 1, 0, korder, w_off=64 * Cin * l, bias_off=64 * l, detect_level=l))
            ws.append(pack_w(Wt.astype(np.float32), Cin, 64, korder).ravel())
            bs.append(bp)
            self.x.append(x), self.Wt.append(Wt), self.bias.append(bias)
        self.arena.dummy_w, self.arena.dummy_b = torch.from_numpy(np.concatenate(ws)).cuda(), torch.from_numpy(np.concatenate(bs)).cuda()
        self.plan = Plan(L, ops, self.arena)
        nl = len(levels)
        self.strides = (ctypes.c_float * 4)(*[float(s) for _, _, s in levels] + [0.0] * (4 - nl))
        flat = [v for l in range(nl) for a in ANCHORS[l] for v in a]
        self.anchors = (ctypes.c_float * 24)(*(flat + [0.0] * (24 - len(flat))))
        self.ny = (ctypes.c_int * 4)(*[ny for ny, _, _ in levels] + [0] * (4 - nl))
        self.nx = (ctypes.c_int * 4)(*[nx for _, nx, _ in levels] + [0] * (4 - nl))
        from yolov7_tracker_amd import _lib
        _lib.check(L.y7t_det_set_detect(self.plan.h, nl, 3, no, self.strides, self.anchors))

    def head(self, l):
        return self.arena.view(2 + 2 * l).view(torch.float32)

    def _ws(self, cap, max_nms):
        n = int(self.L.y7t_det_postprocess_workspace_bytes(self.B, cap, max_nms))
        return torch.full((n,), WS_FILL, dtype=torch.uint8, device="cuda")

    def plain(self, conf, cap, kernel, max_nms=30000):
        """-> candidate arrays of the plain forward + the decode pass (numpy, the workspace's documented head)"""
        from yolov7_tracker_amd import _lib
        rc, name = self.plan.run()
        assert rc == 0 and name == kernel, (rc, name, self.L.y7t_last_error())
        ws = self._ws(cap, max_nms)
        heads = (ctypes.c_void_p * 4)(*[self.head(l).data_ptr() for l in range(len(self.levels))] + [None] * (4 - len(self.levels)))
        lb = torch.tensor([[1.0, 0.0, 0.0, 4096.0, 4096.0]] * self.B, device="cuda")
        dets, ndets = torch.zeros((self.B, 300, 6), device="cuda"), torch.zeros(self.B, dtype=torch.int32, device="cuda")
        keep, cand = torch.zeros((self.B, 300), dtype=torch.int32, device="cuda"), torch.zeros(self.B, dtype=torch.int32, device="cuda")
        _lib.check(self.L.y7t_det_postprocess(heads, self.ny, self.nx, self.strides, self.anchors, len(self.levels), 3, self.no, self.B, float(conf), 0.45, 300, max_nms, cap,
                                              _lib.ptr(lb), _lib.ptr(dets), _lib.ptr(ndets), _lib.ptr(keep), _lib.ptr(cand), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        SEEN.add(name)
        return unpack_candidates(ws.cpu().numpy(), self.B, cap, max_nms)

    def fused(self, conf, cap, kernel, max_nms=30000):
        from yolov7_tracker_amd import _lib
        ws = self._ws(cap, max_nms)
        snap = self.arena.mem.clone()
        _lib.check(self.L.y7t_det_forward_fused(self.plan.h, self.B, 0, -1, float(conf), cap, max_nms, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        name = self.L.y7t_last_kernel().decode()
        assert name == kernel, (name, kernel)
        assert torch.equal(bits(self.arena.mem), bits(snap)), "the fused forward wrote into the arena"      # the head tensors included: they are never written
        SEEN.add(name)
        return unpack_candidates(ws.cpu().numpy(), self.B, cap, max_nms)

    def logits64(self, l):
        ny, nx, _ = self.levels[l]
        x, w = self.x[l].astype(np.float64).reshape(-1, self.Cin), self.Wt[l].astype(np.float64).reshape(self.Cout, self.Cin)
        absum = np.abs(x) @ np.abs(w).T + np.abs(self.bias[l])
        return x @ w.T + self.bias[l], absum

    def close(self):
        self.plan.close()


def _by_cidx(arrs, b, n):
    cbox, cscore, ccls, cidx, _ = arrs
    d = {int(cidx[b, i]): (cbox[b, i].view(np.int32).tolist(), int(cscore[b, i:i + 1].view(np.int32)[0]), int(ccls[b, i:i + 1].view(np.int32)[0])) for i in range(n)}
    assert len(d) == n, "image %d: a candidate row appears twice" % b
    return d


def _assert_untouched_behind(arrs, b, n, what):
    fill4 = np.frombuffer(bytes([WS_FILL] * 4), np.int32)[0]
    for a in arrs[:4]:
        assert (a[b, n:].view(np.int32) == fill4).all(), "%s: image %d: written behind slot %d" % (what, b, n)


def compare_fused_with_plain(dp, conf, cap, label, fused_kernel, plain_kernel="igemm<128,64,32,2> 1x1", runs=3):
    """the fused epilogue's candidates == the plain head's decode pass, bit for bit, as sets keyed by cidx; counts equal; nothing written behind an image's block.
    cap below an image's count: the count keeps counting, exactly cap slots hold distinct members of the full set (the plain pass at a cap that holds them all)"""
    big = max(cap, 3 * sum(ny * nx for ny, nx, _ in dp.levels))
    want = dp.plain(conf, big, plain_kernel)
    wcount = want[4]
    per_run = []
    for _ in range(runs):
        got = dp.fused(conf, cap, fused_kernel)
        assert np.array_equal(got[4], wcount), (label, got[4], wcount)
        sets = []
        for b in range(dp.B):
            n = min(int(wcount[b]), cap)
            g, w = _by_cidx(got, b, n), _by_cidx(want, b, int(wcount[b]))
            assert set(g) <= set(w) and (n < wcount[b] or set(g) == set(w)), (label, b)
            assert all(g[k] == w[k] for k in g), "%s: image %d: %d candidates differ in a bit" % (label, b, sum(g[k] != w[k] for k in g))
            _assert_untouched_behind(got, b, n, label)
            sets.append(g)
        per_run.append(sets)
    assert all(s == per_run[0] for s in per_run[1:]) or int(wcount.max()) > cap      # (over cap the subset kept depends on the order of arrival)
    print("\nMARGIN %-44s %-86s bit-equal to %s + k_decode_filter (%d candidates, max %d of cap %d per image)" % (fused_kernel, label, plain_kernel, int(np.minimum(wcount, cap).sum()),
                                                                                                                int(wcount.max()), cap))
    return wcount


def check_plain_heads(dp, label, kernel):
    """the fp32 heads of the plain forward against float64 at the bar of tests/conv_ref.py"""
    worst = worst32 = 0.0
    for l in range(len(dp.levels)):
        ref, absum = dp.logits64(l)
        got = dp.head(l).double().cpu().numpy().reshape(-1, dp.Cout)
        assert np.isfinite(got).all()
        worst = max(worst, cr.worst_ratio(got, ref, cr.tolerance(ref, absum, dp.Cin)))
        worst32 = max(worst32, cr.worst_ratio(got, ref, cr.f32_bound(ref, absum, dp.Cin)))
    print("\nMARGIN %-44s %-86s %.3g   fp32-only bound: %.3g" % (kernel, label + " (fp32 head)", worst, worst32))
    assert worst <= 1.0


DETECT_CASES = [
    # label, B, levels, Cin, no, korder, obj bias, empty images, conf, cap
    ("5x5 B7: six images in one tile, M = 175, image 3 empty", 7, [(5, 5, 8)], 192, 15, WL.TAP_MAJOR, 1.0, (3,), 0.25, 128),
    ("5x5 B7 no 6, panel-packed", 7, [(5, 5, 8)], 128, 6, WL.PANEL_1X1, 1.0, (3,), 0.25, 128),
    ("3x7 B5 no 21, images 0 and 4 empty", 5, [(3, 7, 16)], 64, 21, WL.TAP_MAJOR, 1.0, (0, 4), 0.25, 64),
    ("5x5 B7 cap 64 below one image's candidates", 7, [(5, 5, 8)], 192, 15, WL.TAP_MAJOR, 4.0, (3,), 0.01, 64),
    ("two levels in one plan, 5x5 + 3x7 (row0 = 75)", 7, [(5, 5, 8), (3, 7, 16)], 128, 15, WL.PANEL_1X1, 1.0, (2,), 0.25, 256),
]


@pytest.mark.parametrize("case", DETECT_CASES, ids=[c[0] for c in DETECT_CASES])
def test_fused_detect_epilogue_is_bit_equal_to_the_decode_pass(L, case):
    label, B, levels, Cin, no, korder, obj_bias, empty, conf, cap = case
    dp = DetectPlan(L, B, levels, Cin, no, korder, obj_bias, empty, seed=len(label) + Cin + no)
    try:
        wcount = compare_fused_with_plain(dp, conf, cap, label, "igemm<128,64,32,4> 1x1 detect-decode")
        check_plain_heads(dp, label, "igemm<128,64,32,2> 1x1")
        assert all(wcount[b] == 0 for b in empty) and all(wcount[b] > 0 for b in range(B) if b not in empty)
        assert ("cap 64 below" in label) == bool(wcount.max() > cap)
        # ... and both agree with the float64 decode of float64 logits on every anchor that is not within rounding of the threshold
        compare_with_float64_decode(dp, dp.plain(conf, 256, "igemm<128,64,32,2> 1x1"), conf, label, "igemm<128,64,32,2> 1x1 + k_decode_filter")
    finally:
        dp.close()


def compare_with_float64_decode(dp, arrs, conf, label, kernel):
    """candidate arrays against the float64 decode of float64 logits, anchor by anchor, each with the bounds its OWN logits' bars leave (tests/conv_ref.py::decode_bounds:
    objectness a quarter of its logit bar; a score -- the product of two probabilities -- a quarter of the objectness bar plus a quarter of the class bar; a box corner
    from that anchor's four box logits).  An anchor whose objectness is above conf by its band and one of whose scores is above conf by ITS band must be a candidate; an
    anchor whose objectness, or every score, is below conf by the band may not be one.  The class the device picked must be one the bounds allow to win
    (score + band >= every other score - its band); the device's score is held against the reference score of that class, the box against its bound."""
    B, worst_s, worst_b, n = dp.B, 0.0, 0.0, 0
    cbox, cscore, ccls, cidx, count = arrs
    row0 = 0
    for l, (ny, nx, stride) in enumerate(dp.levels):
        ref, absum = dp.logits64(l)
        d = cr.decode_bounds(ref.reshape(B, ny, nx, -1), cr.tolerance(ref, absum, dp.Cin).reshape(B, ny, nx, -1), 3, dp.no, ny, nx, stride, ANCHORS[l], row0)
        must = (d["obj"] > conf + d["d_obj"]) & (d["sc"] > conf + d["d_sc"]).any(-1)
        may = (d["obj"] > conf - d["d_obj"]) & (d["sc"] > conf - d["d_sc"]).any(-1)
        where = {int(c): i for i, c in np.ndenumerate(d["cidx"])}                   # cidx -> (y, x, a)
        for b in range(B):
            got = {int(cidx[b, i]): i for i in range(int(count[b])) if row0 <= cidx[b, i] < row0 + 3 * ny * nx}
            assert set(int(c) for c in d["cidx"][must[b]]) <= set(got), (label, l, b)
            assert set(got) <= set(int(c) for c in d["cidx"][may[b]]), (label, l, b)
            for k, i in got.items():
                at = (b,) + where[k]
                sc, dsc, c = d["sc"][at], d["d_sc"][at], int(ccls[b, i])
                assert sc[c] + dsc[c] >= (sc - dsc).max(), (label, l, b, k, c)
                worst_s = max(worst_s, abs(float(cscore[b, i]) - sc[c]) / dsc[c])
                worst_b = max(worst_b, float((np.abs(cbox[b, i] - d["box"][at]) / d["d_box"][at]).max()))
                n += 1
        row0 += 3 * ny * nx
    print("\nMARGIN %-44s %-86s score %.3g box %.3g of the anchor's own bound carried through the decode (%d candidates)" % (kernel, label + " vs float64 decode", worst_s, worst_b, n))
    assert worst_s <= 1.0 and worst_b <= 1.0 and n > 0


def test_fused_detect_epilogue_deep_k(L):
    """Cin = 1024: 32 K-steps, the four-stage ring wraps eight times.  The plain side would split K there (other sums), so the fused candidates are compared with the
    float64 decode at the bound derived in compare_with_float64_decode"""
    label = "5x5 B7 Cin 1024 no 15: the ring wraps"
    dp = DetectPlan(L, 7, [(5, 5, 32)], 1024, 15, WL.PANEL_1X1, 1.0, (3,), seed=1024)
    try:
        runs = [dp.fused(0.25, 128, "igemm<128,64,32,4> 1x1 detect-decode") for _ in range(3)]
        assert all(np.array_equal(r[4], runs[0][4]) for r in runs) and runs[0][4][3] == 0 and runs[0][4].max() <= 128
        sets = [[_by_cidx(r, b, int(r[4][b])) for b in range(7)] for r in runs]
        assert sets[1] == sets[0] and sets[2] == sets[0]
        for b in range(7):
            _assert_untouched_behind(runs[0], b, int(runs[0][4][b]), label)
        compare_with_float64_decode(dp, runs[0], 0.25, label, "igemm<128,64,32,4> 1x1 detect-decode")
    finally:
        dp.close()


def test_fused_detect_epilogue_two_stage_instance(L):
    """more than 4096 pixel tiles keep the two-stage ring: 21 images of 160 x 160 are 4200 tiles; conf_thres leaves a few hundred candidates per image"""
    dp = DetectPlan(L, 21, [(160, 160, 8)], 64, 6, WL.PANEL_1X1, -3.5, (9,), seed=21)
    try:
        assert -(-21 * 160 * 160 // 128) > 4096
        wcount = compare_fused_with_plain(dp, 0.25, 2048, "160x160 B21 Cin 64 no 6, image 9 empty", "igemm<128,64,32,2> 1x1 detect-decode")
        assert wcount[9] == 0 and 50 < np.median(wcount) < 2048 and wcount.max() <= 2048, wcount
        check_plain_heads(dp, "160x160 B21 Cin 64 no 6", "igemm<128,64,32,2> 1x1")
    finally:
        dp.close()


# ------------------------------------------------------------------------------------------------ the listing is complete
def test_every_product_form_has_a_case(request):
    """the kernel names that ran on the device in this session against the hand-written list.  A case adds its name to SEEN only after it has asserted that name and
    passed, so with the whole file run SEEN must BE the list: a form whose case was deleted, skipped or failed is missing here.  Only a run that selects part of the
    file on the command line (-k, a test id, --deselect, --lf, a marker expression other than `gpu`) is excused: there only 'nothing ran that the list does not
    know' can be asserted."""
    assert SEEN <= PRODUCT_FORMS, SEEN - PRODUCT_FORMS
    cfg = request.config
    partial = (cfg.getoption("keyword") or cfg.getoption("markexpr") not in ("", "gpu") or cfg.getoption("deselect") or cfg.getoption("lf", False)
               or any("::" in str(a) for a in cfg.args))
    if not partial:
        assert SEEN == PRODUCT_FORMS, sorted(PRODUCT_FORMS - SEEN)
