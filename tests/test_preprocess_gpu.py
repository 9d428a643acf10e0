"""GPU: the samplers that read the uint8 frame, value by value, at the geometries of tests/preproc_ref.py::GEOMETRIES.

  k_letterbox_layout (csrc/y7t_post.hip, y7t_letterbox_layout_u8), ReOrg'd / 16 channels and plain / 8 channels:
      == the float32 restatement (oracle/letterbox_np.py, == the host loader: tests/test_preprocess_cpu.py) bit for bit as fp16 -- both files are compiled without
      FMA contraction, so the kernel is the same sequence of IEEE float32 operations; and, independently of that claim, == rint(v) / 255 on every pixel the
      float64 formula decides.  Padding channels zero, nothing written behind the last pixel, bad arguments refused.
  k_stem_u8 (csrc/y7t_stem.hip, y7t_det_forward_stem_u8 on a yolov7-w6 plan with random weights), both instantiations, op 0's output buffer:
      == stand-alone letterbox + layout followed by op 0 of the plan built with Y7T_STEM_FUSED=0, bit for bit; within tests/teacher_forced.py's convolution
      tolerance of the oracle's stem conv on the float32 restatement's tensor.  The two nine-frame rows give 256 of the 2048 workgroups a second tile.
A `PREPROC` line per case (pytest -s) names the geometry, the kernel and the counts; profiles/preprocess_tests.txt keeps one run."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import preproc_ref as pr
from tests.preproc_ref import GEOMETRIES, KINDS

pytestmark = pytest.mark.gpu

Y7T_E_ARG = -1
SENTINEL = 0x5A5B       # an fp16 bit pattern (203.4) no layout value takes: they lie in [0, 1]
TAIL = 4096             # guard elements behind the last pixel
STEM_ROWS = [r for r in GEOMETRIES if r.stem is not None]
MAX_B = max(r.B for r in STEM_ROWS)


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


_REF = {}


def reference(row, kind):
    """computed once per (row, kind) and shared, never modified: frames, the float32 restatement's letterboxed images, and per frame the letterboxed rint(v) of
    the float64 formula with its decided mask (None for rows that are not resampled)"""
    key = (row.name, kind)
    if key not in _REF:
        frames = pr.frames_for(row, kind)
        H, W, new_h, new_w, top, left = row.geom
        imgs = np.stack([pr.letterbox_f32(f, row.img_size, row.stride) for f in frames])
        assert imgs.shape == (row.B, H, W, 3)
        f64 = None
        if row.resampled:
            want = np.full((row.B, H, W, 3), 114, np.uint8)
            dec = np.ones((row.B, H, W, 3), bool)
            for b, f in enumerate(frames):
                v, delta = pr.resize_f64(f, new_h, new_w)
                want[b, top:top + new_h, left:left + new_w] = np.rint(v).astype(np.uint8)
                dec[b, top:top + new_h, left:left + new_w] = pr.decided(v, delta)
            f64 = (want, dec)
        for a in (frames, imgs) + (f64 or ()):
            a.setflags(write=False)
        _REF[key] = (frames, imgs, f64)
    return _REF[key]


def run_letterbox(L, frames_dev, row, reorg, ldout, geom=None):
    """y7t_letterbox_layout_u8 into a sentinel-filled buffer -> (return code, the buffer as int16 bit patterns on the host, number of output values)"""
    from yolov7_tracker_amd import _lib
    H, W, new_h, new_w, top, left = geom or row.geom
    B, (H0, W0) = frames_dev.shape[0], row.shape
    n = B * (H // 2 if reorg else H) * (W // 2 if reorg else W) * ldout
    out = torch.full((n + TAIL,), SENTINEL, dtype=torch.int16, device="cuda")
    rc = L.y7t_letterbox_layout_u8(_lib.ptr(frames_dev), B, H0, W0, H, W, new_h, new_w, top, left, int(reorg), _lib.ptr(out), ldout, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), n


@pytest.mark.parametrize("reorg,ldout", [(1, 16), (0, 8)], ids=["reorg16", "plain8"])
@pytest.mark.parametrize("row", GEOMETRIES, ids=repr)
def test_letterbox_layout_kernel(L, row, reorg, ldout):
    H, W, new_h, new_w, top, left = row.geom
    assert H % 2 == 0 and W % 2 == 0
    Ho, Wo, creal = (H // 2, W // 2, 12) if reorg else (H, W, 3)
    for kind in KINDS:
        frames, imgs, f64 = reference(row, kind)
        fd = torch.from_numpy(frames.copy()).cuda()
        rc, raw, n = run_letterbox(L, fd, row, reorg, ldout)
        assert rc == 0
        assert (raw[n:] == SENTINEL).all(), "written behind the last pixel"
        got = raw[:n].reshape(row.B, Ho, Wo, ldout)
        assert (got[..., creal:] == 0).all(), "padding channels"
        want = np.stack([pr.layout_tensor(im, reorg) for im in imgs])
        n_diff = int((got[..., :creal] != want.view(np.int16)).sum())
        n_und = n_dec_off = 0
        if f64 is not None:
            want64, dec = f64
            t64 = np.stack([pr.layout_tensor(im, reorg) for im in want64])
            dmask = np.stack([pr.layout_tensor(d.astype(np.uint8) * 255, reorg) for d in dec]) > 0.5      # the decided mask through the same permutation
            n_und = int((~dmask).sum())
            n_dec_off = int(((got[..., :creal] != t64.view(np.int16)) & dmask).sum())
        print("PREPROC %-14s %-6s %dx%d -> %s  k_letterbox_layout reorg=%d ldout=%d  B=%d  != float32 restatement: %d of %d  undecided %.3f %%  decided != rint(v): %d" % (
            row.name, kind, row.shape[0], row.shape[1], row.geom, reorg, ldout, row.B, n_diff, want.size, 100.0 * n_und / want.size, n_dec_off))
        assert n_dec_off == 0, "%d decided values differ from rint(v) / 255" % n_dec_off
        assert n_diff == 0, "%d values differ from the float32 restatement" % n_diff
        if not row.resampled:       # the same tensor as the plain layout kernel on the host-padded frame
            from yolov7_tracker_amd import _lib
            padded = torch.from_numpy(imgs.copy()).cuda()
            out2 = torch.full((n,), SENTINEL, dtype=torch.int16, device="cuda")
            _lib.check(L.y7t_input_layout(_lib.ptr(padded), 1, row.B, H, W, int(reorg), _lib.ptr(out2), ldout, _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert np.array_equal(out2.cpu().numpy(), raw[:n])


def test_letterbox_layout_refusals(L):
    """Y7T_E_ARG, and not a byte written"""
    row = pr.ROWS["157x211"]
    H, W, new_h, new_w, top, left = row.geom
    fd = torch.from_numpy(pr.frames_for(row, "noise")).cuda()
    for what, geom, reorg, ldout in [("top + new_h > H", (H, W, new_h, new_w, H - new_h + 1, left), 1, 16), ("left + new_w > W", (H, W, new_h, new_w, top, 1), 1, 16),
                                     ("ldout 12", row.geom, 0, 12), ("ldout 24", row.geom, 1, 24), ("reorg needs 16 channels", row.geom, 1, 8),
                                     ("reorg with odd H", (H + 1, W, new_h, new_w, top, left), 1, 16), ("reorg with odd W", (H, W + 1, new_h, new_w, top, left), 1, 16)]:
        rc, raw, _ = run_letterbox(L, fd, row, reorg, ldout, geom)
        assert rc == Y7T_E_ARG, what
        assert (raw == SENTINEL).all(), what


# ------------------------------------------------------------------------------------------------------------------------ fused stem
class Stems:
    """one yolov7-w6 detector with random weights per way of building it (fused stem / Y7T_STEM_FUSED=0), same weights; plans cached per (H, W) inside"""

    def __init__(self):
        from yolov7_tracker_amd.detector import arch, model
        self.fused = model.Detector(arch.ARCHS["yolov7-w6"](10), None, img_size=(64, 64), max_batch=MAX_B, seed=5)
        old = os.environ.get("Y7T_STEM_FUSED")
        os.environ["Y7T_STEM_FUSED"] = "0"
        try:
            self.plain = model.Detector(arch.ARCHS["yolov7-w6"](10), self.fused._sd, img_size=(64, 64), max_batch=MAX_B)
            for hw in sorted({r.geom[:2] for r in STEM_ROWS}):
                self.plain._select(hw)
        finally:
            if old is None:
                del os.environ["Y7T_STEM_FUSED"]
            else:
                os.environ["Y7T_STEM_FUSED"] = old

    def select(self, hw):
        self.fused._select(hw)
        self.plain._select(hw)
        assert self.fused.plan.stem_fused and not self.plain.plan.stem_fused
        return self.fused, self.plain


@pytest.fixture(scope="module")
def stems():
    return Stems()


def op0_out(det, B):
    """(view of op 0's whole output buffer, view of the tensor in it as (B, Ho, Wo, Cout))"""
    op = det.plan.ops[0]
    buf = det.buffer_view(int(op["out_buf"]), B, int(op["out_ld"]))
    t = buf.view(B, int(op["Ho"]), int(op["Wo"]), int(op["out_ld"]))[..., int(op["out_coff"]):int(op["out_coff"]) + int(op["Cout"])]
    return buf, t


@pytest.mark.parametrize("row", STEM_ROWS, ids=repr)
def test_fused_stem(L, stems, row):
    from oracle import detector_torch as dt
    from tests.teacher_forced import conv_tolerance
    from yolov7_tracker_amd import _lib
    H, W, new_h, new_w, top, left = row.geom
    B, (H0, W0) = row.B, row.shape
    det, plain = stems.select((H, W))
    op, wl = det.plan.ops[0], det.plan.wlayout[0]
    assert int(op["type"]) == 0 and wl["kind"] == "conv" and (int(op["H"]), int(op["W"])) == (H // 2, W // 2) and int(op["in_buf"]) == 0
    k, s_, pd = int(op["KH"]), int(op["stride"]), int(op["pad"])
    for kind in KINDS:
        frames, imgs, _ = reference(row, kind)
        fd = torch.from_numpy(frames.copy()).cuda()
        buf, view = op0_out(det, B)
        runs = []
        for _ in range(2 if B > 1 else 1):       # a second run into a cleared buffer: the patch ring carries no state
            buf.zero_()
            _lib.check(L.y7t_det_forward_stem_u8(det.plan.handle, _lib.ptr(fd), B, H0, W0, new_h, new_w, top, left, _lib.stream_ptr()))
            name = L.y7t_last_kernel().decode()
            torch.cuda.synchronize()
            runs.append(view.clone())
        assert name == row.stem, name
        got = runs[0]
        assert all(torch.equal(got, r) for r in runs[1:]), "two runs differ"
        # the three-step path of the plan built without the fused stem: stand-alone letterbox + layout, then op 0
        pbuf, pview = op0_out(plain, B)
        pbuf.zero_()
        _lib.check(L.y7t_letterbox_layout_u8(_lib.ptr(fd), B, H0, W0, H, W, new_h, new_w, top, left, 1, _lib.ptr(plain.plan.arena), 16, _lib.stream_ptr()))
        _lib.check(L.y7t_det_forward_ops(plain.plan.handle, B, 0, 1, _lib.stream_ptr()))
        torch.cuda.synchronize()
        n_diff = [int((got[b] != pview[b]).sum()) for b in range(B)]
        # the oracle's stem conv on the float32 restatement's tensor
        x0 = torch.from_numpy(np.stack([pr.layout_tensor(im, 1) for im in imgs]).astype(np.float32)).permute(0, 3, 1, 2).contiguous()
        ref = dt._conv_bn_act(x0, det._sd, wl["wkey"], k, s_, pd, wl["act"], fp16=True, round_out=False).permute(0, 2, 3, 1)
        absum = dt.conv_abs_sum(x0, det._sd, wl["wkey"], s_, pd).permute(0, 2, 3, 1)
        tol = conv_tolerance(ref, absum, int(op["Cin"]) * k * k)
        ratio = ((got.float().cpu() - ref).abs() / tol).flatten(1).max(1).values
        print("PREPROC %-14s %-6s %dx%d -> %s  %s  B=%d  != letterbox + layout + op 0: %d  worst err/tol per frame %s" % (
            row.name, kind, H0, W0, row.geom, name, B, sum(n_diff), " ".join("%.3f" % float(v) for v in ratio)))
        assert float(got.abs().max()) > 0
        assert sum(n_diff) == 0, "frames %s differ from the unfused path" % [b for b in range(B) if n_diff[b]]
        assert float(ratio.max()) <= 1.0, "frame %d: err / tol %.2f" % (int(ratio.argmax()), float(ratio.max()))


def test_stem_refusals(L, stems):
    """y7t_det_forward_stem_u8 returns Y7T_E_ARG and writes nothing: the resized image does not fit the plan's input; a plan whose image is no multiple of 32"""
    from yolov7_tracker_amd import _lib
    row = pr.ROWS["157x211"]
    H, W, new_h, new_w, top, left = row.geom
    det, _ = stems.select((H, W))
    fd = torch.from_numpy(pr.frames_for(row, "noise")).cuda()
    buf, _v = op0_out(det, 1)
    buf.fill_(7.0)
    for what, g in [("top + new_h > H", (new_h, new_w, H - new_h + 1, left)), ("left + new_w > W", (new_h, new_w, top, 1))]:
        assert L.y7t_det_forward_stem_u8(det.plan.handle, _lib.ptr(fd), 1, row.shape[0], row.shape[1], g[0], g[1], g[2], g[3], _lib.stream_ptr()) == Y7T_E_ARG, what
    # the same plan with op 0 on a 40 x 64 map (an 80 x 128 image: H & 31 = 16); the call is refused before anything of it is used
    p = det.plan
    ops = p.ops.copy()
    ops["H"][0] = ops["Ho"][0] = 40
    h = ctypes.c_void_p()
    _lib.check(L.y7t_det_create(ops.ctypes.data_as(ctypes.c_void_p), len(ops), p.buf_offsets.ctypes.data_as(ctypes.c_void_p), len(p.buf_offsets), _lib.ptr(p.arena),
                                p.arena_bytes, _lib.ptr(p.w_dev), _lib.ptr(p.b_dev), 1, ctypes.byref(h)))
    try:
        assert L.y7t_det_stem_fusable(h) == 0
        small = torch.zeros((1, 80, 128, 3), dtype=torch.uint8, device="cuda")
        assert L.y7t_det_forward_stem_u8(h, _lib.ptr(small), 1, 80, 128, 80, 128, 0, 0, _lib.stream_ptr()) == Y7T_E_ARG
    finally:
        L.y7t_det_destroy(h)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
