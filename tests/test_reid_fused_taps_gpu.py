"""GPU: csrc/y7t_reid_fused.hip::k_osnet_x025 TENSOR BY TENSOR.  The kernel's TAP instance (the same source with TAP == true; measuring build only, bound here with
ctypes) copies every tensor a phase stores -- the crop, the stem, the maxpool, per OSBlock x1, the haloed U and T of the ten lights, the pooled partials and the gate
of the four streams and the block output, both transitions, conv5, the pooled vector, the feature -- from LDS to a per-crop tap buffer; each is held against the
teacher-forced float64 reference of tests/reid_fused_ref.py (pinned on the CPU by tests/test_reid_fused_ref_cpu.py, where the same bars catch planted faults that
the whole-network bars let through).  The tap instance's features equal the product library's bit for bit, which ties the taps to the shipped kernel.

Inputs: the edge frames and boxes of tests/test_reid_gpu.py (1-px boxes, the whole frame, boxes at and over the edge, fractional corners, empty crops = a network of
biases), once on the synthetic frame and once as a batch over the three noise frames with a shuffled frame index; weights (A) the suite's seed 3 and (B) the same
with the gate weights times 6, for which the gates leave the 0.35-0.61 band (asserted on the float64 reference).

Every comparison prints a `MARGIN` line (profiles/reid_fused_taps_margins.txt keeps the table of one run)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import reid_fused_ref as FR
from tests.test_reid_gpu import _edge_boxes, _edge_frames

pytestmark = pytest.mark.gpu

SLACK = 4096
SENTINEL = 0x5A


class Tap(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 40), ("offset", ctypes.c_longlong), ("dtype", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("c", ctypes.c_int),
                ("pitch", ctypes.c_int)]


@pytest.fixture(scope="module")
def abl():
    """the measuring build, for its two tap entry points (not part of include/y7t.h)"""
    from yolov7_tracker_amd import _lib, build
    _lib.require_gpu()
    L = ctypes.CDLL(build.LIB_ABLATE)
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.y7t_reid_fused_tap_layout.restype, L.y7t_reid_fused_tap_layout.argtypes = ci, [vp, ci, vp]
    L.y7t_reid_fused_taps.restype, L.y7t_reid_fused_taps.argtypes = ci, [vp, ci, ci, ci, vp, vp, ci, vp, ll, vp, vp, ll, vp]
    L.y7t_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def layout(abl):
    stride = ctypes.c_longlong()
    n = abl.y7t_reid_fused_tap_layout(None, 0, ctypes.byref(stride))
    table = (Tap * n)()
    assert abl.y7t_reid_fused_tap_layout(table, n, ctypes.byref(stride)) == n
    rows = [(t.name.decode(), t.offset, t.dtype, t.h, t.w, t.c, t.pitch) for t in table]
    assert rows[0][0] == "CR" and rows[-1][0] == "walked" and stride.value % 16 == 0 and len({r[0] for r in rows}) == n == 3 + 6 * 30 + 4 + 4
    return rows, stride.value


def scene(mode):
    """-> frames (B, H, W, 3) uint8, boxes (N, 4), frame index (N) or None"""
    noise, syn = _edge_frames()
    if mode == "frame":                                  # the synthetic 96 x 96 frame, every box once
        return syn[None], np.concatenate(_edge_boxes(96, 96)), None
    one = np.concatenate(_edge_boxes(96, 80))            # every box from every noise frame, rows in a shuffled order (test_fused_crop_stage_at_the_edges)
    order = np.random.default_rng(12).permutation(3 * len(one))
    return noise, np.concatenate([one] * 3)[order], ((np.arange(3 * len(one)) // len(one) + np.arange(3 * len(one))) % 3).astype(np.int32)[order]


def state_dict(weights):
    return FR.gate_scaled_state_dict(1 if weights == "A" else FR.GATE_FACTOR)


class Run:
    """one launch of the tap instance and of the product kernel on the same crops and weights, and every comparison of staged()"""

    def __init__(self, abl, layout, weights, mode):
        from yolov7_tracker_amd import _lib
        from yolov7_tracker_amd.tracker import reid
        rows, stride = layout
        frames, boxes, idx = scene(mode)
        self.frames, self.boxes, self.idx = frames, boxes, (idx if idx is not None else np.zeros(len(boxes), np.int32))
        n = len(boxes)
        self.sd = state_dict(weights)
        product = reid.ReIDExtractor(self.sd, max_crops=64)
        assert product.fused
        blob = reid.pack_fused(self.sd, product.spec)
        d_blob, d_frames, d_boxes = torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(frames).cuda().contiguous(), torch.from_numpy(boxes).cuda().contiguous()
        d_idx = torch.from_numpy(idx).cuda() if idx is not None else None
        d_taps = torch.full((n * stride + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_feats = torch.full((n * 512 + 64,), 7.0, dtype=torch.float32, device="cuda")
        rc = abl.y7t_reid_fused_taps(_lib.ptr(d_frames), frames.shape[0], frames.shape[1], frames.shape[2], _lib.ptr(d_boxes), _lib.ptr(d_idx), n, _lib.ptr(d_blob),
                                     d_blob.numel(), _lib.ptr(d_feats), _lib.ptr(d_taps), n * stride, _lib.stream_ptr())
        assert rc == 0, abl.y7t_last_error()
        torch.cuda.synchronize()
        raw = d_taps.cpu().numpy()
        assert (raw[n * stride:] == SENTINEL).all() and bool((d_feats[n * 512:] == 7.0).all())
        self.taps = FR.decode_taps(raw[:n * stride].reshape(n, stride), rows)
        self.walked_offset = [r[1] for r in rows if r[0] == "walked"][0]
        self.tap_feats = d_feats[:n * 512].view(n, 512).cpu().numpy()
        if idx is None:
            self.product_feats = product.features_for_boxes(frames[0], boxes).cpu().numpy()
        else:
            self.product_feats = product.features_for_frames(d_frames, boxes, idx).cpu().numpy()
        self.P = FR.decode_blob(blob)
        self.rows = [(fam, name) + FR.worst(got, ref, bar) for fam, name, got, ref, bar in FR.staged(self.P, frames, boxes, self.idx, self.taps)]


_runs = {}


@pytest.fixture
def run(abl, layout, request):
    key = request.param
    if key not in _runs:
        _runs[key] = Run(abl, layout, *key)
    return _runs[key]


CASES = [(w, m) for w in "AB" for m in ("frame", "batch")]
case_ids = ["%s-%s" % c for c in CASES]


@pytest.mark.parametrize("family", FR.FAMILIES)
@pytest.mark.parametrize("run", CASES, ids=case_ids, indirect=True)
def test_tapped_tensors_within_their_bars(run, family, request):
    """every tapped tensor of every crop of one family (FR.FAMILIES: the phase a failure names) within the bar of its single op"""
    rows = [r for r in run.rows if r[0] == family]
    assert rows
    case = request.node.callspec.id.rsplit("-", 1)[0]
    for fam, name, ok, w in rows:
        print("MARGIN %-10s %-36s %-8s %s" % (fam, name, case, "exact" if (family in ("zeros", "maxpool") and ok) else "worst err/bar %.3f" % w))
    bad = [(name, w) for fam, name, ok, w in rows if not ok]
    assert not bad, bad[:6]


@pytest.mark.parametrize("run", CASES, ids=case_ids, indirect=True)
def test_tap_instance_is_the_shipped_kernel(run):
    """the tap instance's features == the product library's (features_for_boxes / features_for_frames) on the same crops and weights, bit for bit: one source, and the
    taps only read; the feature in the tap buffer is the one written out; the kernel walked its tap buffer exactly as the layout table says"""
    assert np.isfinite(run.tap_feats).all() and float(np.abs(run.tap_feats).max()) > 0.05
    assert np.array_equal(run.tap_feats.view(np.uint32), run.product_feats.view(np.uint32)), int((run.tap_feats != run.product_feats).sum())
    assert np.array_equal(run.taps["feats"].reshape(-1, 512).view(np.uint32), run.tap_feats.view(np.uint32))
    assert (run.taps["walked"] == run.walked_offset).all()


def float64_trace(run):
    """the float64 network of the staged references on the oracle's crops -> its features and, per block, gates and hidden pre-activations"""
    from oracle import reid_torch
    x = np.zeros((len(run.boxes), 3, 128, 64), np.float32)
    for i, (b, f) in enumerate(zip(run.boxes, run.idx)):
        Hf, Wf = run.frames.shape[1:3]
        if min(max(int(b[2]), 0), Wf) > min(max(int(b[0]), 0), Wf) and min(max(int(b[3]), 0), Hf) > min(max(int(b[1]), 0), Hf):
            x[i] = reid_torch.preprocess(run.frames[int(f)], b[None]).numpy()[0]
    trace = {}
    FR.chain(run.P, x, trace)
    return x, trace


@pytest.mark.parametrize("run", [("B", "frame"), ("B", "batch")], ids=["B-frame", "B-batch"], indirect=True)
def test_weights_b_open_the_gates_and_the_product_path_holds(run):
    """weights (B) do what they are for -- on the float64 reference, not on the device: in every block some gate is below 0.15 and some above 0.75, and in stage 4
    each of the two hidden units is positive for some crop and stream.  And the product path, no taps, on these weights: features against the float64 oracle at the
    bars of test_fused_osnet_kernel_matches_oracle (3e-3 of max|feature|, cosine >= 1 - 1e-5)"""
    from oracle import reid_torch
    x, trace = float64_trace(run)
    for name, (gates, hidden) in trace.items():
        g, h = np.stack(gates), np.stack(hidden)
        print("weights B %s: gates %.3f .. %.3f, hidden units positive somewhere: %s" % (name, g.min(), g.max(), (h > 0).any((0, 1))))
        assert g.min() < 0.15 and g.max() > 0.75, name
        if name.startswith("conv4"):
            assert h.shape[-1] == 2 and (h > 0).any((0, 1)).all(), name
    want = reid_torch.osnet_forward(run.sd, torch.from_numpy(x), dtype=torch.float64).numpy()
    got = run.product_feats.astype(np.float64)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max() / scale)
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    print("product path, weights B: max err %.2e of the feature scale, min cosine 1 - %.1e" % (err, 1 - cos.min()))
    assert np.isfinite(got).all() and float(np.abs(want).mean()) > 0.05
    assert err <= 3e-3, err
    assert cos.min() >= 1 - 1e-5, cos.min()
