"""GPU: augmented inference (test-time augmentation, models/yolo.py:301-317) on the device -- the two kernels of csrc/y7t_tta.hip through the C ABI, and
`model(img, augment=True)` / `Detector.forward_augment` / `Detector.postprocess` on seeded networks small enough that passes share a plan (and its arena).

  1. y7t_tta_scale_layout equals the host build of the same body (tests/_hostsim/tta.py; tests/test_tta_cpu.py holds that one to the reference) bit for bit.
  2. y7t_det_decode_append on planted head tensors of three passes against the restatement (oracle decode + tests/tta_ref.py::transform_ref + the oracle's filter).
  3. passes that share ONE plan: the union candidates are those of three separate runs -- a deferred decode would read the last pass's heads three times.
  4. two and three plans: `decoded()` row blocks, the transform bit for bit, every op of the scaled passes teacher-forced at the project's per-op bound.
  5. one NMS over the union equals the reference walk over the device's own candidates (also with classes / agnostic).
  6. augment=False is the plain path; a different conf_thres raises."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nms_opts_ref, post_scenes as ps, teacher_forced, tta_ref as tr
from tests._hostsim import tta as host

pytestmark = pytest.mark.gpu

TAIL = 4096      # sentinel bytes allocated behind every buffer a kernel writes
CONF = 0.01


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ 1. k_tta_scale_layout
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("geom", tr.GEOMS, ids=tr.GEOM_IDS)
def test_scale_layout_equals_the_host_build(L, geom, kind):
    from yolov7_tracker_amd import _lib
    (H, W), (hs, ws), (Hp, Wp) = geom
    B = 2
    img = tr.source_image(kind, B, H, W, seed=7)
    dev = torch.from_numpy(img).cuda()
    for reorg in (0, 1):
        ld = 16 if reorg else 8
        n = B * (Hp // 2 if reorg else Hp) * (Wp // 2 if reorg else Wp) * ld
        for flip in (0, 2, 3):
            out = torch.full((2 * n + TAIL,), ps.SENTINEL, dtype=torch.uint8, device="cuda")
            _lib.check(L.y7t_tta_scale_layout(_lib.ptr(dev), int(kind == "u8"), B, H, W, flip, hs, ws, Hp, Wp, reorg, _lib.ptr(out), ld, _lib.stream_ptr()))
            torch.cuda.synchronize()
            raw = out.cpu().numpy()
            want = host.scale_layout(img, flip, hs, ws, Hp, Wp, reorg)
            assert np.array_equal(raw[:2 * n].view(np.uint16), want.reshape(-1).view(np.uint16)), (flip, reorg)
            assert (raw[2 * n:] == ps.SENTINEL).all(), "bytes behind the layout tensor were written"


def test_scale_layout_refusals(L):
    from yolov7_tracker_amd import _lib
    img = torch.zeros((1, 3, 8, 8), device="cuda")
    out = torch.zeros(8 * 8 * 16 * 2, dtype=torch.uint8, device="cuda")
    s = _lib.stream_ptr()
    for args in ((1, 8, 8, 1, 6, 6, 8, 8, 0, 8),      # flip 1 is no flip of the reference
                 (1, 8, 8, 0, 9, 6, 8, 8, 0, 8),      # the resampled image leaves the padded one
                 (1, 8, 8, 0, 6, 6, 7, 8, 1, 16),     # ReOrg of an odd size
                 (1, 8, 8, 0, 6, 6, 8, 8, 0, 12)):    # no such layout
        assert L.y7t_tta_scale_layout(_lib.ptr(img), 0, *args[:9], _lib.ptr(out), args[9], s) != 0


# ------------------------------------------------------------------------------------------------ 2. k_decode_append on planted heads
class Append:
    """one workspace of y7t_det_postprocess' layout for B images of `cap` slots, filled by y7t_det_decode_append pass by pass"""

    def __init__(self, L, B, cap):
        self.L, self.B, self.cap = L, B, cap
        self.lay = ps.ws_layout(B, cap)
        self.ws = torch.full((self.lay["total"] + TAIL,), ps.SENTINEL, dtype=torch.uint8, device="cuda")

    def run(self, sc, scale, flip, extent, row_base, first, conf=CONF):
        from yolov7_tracker_amd import _lib
        nl = sc["nl"]
        self._heads = [torch.from_numpy(h).cuda() for h in sc["heads"]]
        hp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in self._heads] + [None] * (4 - nl))
        ny = (ctypes.c_int * 4)(*[s[0] for s in sc["shapes"]] + [0] * (4 - nl))
        nx = (ctypes.c_int * 4)(*[s[1] for s in sc["shapes"]] + [0] * (4 - nl))
        st = (ctypes.c_float * 4)(*[float(v) for v in sc["strides"]] + [0.0] * (4 - nl))
        flat = [float(v) for v in sc["anchors"].ravel()]
        an = (ctypes.c_float * 24)(*(flat + [0.0] * (24 - len(flat))))
        tp = _lib.TtaPass(float(scale), int(flip), float(extent), int(row_base))
        _lib.check(self.L.y7t_det_decode_append(hp, ny, nx, st, an, nl, sc["na"], sc["no"], self.B, float(conf), self.cap, 30000, 0, ctypes.byref(tp), int(first),
                                                _lib.ptr(self.ws), self.lay["total"], _lib.stream_ptr()))
        torch.cuda.synchronize()
        return self.count()

    def bytes(self):
        return self.ws.cpu().numpy()

    def count(self):
        return ps.unpack_candidates(self.bytes(), self.B, self.cap)[4].copy()

    def candidates(self):
        cbox, cscore, ccls, cidx, count = ps.unpack_candidates(self.bytes(), self.B, self.cap)
        return [{"box": cbox[b, :min(n, self.cap)], "score": cscore[b, :min(n, self.cap)], "cls": ccls[b, :min(n, self.cap)], "rows": cidx[b, :min(n, self.cap)]}
                for b, n in enumerate(count)], count.copy()


def _check_rows(got, want, count, cap):
    """one image's candidate slots against the restatement's dict row -> (xyxy, conf, cls, class confidences), at the bar of
    tests/test_postprocess_gpu.py::test_decode_filter_matches_oracle (the transform adds two float32 roundings, far inside it)"""
    n = len(got["rows"])
    rows = got["rows"].tolist()
    assert n == min(int(count), cap) and len(set(rows)) == n and set(rows) <= set(want)
    if count <= cap:
        assert count == len(want) and set(rows) == set(want)
    for j, r in enumerate(rows):
        wbox, wconf, wcls, wvec = want[r]
        top2 = np.sort(wvec)[-2:]
        assert int(got["cls"][j]) == wcls or top2[1] - top2[0] <= 1e-6, r
        np.testing.assert_allclose(got["score"][j], wconf, rtol=1e-5, atol=1e-6, err_msg="row %d score" % r)
        np.testing.assert_allclose(got["box"][j], wbox, rtol=1e-5, atol=1e-4, err_msg="row %d box" % r)


PASS_SETS = {"reference": ((1.0, 0, 0.0), (0.83, 3, 192.0), (0.67, 0, 0.0)), "up-down": ((1.0, 0, 0.0), (0.83, 2, 1280.0), (0.67, 3, 1280.0))}


@pytest.mark.parametrize("passes", sorted(PASS_SETS))
def test_decode_append_matches_the_restatement(L, passes):
    scenes, P = tr.decode_scenes(CONF), PASS_SETS[passes]
    for sc in scenes:      # the restatement alone: no planted score within BAND of conf_thres, so membership is unambiguous
        for obj, conf in ps.scores64(sc["heads"], sc["na"], sc["no"]):
            assert (np.abs(obj - CONF) >= ps.BAND).all() and (np.abs(conf - CONF) >= ps.BAND).all()
    B, total = scenes[0]["B"], sum(sc["A"] for sc in scenes)
    ref = tr.decode_reference_tta(scenes, P, CONF)
    bases = np.cumsum([0] + [sc["A"] for sc in scenes])
    per_pass = [[sum(bases[i] <= r < bases[i + 1] for r in ref[b]) for b in range(B)] for i in range(3)]
    assert all(min(c) > 0 for c in per_pass) and sum(map(sum, per_pass)) < B * total      # some rows pass in every pass, some do not
    ap = Append(L, B, (total + 63) // 64 * 64)
    running = np.zeros(B, np.int64)
    for i, (sc, (scale, flip, extent)) in enumerate(zip(scenes, P)):
        count = ap.run(sc, scale, flip, extent, bases[i], first=i == 0)      # first_pass zeroes the sentinel bytes the counters held; a later pass adds to them
        running += per_pass[i]
        assert count.tolist() == running.tolist(), "count is the running sum after pass %d" % i
    got, count = ap.candidates()
    for b in range(B):
        _check_rows(got[b], ref[b], count[b], ap.cap)
    raw = ap.bytes()
    assert (raw[ap.lay["nsorted"][0]:] == ps.SENTINEL).all(), "the decode pass wrote behind the candidate arrays"
    # the same first pass again with first_pass set: the counters start over
    assert ap.run(scenes[0], *P[0], 0, first=True).tolist() == per_pass[0]
    assert ap.run(scenes[0], *P[0], 0, first=False).tolist() == [2 * c for c in per_pass[0]]


def test_decode_append_overflow(L):
    """every objectness logit at +6 and cap = 64 < the union: the count is every anchor of the passes so far, the first cap slots are real rows with their own box,
    score and class, and nothing else of the workspace is written"""
    scenes, P = tr.decode_scenes(CONF, obj_logit=6.0), PASS_SETS["reference"]
    B = scenes[0]["B"]
    ref = tr.decode_reference_tta(scenes, P, CONF)
    bases = np.cumsum([0] + [sc["A"] for sc in scenes])
    assert all(len(r) == bases[-1] for r in ref) and scenes[0]["A"] > 64
    ap = Append(L, B, 64)
    for i, (sc, (scale, flip, extent)) in enumerate(zip(scenes, P)):
        assert ap.run(sc, scale, flip, extent, bases[i], first=i == 0).tolist() == [bases[i + 1]] * B
    got, count = ap.candidates()
    for b in range(B):
        assert len(got[b]["rows"]) == 64
        _check_rows(got[b], ref[b], count[b], 64)
    assert (ap.bytes()[ap.lay["nsorted"][0]:] == ps.SENTINEL).all()


def test_decode_append_refusals(L):
    from yolov7_tracker_amd import _lib
    sc = tr.decode_scenes(CONF)[0]
    ap = Append(L, sc["B"], 512)
    before = ap.bytes().copy()
    for scale, flip, base in ((0.0, 0, 0), (0.83, 1, 0), (0.83, 3, -1)):
        with pytest.raises(_lib.Y7TError):
            ap.run(sc, scale, flip, 192.0, base, first=True)
    assert np.array_equal(ap.bytes(), before)


# ------------------------------------------------------------------------------------------------ detectors
def _detector(name, hw, B=2, nc=10):
    from yolov7_tracker_amd.detector import arch, model
    det = model.Detector(arch.ARCHS[name](nc), None, img_size=hw, max_batch=B, seed=0)
    img = torch.rand((B, 3) + tuple(hw), generator=torch.Generator().manual_seed(hw[0] + hw[1]))
    return det, img


def _run_pass(det, img, ratio, flip):
    """ONE pass on its own, as forward_augment runs it: the scaled input into buffer 0 of the plan of its size, then the plain launch list.  -> padded size"""
    from yolov7_tracker_amd import _lib
    B, _, H, W = img.shape
    (hs, ws), pad = tr.pass_sizes(H, W, ratio, int(det.stride.max()))
    det._select(pad)
    p = det.plan
    dev = img.cuda().contiguous()
    _lib.check(det._L.y7t_tta_scale_layout(_lib.ptr(dev), 0, B, H, W, int(flip or 0), hs, ws, pad[0], pad[1], int(p.reorg), _lib.ptr(p.arena), p.in_ld, _lib.stream_ptr()))
    det._run_ops(B, 0, -1, None, 0)
    torch.cuda.synchronize()
    return pad


def _xyxy_transform(box, ratio, flip, extent):
    """candidate corners of a pass on its own -> the corners after the pass's transform: back to xywh, tests/tta_ref.py::transform_ref, corners again"""
    c = np.stack([(box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2, box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]], 1).astype(np.float32)
    c = tr.transform_ref(c, ratio, flip, extent)
    return np.stack([c[:, 0] - c[:, 2] / 2, c[:, 1] - c[:, 3] / 2, c[:, 0] + c[:, 2] / 2, c[:, 1] + c[:, 3] / 2], 1)


# ------------------------------------------------------------------------------------------------ 3. arena sharing
@pytest.mark.parametrize("name,hw", [("yolov7-w6", (64, 64)), ("yolov7-tiny", (64, 96))])
def test_passes_that_share_a_plan_are_decoded_one_by_one(name, hw):
    from yolov7_tracker_amd.detector import model
    det, img = _detector(name, hw)
    B, (H, W) = img.shape[0], hw
    gs = int(det.stride.max())
    assert [tr.pass_sizes(H, W, r, gs)[1] for r in tr.SCALES] == [hw] * 3 and tr.TABLE[(gs, hw)][2][1] == hw      # three passes, one plan, one arena
    out = det(img, augment=True)[0]
    torch.cuda.synchronize()
    assert isinstance(out, model.AugmentedOutput) and len(det._plans) == 1
    got = [t.cpu().numpy().copy() for t in out.candidate_arrays()]
    A = out.rows[0]
    assert out.rows == [A] * 3 and out.shape[1] == 3 * A
    want = [dict() for _ in range(B)]
    for i, (ratio, flip) in enumerate(zip(tr.SCALES, tr.FLIPS)):
        _run_pass(det, img, ratio, flip)
        det.postprocess(model.HeadOutput(det, B, hw), CONF, 0.45, None)      # the decode pass of the plain chain: its candidate arrays
        cbox, cscore, ccls, cidx, count = [t.cpu().numpy() for t in det.candidate_arrays(0, B)]
        for b in range(B):
            n = int(count[b])
            assert 0 < n <= A
            box = _xyxy_transform(cbox[b, :n], ratio, flip, W if flip == 3 else H)
            for j in range(n):
                want[b][i * A + int(cidx[b, j])] = (box[j], cscore[b, j], ccls[b, j])
    distinct = 0
    for b in range(B):
        n = int(got[4][b])
        rows = got[3][b, :n].tolist()
        assert n == len(want[b]) and len(set(rows)) == n and set(rows) == set(want[b]), "image %d: the union of the three separate runs" % b
        for j, r in enumerate(rows):
            wbox, wscore, wcls = want[b][r]
            assert got[1][b, j] == wscore and got[2][b, j] == wcls, (b, r)      # the same functions on the same logits
            np.testing.assert_allclose(got[0][b, j], wbox, rtol=1e-5, atol=1e-4, err_msg="image %d row %d" % (b, r))
        distinct += sum(want[b][r][1] != want[b][2 * A + r][1] for r in range(A) if r in want[b] and 2 * A + r in want[b])
    assert distinct, "no row scores differently in the first and the last pass: the test would not see a deferred decode"


# ------------------------------------------------------------------------------------------------ 4. two and three plans
@pytest.mark.parametrize("name,hw,plans", [("yolov7-w6", (256, 256), 2), ("yolov7-tiny", (128, 192), 3)])
def test_decoded_rows_transform_and_teacher_forced_passes(name, hw, plans):
    from yolov7_tracker_amd.detector import model
    det, img = _detector(name, hw)
    B, (H, W) = img.shape[0], hw
    out = det(img, augment=True)[0]
    dec = out.decoded().cpu().numpy()
    assert len(det._plans) == plans and dec.shape == (B, sum(out.rows), det.plan.det["no"]) == tuple(out.shape)
    pads = [p for _, p in tr.TABLE[(int(det.stride.max()), hw)]]
    assert out.rows == [sum(det.plan.det["na"] * (p[0] // s) * (p[1] // s) for s in det.stride.int().tolist()) for p in pads]
    plain = det(img)[0]
    assert (det.plan.H, det.plan.W) == hw      # the augmented forward left the detector on the first pass's plan
    assert np.array_equal(dec[:, :out.rows[0]], plain.decoded().cpu().numpy())
    base = out.rows[0]
    for i in (1, 2):
        ratio, flip = tr.SCALES[i], tr.FLIPS[i]
        pad = _run_pass(det, img, ratio, flip)
        assert pad == pads[i]
        own = model.HeadOutput(det, B, pad).decoded().cpu().numpy()      # the device's own heads of this pass, decoded
        own[..., :4] = tr.transform_ref(own[..., :4], ratio, flip, W if flip == 3 else H)
        assert np.array_equal(dec[:, base:base + out.rows[i]].view(np.uint32), own.view(np.uint32)), "pass %d: de-scale / de-flip bit for bit" % i
        base += out.rows[i]
        # teacher-forced: the device's fp16 scaled input of this pass through the oracle, every op at the bound a plain forward of this graph is held to
        p = det.plan
        x0 = det.buffer_view(0, B, p.in_ld).view(B, p.H // 2 if p.reorg else p.H, p.W // 2 if p.reorg else p.W, p.in_ld)[..., :12 if p.reorg else 3]
        x0 = x0.float().cpu().permute(0, 3, 1, 2).contiguous()
        want0 = host.scale_layout(img.numpy(), flip or 0, *tr.pass_sizes(H, W, ratio, int(det.stride.max()))[0], pad[0], pad[1], int(p.reorg))
        assert np.array_equal(x0.permute(0, 2, 3, 1).numpy().astype(np.float16).view(np.uint16), want0[..., :x0.shape[1]].view(np.uint16))
        names = det.launch_list(B)
        _run_pass(det, img, ratio, flip)      # launch_list re-ran the ops in place: a clean pass again
        r = teacher_forced.check_every_op(det, B, [0], x0[:1], names)
        assert r["visited"] == list(range(len(p.ops)))


def test_uint8_frames_pass_zero_through_the_fused_stem():
    """w6 on uint8 BGR frames: pass 0 enters as the plain forward does (the fused frame -> stem kernel), so its rows are the plain forward's; the scaled passes convert
    the frame as the input layout does, so their rows are those of the float image the frame stands for"""
    det, _ = _detector("yolov7-w6", (64, 64))
    frames = torch.from_numpy(tr.source_image("u8", 2, 64, 64, seed=3))
    assert det.plan.stem_fused and det.plan.reorg
    aug8 = det(frames.cuda(), augment=True)[0]
    d8 = aug8.decoded().cpu().numpy()
    A0 = aug8.rows[0]
    assert np.array_equal(d8[:, :A0], det(frames.cuda())[0].decoded().cpu().numpy())
    d32 = det(torch.from_numpy(tr.float_image(frames.numpy())), augment=True)[0].decoded().cpu().numpy()
    assert np.array_equal(d8[:, A0:], d32[:, A0:])


# ------------------------------------------------------------------------------------------------ 5. one NMS over the union
@pytest.mark.parametrize("classes,agnostic", [(None, False), ([0, 2], True)])
def test_nms_over_the_union_is_the_reference_walk(classes, agnostic):
    det, img = _detector("yolov7-tiny", (128, 192))
    B, (H, W) = img.shape[0], (128, 192)
    out = det.forward_augment(img, conf_thres=CONF)
    dets, nd = det.postprocess(out, CONF, 0.45, None, classes=classes, agnostic=agnostic)
    torch.cuda.synchronize()
    cbox, cscore, ccls, cidx, count = [t.cpu().numpy() for t in out.candidate_arrays()]
    dets, nd, keep = dets.cpu().numpy(), nd.cpu().numpy(), out.aug.keep.cpu().numpy()
    assert out._kept is None
    for b in range(B):
        n = int(count[b])
        assert 0 < n <= sum(out.rows) and cidx[b, :n].min() < out.rows[0] and cidx[b, :n].max() >= out.rows[0] + out.rows[1], "candidates of the first and the last pass"
        scene = {"box": cbox[b, :n], "score": cscore[b, :n], "cls": ccls[b, :n], "rows": cidx[b, :n]}
        ref = nms_opts_ref.walk(scene, 0.45, classes=classes, agnostic=agnostic)
        if classes is None:
            assert np.array_equal(ref, ps.reference_walk(scene, 0.45))
        k = int(nd[b])
        assert k == len(ref) > 0
        np.testing.assert_array_equal(keep[b, :k], ref, err_msg="image %d: kept slots" % b)
        np.testing.assert_array_equal(cidx[b, keep[b, :k]], cidx[b, ref], err_msg="image %d: kept rows" % b)
        np.testing.assert_array_equal(dets[b, :k], ps.expected_rows(scene, ref, (1.0, 0.0, 0.0, float(H), float(W))), err_msg="image %d: rows" % b)
        if classes is not None:
            assert set(dets[b, :k, 5].tolist()) <= {0.0, 2.0}


def test_non_max_suppression_takes_the_augmented_output():
    """the reference's seam: non_max_suppression(model(img, augment=True)[0], ...) -> per image (n, 6) [xyxy un-rounded, conf, cls], the rows postprocess keeps"""
    from yolov7_tracker_amd.detector import non_max_suppression
    det, img = _detector("yolov7-tiny", (64, 96))
    out = det(img, augment=True)[0]
    res = non_max_suppression(out, conf_thres=CONF, iou_thres=0.45)
    cbox = out.candidate_arrays()[0].cpu().numpy()
    nd, keep, dets = out.aug.ndets.cpu().numpy(), out.aug.keep.cpu().numpy(), out.aug.dets.cpu().numpy()
    assert len(res) == img.shape[0]
    for b, r in enumerate(res):
        r = r.cpu().numpy()
        assert len(r) == nd[b] > 0 and np.array_equal(r[:, :4], cbox[b, keep[b, :nd[b]]]) and np.array_equal(r[:, 4:], dets[b, :nd[b], 4:])
    with pytest.raises(ValueError):
        non_max_suppression(out, conf_thres=CONF, multi_label=True)


# ------------------------------------------------------------------------------------------------ 6. the plain path is untouched
def test_augment_false_is_the_plain_forward_and_conf_thres_is_fixed_at_the_forward():
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.detector import model
    det, img = _detector("yolov7-tiny", (64, 96))
    a = det(img)[0]
    da = a.decoded().cpu()
    b = det(img, augment=False)[0]
    assert type(a) is model.HeadOutput and type(b) is model.HeadOutput and torch.equal(da, b.decoded().cpu())
    out = det(img, augment=True)[0]
    assert isinstance(out, model.AugmentedOutput) and out.decoded().shape[1] == 3 * da.shape[1]
    with pytest.raises(ValueError):
        det.postprocess(out, 0.25, 0.45, None)
    det.postprocess(out, CONF, 0.45, None)
    with pytest.raises(_lib.Y7TError):
        out.raw()
    later = det.forward_augment(img)
    with pytest.raises(_lib.Y7TError):      # the set now holds the later forward's candidates
        det.postprocess(out, CONF, 0.45, None)
    with pytest.raises(_lib.Y7TError):
        later.decoded()                     # not kept unless asked for
