"""y7t_det_postprocess_ex through the C ABI: non_max_suppression's `classes`, `agnostic` and `multi_label` on the device (k_decode_filter_ml, k_rank_sort<true> and the
unchanged k_nms_keep of csrc/y7t_post.hip), in the pattern of tests/test_postprocess_gpu.py -- planted candidates, sentinel-filled outputs, the bytes behind the
workspace checked -- against the restatement of tests/nms_opts_ref.py.  Comparisons on planted candidates are exact: ndets, the kept slots, all six columns, nothing
written past ndets.  tests/test_nms_opts_scenes.py shows on the CPU that every scene has the property its case is about."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nms_opts_ref as nr
from tests import post_scenes as ps
from tests.test_postprocess_gpu import DSENT, IDENT, ISENT, Chain

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


class ChainEx(Chain):
    def run_ex(self, opts, iou=0.45, max_det=300, max_nms=30000, lb=IDENT, conf=0.01, heads=None, no=15, expect=0):
        """Chain.run through y7t_det_postprocess_ex.  opts: None (a NULL pointer), or (classes, agnostic, multi_label).  expect: the return code the call must give"""
        from yolov7_tracker_amd import _lib
        B = self.B
        if max_det not in self.out:
            self.out[max_det] = (torch.empty((B, max_det, 6), device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
                                 torch.empty((B, max_det), dtype=torch.int32, device="cuda"))
        dets, nd, keep = self.out[max_det]
        dets.fill_(DSENT); nd.fill_(ISENT); keep.fill_(ISENT); self.cand.fill_(ISENT)
        lbt = torch.tensor(np.broadcast_to(np.asarray(lb, np.float32), (B, 5)).copy(), device="cuda")
        if heads is None:
            hp = ny = nx = st = an = None
            nl, na = 4, 3
        else:
            nl, na, no = heads["nl"], heads["na"], heads["no"]
            self._heads = [torch.from_numpy(h).cuda() for h in heads["heads"]]
            hp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in self._heads] + [None] * (4 - nl))
            ny = (ctypes.c_int * 4)(*[s[0] for s in heads["shapes"]] + [0] * (4 - nl))
            nx = (ctypes.c_int * 4)(*[s[1] for s in heads["shapes"]] + [0] * (4 - nl))
            st = (ctypes.c_float * 4)(*[float(v) for v in heads["strides"]] + [0.0] * (4 - nl))
            flat = [float(v) for v in heads["anchors"].ravel()]
            an = (ctypes.c_float * 24)(*(flat + [0.0] * (24 - len(flat))))
        if opts is None:
            o = None
        else:
            classes, agnostic, multi_label = opts
            o = _lib.NmsOpts(int(agnostic), int(multi_label), int(classes is not None))      # (zeroed for (None, False, False): nms_opts() would say None)
            for c in (classes or ()):
                if 0 <= c < 256:
                    o.class_mask[c >> 5] |= 1 << (c & 31)
            o = ctypes.byref(o)
        rc = self.L.y7t_det_postprocess_ex(hp, ny, nx, st, an, nl, na, no, B, float(conf), float(iou), max_det, max_nms, self.cap, _lib.ptr(lbt), _lib.ptr(dets),
                                           _lib.ptr(nd), _lib.ptr(keep), _lib.ptr(self.cand), _lib.ptr(self.ws), self.lay["total"], _lib.stream_ptr(), o)
        torch.cuda.synchronize()
        assert rc == expect, (rc, self.L.y7t_last_error())
        return dets.cpu().numpy(), nd.cpu().numpy(), keep.cpu().numpy(), self.cand.cpu().numpy()

    def untouched_behind(self):
        return bool((self.ws[self.lay["total"]:] == ps.SENTINEL).all().item())


def check_image(out, b, scene, iou=0.45, max_det=300, max_nms=30000, lb=IDENT, classes=None, agnostic=False):
    """image b of a call's outputs against nms_opts_ref.walk over `scene`: ndets, the kept slots in order, the six columns of every row exactly, nothing past ndets"""
    dets, nd, keep, _ = out
    ref = nr.walk(scene, iou, max_nms, max_det, classes, agnostic)
    n = int(nd[b])
    assert n == len(ref), "image %d: ndets %d, the reference keeps %d" % (b, n, len(ref))
    np.testing.assert_array_equal(keep[b, :n], ref, err_msg="image %d: kept slots" % b)
    np.testing.assert_array_equal(dets[b, :n], ps.expected_rows(scene, ref, lb), err_msg="image %d: rows" % b)
    assert (dets[b, n:] == np.float32(DSENT)).all() and (keep[b, n:] == ISENT).all(), "image %d: rows past ndets were written" % b
    return n


# ------------------------------------------------------------------------------------------------ the defaults
def test_null_zeroed_and_all_classes_are_the_plain_call(L):
    """opts == NULL, zeroed opts and classes = every class are bit-equal to y7t_det_postprocess on the boundary-count scenes (0 ... 1000 candidates)"""
    scenes = [ps.clustered(n, seed=n) for n in ps.BOUNDARY_COUNTS]
    ch = ChainEx(L, len(scenes), 1024)
    ch.plant(scenes)
    want = ch.run()
    assert int(want[1].sum()) > 100
    for opts in (None, (None, False, False), ([0, 1, 2], False, False), (list(range(256)), False, False)):
        got = ch.run_ex(opts)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), opts
    assert np.array_equal(ch.ws.cpu().numpy()[:len(ch.planted)], ch.planted) and ch.untouched_behind()


# ------------------------------------------------------------------------------------------------ agnostic
@pytest.mark.parametrize("iou", [0.0, 0.45, 0.5, 0.65, 1.0])
def test_agnostic(L, iou):
    """identical boxes of two classes keep one; IoU exactly 0.5 across classes is kept at 0.5 and suppressed below; equal scores go by anchor row; at 1.0 nothing is
    suppressed.  The same call with agnostic off gives the class-aware answer on the same workspace."""
    scenes = [nr.mixed_clusters(), nr.two_class_pairs(), nr.tied_pairs(), ps.class_offsets()]
    ch = ChainEx(L, 4, 1024)
    ch.plant(scenes)
    out = ch.run_ex((None, True, False), iou=iou)
    kept = [check_image(out, b, s, iou=iou, agnostic=True) for b, s in enumerate(scenes)]
    aware = ch.run_ex((None, False, False), iou=iou)
    kept_aware = [check_image(aware, b, s, iou=iou) for b, s in enumerate(scenes)]
    if iou == 0.45:
        assert kept[1:3] == [6, 40] and kept_aware[1:3] == [18, 80] and kept[0] < kept_aware[0]
    if iou == 0.5:
        assert kept[1] == 12
    if iou == 1.0:
        assert kept == kept_aware
    assert out[3].tolist() == [len(s["score"]) for s in scenes]


# ------------------------------------------------------------------------------------------------ classes
def test_classes(L):
    """one class, several, an id >= nc, the empty list, on B = 4 images of which one has no candidate of class 1: results per image.  Then other class sets and none on
    the SAME workspace: each call gives its own answer and the candidate arrays are byte-identical before and after."""
    base = ps.clustered(600, seed=600)
    scenes = [base, nr.no_class(base, 1), ps.clustered(0, seed=0), nr.mixed_clusters()]
    ch = ChainEx(L, 4, 1024)
    ch.plant(scenes)
    before = ch.ws.cpu().numpy()[:len(ch.planted)].copy()
    assert np.array_equal(before, ch.planted)
    counts = [len(s["score"]) for s in scenes]
    for classes in ([1], [0, 2], [1, 7], [2, 200, 255], [7], [], None, [1]):
        out = ch.run_ex((classes, False, False))
        kept = [check_image(out, b, s, classes=classes) for b, s in enumerate(scenes)]
        assert out[3].tolist() == counts                                   # cand_count: the candidates found, not the ones the filter let through
        if classes == [1]:
            assert kept[0] > 0 and kept[1] == kept[2] == 0 and kept[3] > 0
        if classes in ([7], []):
            assert kept == [0, 0, 0, 0] and (out[0] == np.float32(DSENT)).all()
        if classes is None:
            assert kept[0] == len(ps.reference_walk(base))
        assert np.array_equal(ch.ws.cpu().numpy()[:len(ch.planted)], before), classes
    out = ch.run_ex(([0, 2], True, False))                                 # ... and with agnostic
    for b, s in enumerate(scenes):
        check_image(out, b, s, classes=[0, 2], agnostic=True)
    assert ch.untouched_behind()


def test_classes_filter_before_the_cuts(L):
    """max_nms = 4 with the four best candidates in an excluded class: the filter comes first (general.py:662-674), the best four of the listed classes are walked.
    max_det: the excluded classes take none of the output slots."""
    s, sep = nr.filter_before_cut(4), ps.separated()
    ch = ChainEx(L, 2, 1024)
    ch.plant([s, sep])
    out = ch.run_ex(([1, 2], False, False), max_nms=4)
    assert check_image(out, 0, s, max_nms=4, classes=[1, 2]) == 4
    check_image(out, 1, sep, max_nms=4, classes=[1, 2])
    for max_det in (1, 50, 65):
        out = ch.run_ex(([3, 4], False, False), max_det=max_det)
        assert check_image(out, 1, sep, max_det=max_det, classes=[3, 4]) == max_det
        check_image(out, 0, s, max_det=max_det, classes=[3, 4])
        assert set(out[0][1, :max_det, 5].tolist()) <= {3.0, 4.0}


# ------------------------------------------------------------------------------------------------ multi_label: k_decode_filter_ml
def _check_ml_candidates(sc, conf, scenes, count, cap):
    """the candidate arrays the multi-label decode left against the restatement's candidates of the same logits: the set of (row, class) pairs and the count exactly,
    score at rtol 1e-5 / atol 1e-6 and box at rtol 1e-5 / atol 1e-4 (the decode pass's tolerances in tests/test_postprocess_gpu.py)"""
    dec = nr.decode(sc)
    for b in range(sc["B"]):
        want, got = nr.candidates(dec[b], conf, True), scenes[b]
        wmap = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(want["rows"], want["cls"]))}
        pairs = list(zip(got["rows"].tolist(), [int(c) for c in got["cls"]]))
        assert int(count[b]) == len(wmap), "image %d: cand_count %d, the reference finds %d" % (b, count[b], len(wmap))
        assert len(pairs) == min(len(wmap), cap) and len(set(pairs)) == len(pairs) and set(pairs) <= set(wmap)
        if len(wmap) <= cap:
            assert set(pairs) == set(wmap)
        idx = np.array([wmap[p] for p in pairs], np.int64)
        np.testing.assert_allclose(got["score"], want["score"][idx], rtol=1e-5, atol=1e-6, err_msg="image %d score" % b)
        np.testing.assert_allclose(got["box"], want["box"][idx], rtol=1e-5, atol=1e-4, err_msg="image %d box" % b)
        for r in set(got["rows"].tolist()):                                # a row's candidates: consecutive slots (one reservation), classes ascending
            sl = np.nonzero(got["rows"] == r)[0]
            assert (np.diff(sl) == 1).all() and (np.diff(got["cls"][sl]) > 0).all()


@pytest.mark.parametrize("conf", [0.01, 0.25])
@pytest.mark.parametrize("gi", range(len(ps.GRIDS)))
def test_multi_label_decode(L, gi, conf):
    """head != NULL with multi_label on the tiny grids: nc == 1 runs the best-class path (bit-equal to the plain call); nc > 1: the (row, class) candidates against the
    restatement, then the NMS outputs exactly against the walk over the DEVICE's own candidates -- class-aware, agnostic, and with a class filter on top"""
    sc = nr.ml_scene(gi, conf)
    nc = sc["no"] - 5
    ch = ChainEx(L, sc["B"], 1024)
    out = ch.run_ex((None, False, True), conf=conf, heads=sc)
    scenes, count = ch.candidates()
    assert np.array_equal(out[3], count)
    if nc == 1:
        for b, s in enumerate(scenes):
            check_image(out, b, s)
        rows = [s["rows"][out[2][b, :out[1][b]]] for b, s in enumerate(scenes)]
        plain = ch.run(conf=conf, heads=sc)                                # (the decode hands its slots out anew: the rows, not the slots, repeat from call to call)
        scenes, _ = ch.candidates()
        assert all(np.array_equal(out[k], plain[k]) for k in (0, 1, 3)) and int(plain[1].sum()) > 0
        assert all(np.array_equal(r, s["rows"][plain[2][b, :plain[1][b]]]) for b, (r, s) in enumerate(zip(rows, scenes)))
        return
    _check_ml_candidates(sc, conf, scenes, count, 1024)
    for b, s in enumerate(scenes):
        assert check_image(out, b, s) > 0
    for classes, agnostic in ((None, True), ([0, nc - 1], False), ([1], True)):
        out = ch.run_ex((classes, agnostic, True), conf=conf, heads=sc)
        scenes, _ = ch.candidates()
        for b, s in enumerate(scenes):
            check_image(out, b, s, classes=classes, agnostic=agnostic)
    assert ch.untouched_behind()


def test_multi_label_at_the_cap(L):
    """every objectness logit at +6, ~60 classes of 80 passing per row, cap inside one row's reservation: cand_count is the true number of (row, class) pairs, image 0's
    slots are the first cap pairs in reservation order (its level-0 rows are one wave's), every image's slots below cap are valid distinct candidates, the walk runs
    over them, and nothing past cap or behind the workspace is touched"""
    conf = 0.25
    sc = nr.ml_scene(3, conf, obj_logit=6.0)
    cap, first = nr.straddle_cap(sc, conf)
    ch = ChainEx(L, sc["B"], cap)
    out = ch.run_ex((None, False, True), conf=conf, heads=sc)
    scenes, count = ch.candidates()
    assert np.array_equal(out[3], count) and all(len(s["rows"]) == cap for s in scenes)
    _check_ml_candidates(sc, conf, scenes, count, cap)
    assert list(zip(scenes[0]["rows"].tolist(), [int(c) for c in scenes[0]["cls"]])) == first
    for b, s in enumerate(scenes):
        check_image(out, b, s)
    ws = ch.ws.cpu().numpy()
    names = [k for k in ch.lay if k != "total"]
    ends = [ch.lay[k][0] for k in names[1:]] + [ch.lay["total"]]
    for k, end in zip(names, ends):                                        # cap is no multiple of 64: the padding behind every array stays as it was
        o, nbytes = ch.lay[k]
        assert (ws[o + nbytes:end] == ps.SENTINEL).all(), "bytes behind %s were written" % k
    assert ch.untouched_behind()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(L):
    """multi_label with head == NULL: Y7T_E_STATE, the message says why; a class filter with nc above the mask's 256 classes: Y7T_E_ARG; outputs and workspace untouched"""
    scenes = [ps.clustered(100, seed=100)]
    ch = ChainEx(L, 1, 1024)
    ch.plant(scenes)
    before = ch.ws.cpu().numpy().copy()
    for opts, no, rc in (((None, False, True), 15, E_STATE), (([1], False, False), 5 + 257, E_ARG)):
        out = ch.run_ex(opts, no=no, expect=rc)
        assert (out[0] == np.float32(DSENT)).all() and (out[1] == ISENT).all() and (out[2] == ISENT).all() and (out[3] == ISENT).all()
        assert np.array_equal(ch.ws.cpu().numpy(), before)
        if rc == E_STATE:
            assert b"fused" in L.y7t_last_error() and b"multi_label" in L.y7t_last_error()
    check_image(ch.run_ex((None, False, True), no=6), 0, scenes[0])        # nc == 1: multi_label is ignored, head == NULL is fine
    check_image(ch.run_ex(([1], False, False), no=5 + 256), 0, scenes[0], classes=[1])


# ------------------------------------------------------------------------------------------------ product level
@pytest.fixture(scope="module")
def tiny3():
    from yolov7_tracker_amd.detector import arch, model
    return model.Detector(arch.ARCHS["yolov7-tiny"](3), None, img_size=(128, 192), max_batch=2, seed=0)


def _kept(det, out, nd, **kw):
    """per image the (anchor row, class) of the kept detections, in output order -- after checking the kept slots against the walk over the candidates the call saw"""
    torch.cuda.synchronize()
    ps_ = det.plan.post[out.pset]
    cbox, cscore, ccls, cidx, count = (t.cpu().numpy() for t in det.candidate_arrays(out.pset))
    res = []
    for b in range(out.B):
        n = int(count[b])
        assert 0 < n <= det.max_cand
        scene = {"box": cbox[b, :n], "score": cscore[b, :n], "cls": ccls[b, :n], "rows": cidx[b, :n]}
        k = ps_.keep[b, :int(nd[b])].cpu().numpy()
        np.testing.assert_array_equal(k, nr.walk(scene, 0.45, **kw))
        res.append(list(zip(cidx[b][k].tolist(), ccls[b][k].tolist())))
    return res


def test_detector_classes_and_agnostic_fused_and_unfused(tiny3):
    """Detector.postprocess with classes / agnostic after a fused forward (candidates from the Detect epilogues, head == NULL) and after a plain one (decode pass) keeps
    the same anchor rows with the same classes; the options change the answer; multi_label on the fused output is a ValueError that names fuse_decode"""
    det = tiny3
    img = torch.rand((2, 3, 128, 192), generator=torch.Generator().manual_seed(12))
    res = {}
    for fused in (False, True):
        for key, kw in (("plain", {}), ("classes", {"classes": [0, 2]}), ("agnostic", {"agnostic": True}), ("both", {"classes": [1, 2], "agnostic": True})):
            out = det.forward(img, fuse_decode=0.01) if fused else det.forward(img)
            _, nd = det.postprocess(out, 0.01, 0.45, None, **kw)
            res[(fused, key)] = _kept(det, out, nd.cpu().numpy(), **kw)
    for key in ("plain", "classes", "agnostic", "both"):
        assert res[(True, key)] == res[(False, key)], key
    plain = res[(False, "plain")]
    assert all(len(p) > 0 for p in plain) and {c for p in plain for _, c in p} == {0.0, 1.0, 2.0}
    assert all(len(p) > 0 and {c for _, c in p} <= {0.0, 2.0} for p in res[(False, "classes")])
    assert all(len(p) > 0 and {c for _, c in p} <= {1.0, 2.0} for p in res[(False, "both")])
    assert res[(False, "agnostic")] != plain
    out = det.forward(img, fuse_decode=0.01)
    with pytest.raises(ValueError, match="fuse_decode"):
        det.postprocess(out, 0.01, 0.45, None, multi_label=True)


def test_non_max_suppression_honours_the_three_options(tiny3):
    """detector.non_max_suppression on planted head tensors returns the restatement's rows for every combination (multi_label unfused); labels stay NotImplementedError"""
    from oracle import detector_torch as dt
    from yolov7_tracker_amd.detector import model
    det = tiny3
    g = torch.Generator().manual_seed(11)
    out = det(torch.rand((2, 3, 128, 192), generator=g))[0]
    for l in range(len(det.plan.heads)):
        t = det.head_tensor(l, 2)
        t.copy_((torch.randn(t.shape, generator=g) * 1.5).cuda())
        # objectness logits 2 lower: about a quarter of the rows pass 0.25, so that the (row, class) candidates of multi_label stay below the detector's candidate
        # capacity -- one slot per anchor row, which the best-class path can never overflow
        t.view(2, t.shape[1], t.shape[2], 3, det.plan.det["no"])[..., 4] -= 2.0
    dec = dt.decode_heads([r.cpu() for r in out.raw()], det.spec["anchors"], 128).numpy()
    n_ml = 0
    for kw in ({}, {"classes": [1]}, {"agnostic": True}, {"multi_label": True}, {"classes": [0, 2], "agnostic": True, "multi_label": True}):
        got = model.non_max_suppression(out, 0.25, 0.45, **kw)
        want = nr.nms(dec, 0.25, 0.45, **kw)
        for b in range(2):
            g_, w_ = got[b].cpu().numpy(), want[b]
            assert len(g_) == len(w_) > 0, (kw, b, len(g_), len(w_))
            assert np.array_equal(g_[:, 5], w_[:, 5])
            np.testing.assert_allclose(g_[:, 4], w_[:, 4], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(g_[:, :4], w_[:, :4], rtol=1e-5, atol=1e-4)
        if kw == {"multi_label": True}:
            n_ml = sum(len(w) for w in want)
    assert n_ml > sum(len(w) for w in nr.nms(dec, 0.25, 0.45))
    with pytest.raises(NotImplementedError):
        model.non_max_suppression(out, 0.25, 0.45, labels=[torch.zeros((1, 5))])
    with pytest.raises(ValueError, match="fuse_decode"):
        model.non_max_suppression(det.forward(torch.rand((2, 3, 128, 192), generator=g), fuse_decode=0.25), 0.25, 0.45, multi_label=True)
