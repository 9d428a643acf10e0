"""CPU: the mAP evaluation's portable bodies (csrc/y7t_map.h, host build tests/_hostsim/map.py) against the goldens recorded from the reference's functions
(tests/golden/map_*.npz) and against the restatement tests/map_np.py.  Integers and the float32 matching are array-equal; the float64 curves are held to 1e-12
absolute, the bar of the TrackEval port, on quantities in [0, 1]."""
import os

import numpy as np
import pytest
import torch

from tests import map_np, map_scenes as sc
from tests._hostsim import map as hs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-12


@pytest.fixture(scope="module")
def gold_match():
    return np.load(os.path.join(GOLD, "map_match.npz"))


@pytest.fixture(scope="module")
def gold_compute():
    return np.load(os.path.join(GOLD, "map_compute.npz"))


def run_case(hm, case, **kw):
    hm.update_raw(**sc.raw_args(case, **kw))


def inject(hm, case):
    """stored rows straight into the state: conf, cls, the correct masks, nt and the row count"""
    n = len(case["conf"])
    assert n <= hm.cap
    hm.reset()
    for k, a in (("conf", case["conf"].astype(np.float32)), ("cls", case["cls"].astype(np.int32)), ("correct", sc.masks(case["tp"]))):
        hm.state[hm._off[k]:hm._off[k] + 4 * n] = a.view(np.uint8)
    hm.state[hm._off["nt"]:hm._off["nt"] + 8 * hm.nc] = case["nt"].astype(np.int64).view(np.uint8)
    hm.header()[0] = n


def test_the_parallel_rule_is_the_literal_loop():
    """the restatement the kernels implement against the reference's loop, on random images with many same-class collisions"""
    rng = np.random.default_rng(5)
    diff = 0
    for i in range(60):
        P, T = int(rng.integers(0, 40)), int(rng.integers(0, 12))
        pred, tg = sc._image(rng, P, T, 640, int(rng.integers(1, 4)), 0)
        pred[:, 4] = np.sort(rng.random(P).astype(np.float32))[::-1]
        pred, lab = torch.from_numpy(pred), torch.from_numpy(tg[:, 1:])
        lb = sc._lb_square(1, 640)[0]
        diff += int((map_np.image_stats(pred, lab, (640, 640), lb) != map_np.image_stats_rule(pred, lab, (640, 640), lb)).any())
    assert diff == 0


def test_grids_are_numpys_linspace():
    assert np.array_equal(hs.linspace01(101), np.linspace(0, 1, 101))
    assert np.array_equal(hs.linspace01(1000), np.linspace(0, 1, 1000))


def test_box_arithmetic_is_torchs_bit_for_bit():
    rng = np.random.default_rng(11)
    lb = np.array([0.64, 3.5, 32.0, 500.0, 1000.0], np.float32)
    for _ in range(200):
        row = np.concatenate([[0, 1], rng.uniform(0, 1, 2), rng.uniform(0.01, 0.6, 2)]).astype(np.float32)
        box = (rng.uniform(-30, 600, 4)).astype(np.float32)
        box[2:] = box[:2] + rng.uniform(1, 200, 2).astype(np.float32)
        predn, tbox = map_np.native_boxes(torch.from_numpy(np.concatenate([box, [0.5, 1]]).astype(np.float32))[None], torch.from_numpy(row[1:])[None], (384, 640), lb)
        got_t, got_p = hs.target_box(row, 640, 384, lb), hs.scale_coords(box, lb)
        assert np.array_equal(got_t, tbox[0].numpy()) and np.array_equal(got_p, predn[0].numpy())
        assert hs.iou(got_p, got_t) == np.float32(map_np.box_iou(predn, tbox)[0, 0].item())


@pytest.mark.parametrize("name", list(sc.MATCH_CASES))
def test_matching_equals_the_golden(name, gold_match):
    case = sc.MATCH_CASES[name]()
    hm = hs.HostMAP(case["nc"], 1024)
    run_case(hm, case)
    conf, cls, cor, nt = hm.rows()
    for k, a in (("correct", cor), ("conf", conf), ("cls", cls), ("nt", nt)):
        assert np.array_equal(a, gold_match[name + "." + k]), k
    assert int(hm.header()[1]) == len(case["preds"]) and int(hm.header()[2]) == 0


def test_ulp_case_sits_on_the_thresholds(gold_match):
    """the fixture is what it says: pair 3k + 1 has exactly IoU iouv[k] (false at k: the comparison is strict), 3k below (false), 3k + 2 above (true)"""
    cor = gold_match["ulp.correct"]
    for k in range(10):
        assert not cor[3 * k, k] and not cor[3 * k + 1, k] and cor[3 * k + 2, k]
        assert cor[3 * k:3 * k + 3, :k].all() and not cor[3 * k:3 * k + 3, k + 1:].any()


def test_two_claimants_the_loser_stays_false(gold_match):
    assert gold_match["two_claim.correct"][:, 0].tolist() == [True, False, True]


@pytest.mark.parametrize("cuts", [(1,), (3,), (1, 2, 4)])
def test_the_batch_split_does_not_change_the_rows(cuts, gold_match):
    case = sc.MATCH_CASES["batch5"]()
    hm = hs.HostMAP(case["nc"], 1024)
    edges = (0,) + tuple(cuts) + (5,)
    for lo, hi in zip(edges[:-1], edges[1:]):
        run_case(hm, sc.split(case, lo, hi), seed=lo)
    conf, cls, cor, nt = hm.rows()
    for k, a in (("correct", cor), ("conf", conf), ("cls", cls), ("nt", nt)):
        assert np.array_equal(a, gold_match["batch5." + k]), k
    assert int(hm.header()[1]) == 5


def test_overflow_sets_the_status_bit_and_stores_nothing():
    case = sc.MATCH_CASES["batch5"]()
    hm = hs.HostMAP(case["nc"], 350)
    run_case(hm, sc.split(case, 0, 3))
    before = [a.copy() for a in hm.rows()] + [hm.header()[:2].copy()]
    run_case(hm, sc.split(case, 3, 5))      # 57 + 303 > 350
    after = [a.copy() for a in hm.rows()] + [hm.header()[:2].copy()]
    assert int(hm.header()[2]) & 1 and all(np.array_equal(a, b) for a, b in zip(before, after)) and int(hm.header()[0]) == 57


def check_compute(raw, case, want, tol=TOL):
    """raw device / host outputs against ap_per_class's tuple -> the largest absolute differences (ap, p, r, f1)"""
    from yolov7_tracker_amd.detector.evaluate import finish
    assert raw["rows"] == len(case["conf"]) and np.array_equal(raw["nt"], case["nt"])
    assert np.array_equal(raw["classes"], want["classes"])
    p, r, ap, f1, classes = finish(raw["ap"], raw["p"], raw["r"], raw["classes"])
    errs = [float(np.abs(a - want[k]).max()) if a.size else 0.0 for k, a in (("ap", ap), ("p", p), ("r", r), ("f1", f1))]
    assert max(errs) <= tol, errs
    return errs


@pytest.mark.parametrize("name", list(sc.COMPUTE_CASES))
def test_compute_equals_the_golden(name, gold_compute):
    case = sc.COMPUTE_CASES[name]()
    hm = hs.HostMAP(case["nc"], len(case["conf"]) + 3)
    inject(hm, case)
    raw = hm.compute_raw()
    check_compute(raw, case, {k: gold_compute[name + "." + k] for k in ("p", "r", "ap", "f1", "classes")})
    # the integers: the sorted order is the stable (class, -conf, arrival) order, the counts are its per-class cumulative sums
    order = np.lexsort((np.arange(len(case["conf"])), -case["conf"].astype(np.float64), case["cls"]))
    assert np.array_equal(raw["order"], order)
    tp, cls = case["tp"][order], case["cls"][order]
    for c in np.unique(cls):
        assert np.array_equal(raw["tpc"][cls == c], tp[cls == c].cumsum(0))
    # ... and the whole curves, not only the column ap_per_class returns
    ap, p, r, classes = map_np.ap_curves(case["tp"], case["conf"], case["cls"].astype(np.float32), sc.target_cls_of(case["nt"]))
    assert np.abs(raw["p"][classes] - p).max() <= TOL and np.abs(raw["r"][classes] - r).max() <= TOL and np.abs(raw["ap"][classes] - ap).max() <= TOL
    rest = np.setdiff1d(np.arange(case["nc"]), classes)
    assert not raw["p"][rest].any() and not raw["r"][rest].any() and not raw["ap"][rest].any()


def test_equal_confidences_keep_their_arrival_order():
    case = sc.EQUAL_CONF_CASE()
    assert len(np.unique(case["conf"])) < 20
    hm = hs.HostMAP(case["nc"], 1000)
    inject(hm, case)
    raw = hm.compute_raw()
    check_compute(raw, case, sc.expected_compute(case))
    assert np.array_equal(raw["order"], np.lexsort((np.arange(900), -case["conf"].astype(np.float64), case["cls"])))


def test_two_computes_give_the_same_bits():
    case = sc.COMPUTE_CASES["nc80"]()
    hm = hs.HostMAP(case["nc"], 3000)
    inject(hm, case)
    a, b = hm.compute_raw(), hm.compute_raw()
    assert all(np.array_equal(a[k], b[k]) for k in ("ap", "p", "r", "nt", "classes", "order"))


def test_wrong_interp_index_would_show():
    """the n_l cases are sharp: taking the FIRST j with mrec[j] <= x on repeated recalls moves an AP by far more than the tolerance"""
    case = sc.COMPUTE_CASES["nl_10"]()
    tp, conf = case["tp"][np.argsort(-case["conf"], kind="stable")], None
    tpc = tp[:, 0].cumsum()
    rec, prec = tpc / (10 + 1e-16), tpc / np.arange(1, len(tpc) + 1)
    mrec = np.concatenate(([0.], rec, [rec[-1] + 0.01]))
    mpre = np.flip(np.maximum.accumulate(np.flip(np.concatenate(([1.], prec, [0.])))))
    x = np.linspace(0, 1, 101)
    first = np.array([mpre[np.searchsorted(mrec, v, side="left")] if v in mrec else np.interp(v, mrec, mpre) for v in x])
    assert np.abs(first - np.interp(x, mrec, mpre)).max() > 1e-3


def test_host_arithmetic_and_group_targets():
    from yolov7_tracker_amd.detector import evaluate as ev
    t = torch.tensor([[1, 0, .5, .5, .1, .1], [0, 2, .5, .5, .1, .1], [1, 1, .2, .2, .1, .1], [3, 0, .2, .2, .1, .1]])
    rows, off = ev.group_targets(t, 4)
    assert off.tolist() == [0, 1, 3, 3, 4] and rows[:, 0].tolist() == [0, 1, 1, 3] and rows[1:3, 1].tolist() == [0, 1]
    with pytest.raises(ValueError):
        ev.group_targets(t, 3)
    lb = ev.letterbox_rows([((500, 1000), ((0.64, 0.64), (0.0, 32.0))), (384, 640)], 2, (384, 640))
    assert np.allclose(lb, [[0.64, 0, 32, 500, 1000], [1, 0, 0, 384, 640]])
    order, bi, shapes = ev.rect_batch_shapes([(480, 640), (640, 480), (500, 500), (300, 600)], 640, 2, 32)
    assert order.tolist() == [3, 0, 2, 1] and bi.tolist() == [0, 0, 1, 1] and shapes.tolist() == [[512, 672], [672, 672]]
    labels = __import__("yolov7_tracker_amd.synth", fromlist=["x"]).make_frame_labels(2, 10, 320, 0)
    assert len(labels) == 2 and labels[0].shape[1] == 5 and (labels[0][:, 1:] >= 0).all() and (labels[0][:, 1:] <= 1).all()


def test_yaml_loader_batches_images_and_moves_the_labels(tmp_path):
    """the data-yaml loader on three small image files: rect batch shapes, the /images/ -> /labels/ rule, labels carried into the letterboxed image, shapes[si]"""
    from PIL import Image
    from yolov7_tracker_amd.detector import evaluate as ev
    img_dir, lab_dir = tmp_path / "set" / "images" / "val", tmp_path / "set" / "labels" / "val"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir(parents=True)
    for name, (h, w) in (("a", (48, 96)), ("b", (96, 96)), ("c", (40, 80))):
        Image.fromarray(np.full((h, w, 3), 90, np.uint8)).save(str(img_dir / (name + ".png")))
    (lab_dir / "a.txt").write_text("3 0.5 0.5 0.5 0.5\n1 0.25 0.25 0.1 0.2\n")
    (lab_dir / "b.txt").write_text("0 0.5 0.5 1.0 1.0\n")
    batches = list(ev.yaml_batches({"val": str(tmp_path / "set" / "images" / "val")}, "val", img_size=96, batch_size=2, stride=32))
    assert [tuple(b[0].shape) for b in batches] == [(2, 3, 64, 128), (1, 3, 128, 128)]      # ceil([0.5, 1] * 96 / 32 + 0.5) * 32 and ceil(3.5) * 32
    img, targets, paths, shapes = batches[0]
    assert [os.path.basename(p) for p in paths] == ["a.png", "c.png"] and img.dtype == torch.uint8
    (h0, w0), (ratio, pad) = shapes[0]
    assert (h0, w0) == (48, 96) and ratio == (1.0, 1.0) and pad == (16.0, 8.0)
    t = targets[targets[:, 0] == 0].numpy()
    assert t[:, 1].tolist() == [1.0, 3.0]
    # class 3: centre (48, 24) + pad (16, 8) = (64, 32) of 128 x 64, size 48 x 24
    assert np.allclose(t[1, 2:], [64 / 128, 32 / 64, 48 / 128, 24 / 64], atol=1e-6)
    assert len(targets[targets[:, 0] == 1]) == 0 and (img[0, :, 0, 0] == 114).all() and (img[0, :, 32, 64] == 90).all()
    lb = ev.letterbox_rows(shapes, 2, (64, 128))
    assert np.allclose(lb[0], [1.0, 16.0, 8.0, 48, 96]) and np.allclose(lb[1], [1.2, 16.0, 8.0, 40, 80])
    (h0, w0), (ratio, pad) = batches[1][3][0]
    assert (h0, w0) == (96, 96) and pad == (16.0, 16.0) and np.allclose(batches[1][1][0, 2:].numpy(), [0.5, 0.5, 0.75, 0.75])
