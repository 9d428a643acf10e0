"""GPU: the mAP evaluation through the C ABI (y7t_map_*) and the Python surface (detector/evaluate.py) against the goldens recorded from the reference's functions
and the restatement tests/map_np.py.  The matching is array-equal; the float64 curves are held to 1e-12 absolute (quantities in [0, 1])."""
import os

import numpy as np
import pytest
import torch

from tests import map_np, map_scenes as sc
from tests.test_map_cpu import check_compute

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold_match():
    return np.load(os.path.join(GOLD, "map_match.npz"))


@pytest.fixture(scope="module")
def gold_compute():
    return np.load(os.path.join(GOLD, "map_compute.npz"))


def device_map(nc, cap):
    from yolov7_tracker_amd.detector.evaluate import DeviceMAP
    return DeviceMAP(nc, cap)


def run_case(dm, case, **kw):
    a = sc.raw_args(case, **kw)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in a.items() if k not in ("hw", "targets")}
    tg = a["targets"] if len(a["targets"]) else np.zeros((1, 6), np.float32)
    d["targets"] = torch.from_numpy(np.ascontiguousarray(tg)).cuda()
    cap = a["cbox"].shape[1]
    dm.update_arrays(d["dets"], d["ndets"], d["keep"], d["cbox"], cap, cap, len(a["ndets"]), d["targets"], d["toff"], a["hw"], d["lb"])
    torch.cuda.synchronize()


def inject(dm, case):
    n = len(case["conf"])
    assert n <= dm.cap_rows
    dm.reset()
    for k, a in (("conf", case["conf"].astype(np.float32)), ("cls", case["cls"].astype(np.int32)), ("correct", sc.masks(case["tp"]))):
        dm.state[dm._off[k]:dm._off[k] + 4 * n].copy_(torch.from_numpy(a.view(np.uint8).copy()))
    dm.state[dm._off["nt"]:dm._off["nt"] + 8 * dm.nc].copy_(torch.from_numpy(case["nt"].astype(np.int64).view(np.uint8).copy()))
    dm.header()[0] = n


@pytest.mark.parametrize("name", list(sc.MATCH_CASES))
def test_matching_equals_the_golden(name, gold_match):
    case = sc.MATCH_CASES[name]()
    dm = device_map(case["nc"], 1024)
    run_case(dm, case)
    conf, cls, cor, nt = dm.rows()
    for k, a in (("correct", cor), ("conf", conf), ("cls", cls), ("nt", nt)):
        assert np.array_equal(a, gold_match[name + "." + k]), k
    h = dm.header().cpu().numpy()
    assert h[1] == len(case["preds"]) and h[2] == 0


@pytest.mark.parametrize("cuts", [(1,), (3,)])
def test_the_batch_split_does_not_change_the_rows(cuts, gold_match):
    case = sc.MATCH_CASES["batch5"]()
    dm = device_map(case["nc"], 1024)
    edges = (0,) + tuple(cuts) + (5,)
    for lo, hi in zip(edges[:-1], edges[1:]):
        run_case(dm, sc.split(case, lo, hi), seed=lo)
    conf, cls, cor, nt = dm.rows()
    for k, a in (("correct", cor), ("conf", conf), ("cls", cls), ("nt", nt)):
        assert np.array_equal(a, gold_match["batch5." + k]), k
    assert int(dm.header()[1].item()) == 5


def test_overflow_sets_the_status_bit_and_stores_nothing():
    case = sc.MATCH_CASES["batch5"]()
    dm = device_map(case["nc"], 350)
    run_case(dm, sc.split(case, 0, 3))
    before = list(dm.rows()) + [dm.header()[:2].cpu().numpy()]
    run_case(dm, sc.split(case, 3, 5))      # 57 + 303 > 350
    after = list(dm.rows()) + [dm.header()[:2].cpu().numpy()]
    assert int(dm.header()[2].item()) & 1 and all(np.array_equal(a, b) for a, b in zip(before, after)) and int(dm.header()[0].item()) == 57
    from yolov7_tracker_amd import _lib
    with pytest.raises(_lib.Y7TError):
        dm.compute()


@pytest.mark.parametrize("name", list(sc.COMPUTE_CASES))
def test_compute_equals_the_golden(name, gold_compute):
    case = sc.COMPUTE_CASES[name]()
    dm = device_map(case["nc"], len(case["conf"]) + 3)
    inject(dm, case)
    raw = dm.compute_raw()
    errs = check_compute(raw, case, {k: gold_compute[name + "." + k] for k in ("p", "r", "ap", "f1", "classes")})
    print("%s: max |ap|, |p|, |r|, |f1| error %s" % (name, " ".join("%.3g" % e for e in errs)))
    # the device against the host build of the same bodies: the same bits, whole curves included
    from tests._hostsim import map as hs
    from tests.test_map_cpu import inject as inject_host
    hm = hs.HostMAP(case["nc"], len(case["conf"]) + 3)
    inject_host(hm, case)
    host = hm.compute_raw()
    for k in ("ap", "p", "r", "nt", "classes"):
        assert np.array_equal(raw[k], host[k]), k


def test_equal_confidences_keep_their_arrival_order():
    case = sc.EQUAL_CONF_CASE()
    dm = device_map(case["nc"], 1000)
    inject(dm, case)
    check_compute(dm.compute_raw(), case, sc.expected_compute(case))


def test_two_computes_give_the_same_bits():
    case = sc.COMPUTE_CASES["nc80"]()
    dm = device_map(case["nc"], 3000)
    inject(dm, case)
    a, b = dm.compute_raw(), dm.compute_raw()
    assert all(np.array_equal(a[k], b[k]) for k in ("ap", "p", "r", "nt", "classes"))


# ---- end to end: yolov7-tiny with seeded weights on the synthetic frames ----
@pytest.fixture(scope="module")
def tiny():
    from yolov7_tracker_amd.detector import evaluate as ev, model
    spec, sd, seed = model.load_checkpoint("random:yolov7-tiny", None, 80)
    det = model.Detector(spec, sd, img_size=(320, 320), max_batch=4, seed=seed)
    first = next(iter(ev.synthetic_batches(4, 40, 320, 4)))
    det.plant_objectness_bias(first[0][:1].float() / 255.0, target=400)
    return det


def test_device_map_equals_the_restatement_on_the_detectors_own_rows(tiny):
    from yolov7_tracker_amd.detector import evaluate as ev
    det = tiny
    dm = ev.DeviceMAP(80, 1200)
    preds, tgs = [], []
    for img, targets, paths, shapes in ev.synthetic_batches(4, 40, 320, 2):
        out = det.forward(img.cuda().float() / 255.0)
        dets, nd = dm.update(det, out, targets, shapes)
        torch.cuda.synchronize()
        nd = nd.cpu().numpy()
        for b in range(out.B):
            d = dets[b, :nd[b]].clone()
            d[:, :4] = det.plan_raw_boxes(b, int(nd[b]), out.pset)      # the un-rounded candidate boxes
            preds.append(d.cpu())
        t = targets.clone()
        t[:, 0] += len(preds) - out.B
        tgs.append(t)
    assert sum(len(p) for p in preds) > 50      # (multi-label rows at conf 0.001: the planted head fires)
    case = dict(hw=(320, 320), lb=sc._lb_square(4, 320), preds=preds, targets=torch.cat(tgs), nc=80)
    cor, conf, cls, nt = sc.expected_stats(case)
    gconf, gcls, gcor, gnt = dm.rows()
    assert np.array_equal(gconf, conf) and np.array_equal(gcls, cls) and np.array_equal(gcor, cor) and np.array_equal(gnt, nt)
    p, r, ap, f1, classes, nt2 = dm.compute()
    wp, wr, wap, wf1, wcl = map_np.ap_per_class(cor, conf, cls.astype(np.float32), sc.target_cls_of(nt))
    assert np.array_equal(classes, wcl) and np.array_equal(nt2, nt) and dm.seen == 4
    for a, b in ((p, wp), (r, wr), (ap, wap), (f1, wf1)):
        assert np.abs(a - b).max() <= 1e-12


def test_cli_prints_the_table_and_returns_the_tuple_of_its_own_rows(capsys):
    """the command line prints test.py's table and returns test()'s tuple; the tuple is what the restatement computes from the rows that run stored"""
    from yolov7_tracker_amd.detector import evaluate as ev
    got, gmaps, gt = ev.main(["--weights", "random:yolov7-tiny", "--data", "synthetic:4:40", "--img-size", "320", "--batch-size", "4", "--plant-objectness", "400",
                              "--verbose"])
    text = capsys.readouterr().out
    assert "mAP@.5:.95" in text and "all" in text and "Speed:" in text and len(text.splitlines()) >= 4
    assert len(got) == 7 and got[4:] == (0.0, 0.0, 0.0) and gt[3:] == (320, 320, 4) and gmaps.shape == (80,)
    last = ev.evaluate.last
    conf, cls, cor, nt = last["dmap"].rows()
    assert last["seen"] == 4 and len(conf) > 50 and nt.sum() == sum(len(b[1]) for b in ev.synthetic_batches(4, 40, 320, 4))
    wp, wr, wap, wf1, wcl = map_np.ap_per_class(cor, conf, cls.astype(np.float32), sc.target_cls_of(nt))
    want, wmaps = map_np.metrics(wp, wr, wap, wcl, 80)
    assert np.abs(np.array(got[:4]) - np.array(want)).max() <= 1e-12 and np.abs(gmaps - wmaps).max() <= 1e-12
    assert ("%12.3g" % got[2]).strip() in text.splitlines()[1]


def test_augmented_evaluation_runs_the_best_class_form(tiny):
    from yolov7_tracker_amd.detector import evaluate as ev
    res, maps, t = ev.evaluate(tiny, ev.synthetic_batches(4, 40, 320, 4), 80, conf_thres=0.01, augment=True, cap_rows=1200, print_fn=lambda *a: None)
    assert len(res) == 7 and maps.shape == (80,) and ev.evaluate.last["seen"] == 4 and all(0.0 <= v <= 1.0 for v in res[:4])


def test_a_run_over_many_shapes_keeps_a_bounded_number_of_plans():
    """rect batches of several shapes: with one plan kept alive (the others destroyed and re-lowered when their shape returns) the result is that of keeping all"""
    from yolov7_tracker_amd.detector import evaluate as ev, model
    rng = np.random.default_rng(3)
    batches = []
    for H, W in ((64, 64), (64, 96), (96, 64), (64, 64)):
        img = torch.from_numpy(rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8))
        t = np.concatenate([np.repeat([0.0, 1.0], 3)[:, None], rng.integers(0, 80, (6, 1)), rng.uniform(0.3, 0.7, (6, 2)), rng.uniform(0.2, 0.5, (6, 2))], 1)
        batches.append((img, torch.from_numpy(t.astype(np.float32)), ["x"] * 2, [((H, W), ((1.0, 1.0), (0.0, 0.0)))] * 2))
    res = []
    for keep in (4, 1):
        spec, sd, seed = model.load_checkpoint("random:yolov7-tiny", None, 80)
        det = model.Detector(spec, sd, img_size=(64, 64), max_batch=2, seed=seed)
        res.append(ev.evaluate(det, batches, 80, cap_rows=2400, print_fn=lambda *a: None, max_plans=keep))
        assert len(det._plans) == (3 if keep == 4 else 1) and ev.evaluate.last["seen"] == 8
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])
