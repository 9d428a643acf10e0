"""CPU: the scenes of tests/nms_opts_ref.py have the properties the cases of tests/test_nms_opts_gpu.py are about, under the reference restatement alone -- so no GPU
test passes vacuously -- and the restatement with its three options off is the oracle the project already has (oracle.detector_torch)."""
import numpy as np
import pytest
import torch

from tests import nms_opts_ref as nr
from tests import post_scenes as ps


def _as_cands(scene):
    """a candidate scene as the dict oracle.detector_torch.nms_rows takes (unique rows)"""
    return {int(r): (scene["box"][i], float(scene["score"][i]), int(scene["cls"][i])) for i, r in enumerate(scene["rows"])}


def test_defaults_equal_the_projects_oracle():
    """classes=None, agnostic=False, multi_label=False: walk == oracle.detector_torch.nms_rows / post_scenes.reference_walk on candidate scenes, nms ==
    oracle.detector_torch.non_max_suppression on decoded tensors"""
    from oracle import detector_torch as dt
    for s in (ps.clustered(600, seed=600), ps.ties(), ps.class_offsets(), nr.mixed_clusters(), nr.tied_pairs()):
        k = nr.walk(s)
        assert np.array_equal(k, ps.reference_walk(s)) and np.array_equal(s["rows"][k], dt.nms_rows(_as_cands(s)))
    for gi in range(len(ps.GRIDS)):
        for conf in (0.01, 0.25):
            dec = nr.decode(nr.ml_scene(gi, conf))
            want = dt.non_max_suppression(torch.from_numpy(dec.copy()), conf, 0.45)
            got = nr.nms(dec, conf, 0.45)
            assert len(got) == len(want) and sum(len(g) for g in got) > 0
            for g, w in zip(got, want):
                assert np.array_equal(g, w.numpy().reshape(-1, 6))


def test_agnostic_scenes():
    s = nr.mixed_clusters()
    aware, agn = nr.walk(s), nr.walk(s, agnostic=True)
    assert set(agn.tolist()) != set(aware.tolist()) and 20 < len(agn) < len(aware)
    p = nr.two_class_pairs()
    assert [len(nr.walk(p, iou_thres=t, agnostic=True)) for t in (0.45, 0.5, 1.0)] == [6, 12, 18] and len(nr.walk(p)) == 18
    t = nr.tied_pairs()
    k = nr.walk(t, agnostic=True)
    assert len(k) == 40 and len(nr.walk(t)) == 80
    # in every pair the smaller anchor row survives, whatever its class and slot; both classes and both slot orders occur among the survivors
    for i in k:
        twin = [j for j in range(80) if j != i and np.array_equal(t["box"][j], t["box"][i])]
        assert len(twin) == 1 and t["score"][twin[0]] == t["score"][i] and t["rows"][i] < t["rows"][twin[0]] and t["cls"][i] != t["cls"][twin[0]]
    assert set(t["cls"][k].tolist()) == {0.0, 1.0}
    twins = [[j for j in range(80) if j != i and np.array_equal(t["box"][j], t["box"][i])][0] for i in k]
    assert any(i < j for i, j in zip(k, twins)) and any(i > j for i, j in zip(k, twins))
    assert len(np.unique(t["score"])) == 10                                # ... and ties across pairs: output order by anchor row inside a score
    for a, b in zip(k[:-1], k[1:]):
        assert t["score"][a] > t["score"][b] or (t["score"][a] == t["score"][b] and t["rows"][a] < t["rows"][b])


def test_class_filter_scenes():
    s = ps.clustered(600, seed=600)
    full = nr.walk(s)
    for classes in ([1], [0, 2], [1, 7], [7], []):
        k = nr.walk(s, classes=classes)
        assert set(s["cls"][k].tolist()) <= set(float(c) for c in classes)
        # per-class NMS: filtering commutes with the walk as long as no cut bites
        assert np.array_equal(k, full[np.isin(s["cls"][full], classes)])
    assert 0 < len(nr.walk(s, classes=[1])) < len(full) and len(nr.walk(s, classes=[7])) == len(nr.walk(s, classes=[])) == 0
    assert len(nr.no_class(s, 1)["score"]) < 600 and len(nr.walk(nr.no_class(s, 1), classes=[1])) == 0
    # the max_det cut: the filter comes first, so the other classes take none of the slots
    sep = ps.separated()
    k = nr.walk(sep, classes=[3, 4], max_det=50)
    assert len(k) == 50 and not np.array_equal(k, nr.walk(sep, max_det=50)) and set(sep["cls"][nr.walk(sep, max_det=50)].tolist()) - {3.0, 4.0}


def test_filter_before_cut_scene():
    s = nr.filter_before_cut(4)
    top = np.argsort(-s["score"])[:4]
    assert (s["cls"][top] == 0).all() and (s["cls"][np.argsort(-s["score"])[4:]] > 0).all()
    k = nr.walk(s, classes=[1, 2], max_nms=4)
    assert len(k) == 4 and np.array_equal(k, np.argsort(-s["score"])[4:8])
    cut_first = nr.walk(s, max_nms=4)
    assert len(cut_first) == 4 and not nr.class_filter(s["cls"][cut_first], [1, 2]).any()


@pytest.mark.parametrize("conf", [0.01, 0.25])
@pytest.mark.parametrize("gi", range(len(ps.GRIDS)))
def test_multi_label_scenes(gi, conf):
    sc = nr.ml_scene(gi, conf)
    na, no = sc["na"], sc["no"]
    nc = no - 5
    for h in sc["heads"]:
        obj, c = nr.conf64(h, na, no)
        assert (np.abs(obj - conf) >= ps.BAND).all() and (np.abs(c - conf) >= ps.BAND).all()
    dec = nr.decode(sc)
    per_row = {}
    for b in range(sc["B"]):
        ml, best = nr.candidates(dec[b], conf, True), nr.candidates(dec[b], conf, False)
        if nc == 1:
            assert all(np.array_equal(ml[k], best[k]) for k in ml)         # multi_label &= nc > 1
            continue
        assert len(set(zip(ml["rows"].tolist(), ml["cls"].tolist()))) == len(ml["rows"]) > len(best["rows"]) > 0
        assert set(best["rows"].tolist()) == set(ml["rows"].tolist())      # a row has a candidate iff its best class passes
        for r in range(dec.shape[1]):
            per_row[(b, r)] = int((ml["rows"] == r).sum())
    if nc > 1:
        assert {0, 1, 2, nc} <= set(per_row.values())
        # the planted rows: bit-equal logits -> bit-equal scores inside the row, candidates in class order
        ml = nr.candidates(dec[0], conf, True)
        order = nr.thread_order_rows(sc, 0)
        nx = sc["shapes"][0][1]
        for (b, l, y, x, an), k in nr.planted_rows(gi).items():
            m = ml["rows"] == order[(y * na + an) * nx + x]
            assert m.sum() == k and len(set(ml["score"][m].tolist())) <= 1 and (np.diff(ml["cls"][m]) > 0).all()
        # multi-label and agnostic together: the planted row with all its classes passing keeps its lowest class alone
        r_all = order[(1 * na + 0) * nx + 1]
        k = nr.walk(ml, agnostic=True)
        assert ml["cls"][k][ml["rows"][k] == r_all].tolist() == [0.0] and (ml["rows"][nr.walk(ml)] == r_all).sum() == nc


def test_multi_label_cap_scene():
    sc = nr.ml_scene(3, 0.25, obj_logit=6.0)
    cap, pairs = nr.straddle_cap(sc, 0.25)
    assert cap >= 64 and len(pairs) == cap and len(set(pairs)) == cap
    dec = nr.decode(sc)
    ml0 = nr.candidates(dec[0], 0.25, True)
    n_last = int((ml0["rows"] == pairs[-1][0]).sum())
    written = sum(1 for r, _ in pairs if r == pairs[-1][0])
    assert 0 < written < n_last                                            # the last row below cap is cut inside its reservation
    assert all(len(nr.candidates(dec[b], 0.25, True)["rows"]) > 10 * cap for b in range(sc["B"]))
