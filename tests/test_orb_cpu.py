"""CPU: the feature-based camera-motion estimate (GMC('features'); DESIGN.md section 4 "GMC / features").  The host build of the kernel bodies
(tests/_hostsim/orb.py) against the NumPy restatement (tests/orb_np.py), ARRAY-EQUAL stage by stage on the fixtures of tests/orb_scenes.py; the pattern header; the
degenerate cases; the state handling of the GMC class; and the restatement's own distance from the planted motion."""
import numpy as np
import pytest

from tests import orb_np, orb_scenes as sc

NAMES = list(sc.FIXTURES)


@pytest.fixture(scope="module")
def hs():
    from tests._hostsim import orb
    orb.lib()
    return orb


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def host_run(hs, name):
    """-> (taps of frame 0, taps of frame 1 with the estimate's arrays, warp, status)"""
    (H, W), ds, cap = sc.FIXTURES[name][0], sc.FIXTURES[name][1], sc.FIXTURES[name][5]
    h, w = H // ds, W // ds
    be = hs.HostFeatures()
    f = sc.frames(name)[0]
    a = be.extract(f[0], ds, sc.dets(name), cap)
    ta = hs.read_taps(be.workspace(h, w, cap).copy(), a, h, w, cap)
    b = be.extract(f[1], ds, sc.dets(name), cap)
    warp, status = be.estimate(a, b, h, w, ds, cap)
    return ta, hs.read_taps(be.workspace(h, w, cap), b, h, w, cap), warp, status


def check_extraction(got, want):
    assert got["h"] == want["h"] and got["w"] == want["w"]
    assert np.array_equal(got["plane"], want["plane"])
    assert np.array_equal(got["scores"], want["scores"])
    assert np.array_equal(got["keep"], want["keep"]) and np.array_equal(got["rowcnt"], want["keep"].sum(1))
    assert got["total"] == want["total"] and got["truncated"] == want["truncated"] and got["n"] == len(want["kp"])
    assert np.array_equal(got["kp"], want["kp"])
    assert np.array_equal(got["moments"], want["moments"])
    assert np.array_equal(got["smooth"], want["smooth"])
    assert np.array_equal(got["desc"], want["desc"])


def check_estimate(taps, warp, status, want):
    n_prev, n_good = int(want["status"][0]), int(want["status"][2])
    assert np.array_equal(status, want["status"])
    assert np.array_equal(taps["matches"][:n_prev], want["matches"])
    assert taps["est"]["n_good"] == n_good and taps["est"]["n_first"] == want["n_first"] and np.array_equal(taps["good"][:n_good], want["good"])
    assert np.array_equal(taps["counts"], want["counts"]) and taps["est"]["winner"] == want["winner"]
    assert same_bits(warp, want["warp"])


def test_pattern_header_regenerates_identically():
    assert open(orb_np.PATTERN_H).read() == orb_np.pattern_header_text()
    p = orb_np.read_pattern()
    assert np.array_equal(p, orb_np.generate_pattern()) and np.abs(p).max() == 13 and len(np.unique(p, axis=0)) > 250


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_restatement_stage_by_stage(name, hs):
    ta, tb, warp, status = host_run(hs, name)
    a, b = sc.extracted(name)
    check_extraction(ta, a)
    check_extraction(tb, b)
    check_estimate(tb, warp, status, sc.estimated(name))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_counts_and_planted_truth(name):
    """the restatement alone: the recorded counts, enough matches on every ordinary fixture, and its warp within twice the recorded distance from the planted one"""
    a, b = sc.extracted(name)
    e = sc.estimated(name)
    got = (len(a["kp"]), len(b["kp"]), int(e["status"][2]), int(e["status"][3]))
    print(name, got, "flag", e["status"][4], "truth error", sc.truth_error(name, e["warp"]), "recorded", sc.TRUTH_ERR[name])
    assert got == sc.COUNTS[name] and e["status"][4] == orb_np.OK
    if name in sc.ORDINARY:
        assert got[2] >= 30 and got[3] >= 20 and not a["truncated"] and not b["truncated"]
    rot, tr = sc.truth_error(name, e["warp"])
    assert rot <= 2 * sc.TRUTH_ERR[name][0] and tr <= 2 * sc.TRUTH_ERR[name][1]
    assert abs(rot - sc.TRUTH_ERR[name][0]) <= 0.01 * sc.TRUTH_ERR[name][0] + 1e-6      # (the record is the measurement)


def test_fixtures_reach_what_they_are_for():
    a, b = sc.extracted("wide")
    assert a["w"] > 4 * 64 and len(a["kp"]) > 256 and len(b["kp"]) > 256                    # several FAST tiles; more than a matching tile and a wave
    a, b = sc.extracted("capped")
    assert a["truncated"] and b["truncated"] and a["total"] > 150 == len(a["kp"]) and sc.estimated("capped")["status"][5] == 3
    assert np.array_equal(a["kp"], sc.extracted("wide")[0]["kp"][:150])
    a, c = sc.extracted("boxes")[0], sc.extracted("wide")[0]
    assert 0 < len(a["kp"]) < len(c["kp"]) and set(map(tuple, a["kp"])) < set(map(tuple, c["kp"]))
    boxes = orb_np.det_boxes(sc.BOXES, 2)
    assert (boxes < 0).any()                                                                 # the negative corners: slices from the far end, here empty ones
    inside = lambda k, p: boxes[k][0] <= p[0] < boxes[k][2] and boxes[k][1] <= p[1] < boxes[k][3]
    assert not any(inside(0, p) or inside(3, p) for p in a["kp"]) and any(inside(0, p) for p in c["kp"])
    assert any(0 <= p[0] < boxes[1][2] and boxes[1][1] <= p[1] < boxes[1][3] for p in a["kp"])      # box 1 starts at -20: Python's slice [-20:65] of 260 is empty


def test_integer_inlier_test_against_python_integers():
    good = sc.estimated("wide")["good"]
    rows = orb_np.all_hypotheses(good)
    for k in list(range(40)) + [sc.estimated("wide")["winner"], 1999]:
        assert np.array_equal(rows[k], orb_np.hypothesis_inliers(good, k)), k
    far = good.copy()
    far[:, :2] = far[:, :2] * 31 % 8191                                                      # scattered over the largest plane: the guard before the squares matters
    far[:, 2:] = far[:, 2:] * 29 % 8191
    rows = orb_np.all_hypotheses(far)
    for k in range(40):
        assert np.array_equal(rows[k], orb_np.hypothesis_inliers(far, k)), k


def test_hash_picks_and_statistics(hs):
    for n in (5, 6, 257, 8192):
        k = np.arange(2000)
        for c in (0, 1):
            p = orb_np.pick(k, c, n)
            assert p.min() >= 0 and p.max() < n and [hs.lib().hs_orb_pick(int(i), c, n) for i in (0, 1, 7, 1999)] == [int(p[i]) for i in (0, 1, 7, 1999)]
    d = np.array([3, -7, 12, 5, 5, -1, 0, 44], np.int64)
    m, s = orb_np.mean_std(d)
    assert m == d.mean() and abs(s - d.std()) <= 4 * np.finfo(np.float64).eps * s           # np.std's two-pass formula differs in the last bits only


def _first(d, k):
    return dict(d, kp=d["kp"][:k], desc=d["desc"][:k])


def _host_first(state, k):
    s = state.copy()
    s[:4].view(np.int32)[0] = k
    return s


def test_degenerate_cases_give_identity_and_flag(hs):
    name = "ragged"
    (H, W), ds, cap = sc.FIXTURES[name][0], sc.FIXTURES[name][1], 8192
    h, w = H // ds, W // ds
    be = hs.HostFeatures()
    f = sc.frames(name)[0]
    a, b = sc.extracted(name)
    sa, sb = be.extract(f[0], ds, None, cap), be.extract(f[1], ds, None, cap)
    flat = np.full((H, W, 3), 100, np.uint8)
    nf, sf = orb_np.extract(flat, ds), be.extract(flat, ds, None, cap)
    assert len(nf["kp"]) == 0 and sf[:4].view(np.int32)[0] == 0
    cases = [("flat current frame", a, nf, sa, sf, orb_np.NO_MATCHES), ("flat previous frame", nf, b, sf, sb, orb_np.NO_MATCHES),
             ("one current keypoint", a, _first(b, 1), sa, _host_first(sb, 1), orb_np.NO_MATCHES),
             ("four previous keypoints", _first(a, 4), b, _host_first(sa, 4), sb, orb_np.NOT_ENOUGH)]
    for what, na, nb, ha, hb, flag in cases:
        want = orb_np.estimate(na, nb, ds)
        warp, status = be.estimate(ha, hb, h, w, ds, cap)
        assert want["status"][4] == flag and np.array_equal(status, want["status"]) and warp.tolist() == [1, 0, 0, 0, 1, 0] == want["warp"].tolist(), what
    # all pairs degenerate: every match leaves the same previous point (the matcher cannot produce this; the hypotheses alone are run)
    same = np.array([[40, 50, 40 + i, 50 - i] for i in range(8)], np.int64)
    counts, est, warp = hs.ransac(same)
    assert not counts.any() and est["flag"] == orb_np.NO_MODEL and est["n_inliers"] == 0 and warp.tolist() == [1, 0, 0, 0, 1, 0]
    rc, rk, rin = orb_np.ransac(same)
    assert not rc.any() and rk == est["winner"] == 0 and not rin.any()
    # ... and a list with one usable pair direction gives a model from the pairs that are not degenerate
    counts, est, warp = hs.ransac(sc.estimated(name)["good"])
    assert np.array_equal(counts, sc.estimated(name)["counts"]) and est["flag"] == orb_np.OK and same_bits(warp, sc.estimated(name)["warp"])


def test_gmc_class_with_the_host_backend(hs, capsys):
    from yolov7_tracker_amd.tracker.gmc import GMC
    f, planted, dets = sc.sequence(4)
    g = GMC('features', downscale=2, backend=hs.HostFeatures())
    ref = orb_np.Features(2)
    for t in range(3):                                                                       # three frames: the previous state becomes the current one
        got, want = g.apply(f[t], dets[t]), ref.apply(f[t], dets[t])
        assert got.shape == (2, 3) and got.dtype == np.float64 and same_bits(got, want)
        assert g._states[t & 1] is g.prevFrame and np.array_equal(g.prevFrame[32:32 + 32 * len(ref.prev["kp"])].view(np.uint32).reshape(-1, 8), ref.prev["desc"])
        if t == 0:
            assert got.tolist() == np.eye(2, 3).tolist() and g.last_status is None
        else:
            assert np.array_equal(g.last_status, ref.last["status"]) and g.last_status[4] == orb_np.OK and g.last_status[2] >= 30
            assert np.abs(got - np.eye(2, 3)).max() > 0.1                                    # (the camera does move; the bounds on truth are the fixtures')
    on_dev = GMC('features', backend=hs.HostFeatures())
    assert on_dev.apply_device(f[0]).tolist() == [1, 0, 0, 0, 1, 0] and same_bits(on_dev.apply_device(f[1]), _second(f).ravel())
    assert capsys.readouterr().out == ""
    few = GMC('features', backend=hs.HostFeatures(), max_keypoints=4)                       # at most 4 matches: the reference's warning, the identity
    few.apply(f[0])
    assert few.apply(f[1]).tolist() == np.eye(2, 3).tolist() and few.last_status[4] == orb_np.NOT_ENOUGH and few.last_status[5] == 3
    assert capsys.readouterr().out == "Warning: not enough matching points\n"
    with pytest.raises(ValueError, match="frame size"):
        few.apply(f[1][:150])
    for method in ('orb', 'sift', 'file'):
        with pytest.raises(NotImplementedError, match="scope"):
            GMC(method)


def _second(f):
    r = orb_np.Features(2)
    r.apply(f[0])
    return r.apply(f[1])
