"""UAVMOT without a GPU: the CPU build of the tracker workgroup programs (tests/_hostsim) with tracker kind 5 against the reference's golden vectors
(tests/golden/tracker_uavmot_*.npz, tests/golden/make_golden_uavmot.py) and, where the reference sources exist, against the live reference on random
scenes; the port's matching.structure_* functions against the reference's, and the float64 pins of the AMF arithmetic against numpy / scipy."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import _hostsim as hs
from tests import tracker_case as tc

NAMES = tc.NAMES["uavmot"]
load_golden = functools.partial(tc.load_golden, "uavmot")


def replay(want, arena_frames=0, n_frames=None):
    """the host build over the scene, every frame compared with `want` (a golden / the live reference's frames)"""
    trk = hs.HostSimTracker("uavmot", conf_thresh=want["conf"], kalman_format=want.get("kalman_format", "default"))
    return tc.replay_host(trk, want, arena_frames, n_frames)


@pytest.mark.parametrize("name", NAMES)
def test_hostsim_uavmot_matches_reference_golden(name):
    g = load_golden(name)
    replay(g)


@pytest.mark.parametrize("name,frames", [("default", 8), ("misses", 16), ("crowd", 5), ("sparse3", 7)])
def test_hostsim_uavmot_with_list_arena_matches_reference_golden(name, frames):
    g = load_golden(name)
    replay(g, arena_frames=frames)


def test_hostsim_uavmot_without_fast_scratch_matches_reference_golden(monkeypatch):
    """every work array in the state blob (the placement branches a workgroup without enough LDS takes): the centres of the AMF pass behind its vectors"""
    g = load_golden("crowd")
    hs.lib().hs_set_fast_bytes(0)
    try:
        replay(g, n_frames=6)
    finally:
        hs.reset_fast_bytes()


def test_uavmot_goldens_cover_the_scenes():
    """the goldens hold what UAVMOT's branches need: long lost lists, one-object frames (the "(0, 0) only" gate), a crowd"""
    g = load_golden("misses")
    assert max(len(x) for x in g["lost"]) >= 10
    s1 = load_golden("sparse1")
    assert max(len(d) for d in s1["dets"]) <= 2 and len(s1["frames"]) == 150
    assert max(len(x) for x in load_golden("crowd")["lost"]) >= 20


def test_hostsim_uavmot_differs_from_bytetrack():
    """kind 5 is not ByteTrack: on the CLI's sequence the two disagree (the 0.7 / AMF first association, the index quirk)"""
    g = load_golden("default")
    uav = hs.HostSimTracker("uavmot", conf_thresh=g["conf"])
    u = [uav.update(d) for d in g["dets"][:40]]
    b = hs.run("bytetrack", g["dets"][:40])
    assert any([r[0] for r in x] != [r[0] for r in y] or not np.array_equal(np.array([r[1] for r in x]), np.array([r[1] for r in y])) for x, y in zip(u, b))


def test_hostsim_uavmot_pool_overflow_sets_status():
    trk = hs.HostSimTracker("uavmot", cap_t=16)
    from yolov7_tracker_amd import synth
    with pytest.raises(RuntimeError, match="capacity"):
        for d in synth.make_detections(5, 40, seq_idx=3):
            trk.update(d)


# ---- the float64 pins of the AMF arithmetic (matching.py:284-388 on numpy / scipy) ----
def _libm():
    m = ctypes.CDLL("libm.so.6")
    m.fma.restype = ctypes.c_double
    m.fma.argtypes = [ctypes.c_double] * 3
    return m


def test_pin_float64_distance_is_fused():
    """np.linalg.norm([|dx|, |dy|]) of float64 values == sqrt(fma(|dy|, |dy|, |dx| * |dx|)); plain sqrt(dx^2 + dy^2) differs on some"""
    fma = _libm().fma
    rng = np.random.default_rng(7)
    p = np.abs(rng.uniform(-600, 600, (20000, 2)))
    plain_differs = 0
    for a, b in p:
        want = np.linalg.norm([a, b])
        assert math.sqrt(fma(b, b, a * a)) == want
        plain_differs += math.sqrt(a * a + b * b) != want
    assert plain_differs > 0


def test_pin_float32_distance():
    """detections: get_xy() is float32 (tl + wh // 2), so norm([|dx|, |dy|]) is float32 arithmetic: sqrtf(fl(dx^2) + fl(dy^2))"""
    rng = np.random.default_rng(8)
    p = np.abs(rng.uniform(-600, 600, (20000, 2))).astype(np.float32)
    p[:10000] = np.round(p[:10000] * 2) / 2
    for a, b in p:
        want = np.linalg.norm([a, b])
        assert want.dtype == np.float32 and np.sqrt(np.float32(a * a) + np.float32(b * b)) == want


def test_pin_cosine_distance():
    """cdist(u, v, "cosine") == 1 - clip(dot / (sqrt(uu) sqrt(vv)), -1, 1), unfused left-to-right sums; the clip matters for equal directions"""
    from scipy.spatial.distance import cdist
    from yolov7_tracker_amd.tracker import matching as pm
    rng = np.random.default_rng(9)
    T = np.abs(rng.uniform(0, 400, (300, 3)))
    T[:, 2] = rng.integers(0, 181, 300)
    T[:50] = 1e-4
    T[50:80, 2] = 1e-4
    D = np.abs(rng.uniform(0, 400, (300, 3)))
    D[:, 2] = rng.integers(0, 181, 300)
    D[:40] = 1e-4
    D[40:60] = T[80:100] * 2
    want = np.maximum(0.0, cdist(T, D, "cosine"))
    assert np.array_equal(pm._structure_cosine(T, D), want)


def test_pin_mixing_weight():
    assert 1 - 0.98 == 0.020000000000000018 != 0.02


def test_pin_atan2_exact_directions():
    """the exact directions the device pins (csrc/y7t_track_step.h: y7t_atan2_pinned) are what math.atan2 returns"""
    pi, pi_2, pi_4, pi3_4 = 3.141592653589793, 1.5707963267948966, 0.7853981633974483, 2.356194490192345
    for v in (0.5, 1.0, 3.5, 399.5, 1e-3):
        assert math.atan2(v, 0.0) == pi_2 and math.atan2(-v, 0.0) == -pi_2 and math.atan2(v, -0.0) == pi_2
        assert math.atan2(0.0, v) == 0.0 and math.atan2(0.0, -v) == pi and math.atan2(-0.0, -v) == -pi
        assert math.atan2(v, v) == pi_4 and math.atan2(-v, v) == -pi_4 and math.atan2(v, -v) == pi3_4 and math.atan2(-v, -v) == -pi3_4
    assert [int(a * 180 / math.pi) for a in (pi_2, pi_4, pi3_4, pi, -pi_2)] == [90, 45, 135, 180, -90]


# ---- the port's structure functions against the reference's ----
from oracle import ref_harness  # noqa: E402

needs_ref = pytest.mark.skipif(not ref_harness.available(), reason="reference sources not present")


class _T:
    """a track as structure_representation sees it: mean[0:2]"""
    def __init__(self, xy):
        self.mean = np.array([xy[0], xy[1], 0.5, 100.0, 0, 0, 0, 0], np.float64)


def _scenes(rng):
    out = []
    for k in range(12):
        n = int(rng.integers(1, 60))
        if k % 3 == 0:      # the half-pixel lattice: exact directions, equal distances, ties of max / min
            xy = np.round(rng.uniform(0, 900, (n, 2)) * 2) / 2
            xy[: n // 3] = xy[0] + np.round(rng.uniform(-30, 30, (n // 3, 2))) / 2
        elif k % 3 == 1:    # the 400 px boundary
            xy = rng.uniform(0, 1200, (n, 2))
            xy[1::2] = xy[0] + np.array([400.0, 0.0])
            xy[2::3] = xy[0] + np.array([0.0, 399.5])
        else:
            xy = rng.uniform(0, 1500, (n, 2))
        out.append(xy)
    return out


@needs_ref
def test_structure_functions_equal_reference():
    """structure_representation (both modes), angle and structure_similarity_distance (its numpy restatement -- the port runs it on the device) bit for
    bit against the reference's, on random, lattice and boundary centres"""
    from yolov7_tracker_amd.tracker import matching as pm
    from yolov7_tracker_amd.tracker.uavmot import AMF_STrack
    mg = tc.maker("uavmot")
    mod = mg.load_uavmot()
    rm = ref_harness.load_tracker().matching
    rng = np.random.default_rng(11)
    for xy in _scenes(rng):
        tracks = [_T(p) for p in xy]
        dets_r = [mod.AMF_STrack(0, np.array([x, y, 2 * (i % 7) + 1, 3 + i % 5], np.float32), 0.9) for i, (x, y) in enumerate(xy)]
        dets_p = [AMF_STrack(0, np.array([x, y, 2 * (i % 7) + 1, 3 + i % 5], np.float32), 0.9) for i, (x, y) in enumerate(xy)]
        for r, p in zip(dets_r, dets_p):
            assert r.get_xy().dtype == p.get_xy().dtype and np.array_equal(r.get_xy(), p.get_xy())
        want_t = rm.structure_representation(tracks)
        want_d = rm.structure_representation(dets_r, mode="detection")
        assert np.array_equal(pm.structure_representation(tracks), want_t)
        assert np.array_equal(pm.structure_representation(dets_p, mode="detection"), want_d)
        want = rm.structure_similarity_distance(tracks, dets_r)
        got = pm._structure_cosine(pm._structure_vectors(pm._track_xy(tracks), np.float64), pm._structure_vectors(pm._det_xy(dets_p), np.float32))
        assert np.array_equal(got, want)
    for _ in range(2000):
        v1, v2 = np.round(rng.uniform(-50, 50, 2) * 2) / 2, rng.uniform(-50, 50, 2)
        assert pm.angle(v1, v2) == rm.angle(v1, v2)


@needs_ref
@pytest.mark.parametrize("seed", range(12))
def test_hostsim_uavmot_matches_live_reference(seed):
    from yolov7_tracker_amd import synth
    mg = tc.maker("uavmot")
    rng = np.random.default_rng(3000 + seed)
    nf, nobj = int(rng.integers(20, 50)), int(rng.integers(1, 120))
    extra = {"bounce": bool(rng.integers(0, 2)), "miss": float(rng.uniform(0.0, 0.4))}
    dets = synth.make_detections(nf, nobj, seq_idx=300 + seed, **extra)
    if seed % 3 == 0:
        dets = [np.zeros((0, 6), np.float32) if rng.random() < 0.15 else d for d in dets]
    conf = [0.2, 0.3, 0.4, 0.25][seed % 4]
    kform = "botsort" if seed % 5 == 4 else "default"
    ref = mg.run_reference(dets, conf, kform)
    replay(tc.want_from_reference(ref, dets=dets, conf=conf, kalman_format=kform), arena_frames=(7 if seed % 2 else 0))


@needs_ref
def test_hostsim_uavmot_update_without_detection_matches_live_reference():
    """frames without detections (update_without_detection, basetrack.py:489-537 -- ByteTrack's) between ordinary ones"""
    from yolov7_tracker_amd import synth
    mg = tc.maker("uavmot")
    dets = list(synth.make_detections(30, 40, seq_idx=320, miss=0.2))
    dets[8:8] = [None, None]
    dets[20:20] = [None]
    ref = mg.run_reference(dets, 0.2)
    want = tc.want_from_reference(ref, dets=dets, conf=0.2)
    assert len(want["frames"][8][0]) > 0
    replay(want)
