"""UAVMOT without a GPU: the CPU build of the tracker workgroup programs (tests/_hostsim) with tracker kind 5 against the reference's golden vectors
(tests/golden/tracker_uavmot_*.npz, tests/golden/make_golden_uavmot.py) and, where the reference sources exist, against the live reference on random
scenes; the port's matching.structure_* functions against the reference's, and the float64 pins of the AMF arithmetic against numpy / scipy."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import _hostsim as hs
from tests import util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["default", "misses", "sparse1", "sparse3", "crowd", "empty", "conf04", "botsort"]
LIB = os.path.join(os.path.dirname(GOLDEN), "..", "yolov7-tracker_amd", "lib", "liby7t.so")


class UAVHost(hs.HostSimTracker):
    TRACKERS = dict(hs.HostSimTracker.TRACKERS, uavmot=5)


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, "tracker_uavmot_%s.npz" % name))
    off = np.concatenate([[0], np.cumsum(g["det_counts"])])
    dets = [g["dets"][off[i]:off[i + 1]] for i in range(len(g["det_counts"]))]

    def split(counts, flat):
        o = np.concatenate([[0], np.cumsum(counts)])
        return [flat[o[i]:o[i + 1]].tolist() for i in range(len(counts))]
    frames = []
    for f in range(len(dets)):
        sel = g["frame"] == f
        frames.append((g["track_id"][sel], g["tlwh"][sel], g["cls"][sel], g["score"][sel]))
    return dict(dets=dets, frames=frames, tracked=split(g["tracked_counts"], g["tracked_ids"]), lost=split(g["lost_counts"], g["lost_ids"]),
                conf=float(g["conf_thresh"]), kalman_format=str(g["kalman_format"]))


_LAYOUT = {}


def layout(cap_t, cap_d):
    """byte offsets of the pool blob's fields (the product library's y7t_tracker_layout: host code, no device needed)"""
    if (cap_t, cap_d) not in _LAYOUT:
        L = ctypes.CDLL(LIB)
        L.y7t_tracker_layout.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.y7t_tracker_field_name.restype = ctypes.c_char_p
        n = L.y7t_tracker_layout(cap_t, cap_d, None, 0)
        offs = (ctypes.c_int64 * n)()
        L.y7t_tracker_layout(cap_t, cap_d, offs, n)
        _LAYOUT[(cap_t, cap_d)] = {L.y7t_tracker_field_name(i).decode(): int(offs[i]) for i in range(n)}
    return _LAYOUT[(cap_t, cap_d)]


def id_lists(trk):
    """-> (ids of the tracked list, ids of the lost list) of a host pool, in list order"""
    lo, b = layout(trk.cap_t, 1024), trk.blob
    i32 = lambda off, n: b[off:off + 4 * n].view(np.int32)      # noqa: E731
    tid = i32(lo["tid"], trk.cap_t)
    nt, nl = int(i32(lo["hdr_n_tracked"], 1)[0]), int(i32(lo["hdr_n_lost"], 1)[0])
    return tid[i32(lo["tracked"], nt)].tolist(), tid[i32(lo["lost"], nl)].tolist()


def replay(dets, conf, kalman_format="default", arena_frames=0, want=None):
    """run the host build over `dets`; with `want` (golden / reference frames) compare every frame"""
    trk = UAVHost("uavmot", conf_thresh=conf, kalman_format=kalman_format)
    got = []
    for f, d in enumerate(dets):
        if arena_frames and f % arena_frames == 0:
            assert hs.lib().hs_arena_begin(trk.blob.ctypes.data)
        rows = trk.update(d)
        group_end = not arena_frames or f % arena_frames == arena_frames - 1 or f == len(dets) - 1
        if arena_frames and group_end:
            hs.lib().hs_arena_end(trk.blob.ctypes.data)
        got.append(rows)
        if want is None:
            continue
        ids, tlwh, cls, score = want["frames"][f]
        assert [r[0] for r in rows] == ids.tolist(), "frame %d: ids" % f
        # (the Kalman arithmetic matches the reference to util's tolerance, as for ByteTrack: tests/test_hostsim.py; ids and lists exactly)
        np.testing.assert_allclose(np.array([r[1] for r in rows]).reshape(-1, 4), tlwh, rtol=util.TLWH_RTOL, atol=util.TLWH_ATOL, err_msg="frame %d: tlwh" % f)
        assert np.array_equal(np.array([r[2] for r in rows], np.float32), cls) and np.array_equal(np.array([r[3] for r in rows], np.float32), score)
        if group_end:      # (inside an arena group the lists live in the arena)
            assert id_lists(trk) == (want["tracked"][f], want["lost"][f]), "frame %d: tracked / lost lists" % f
    return got


@pytest.mark.parametrize("name", NAMES)
def test_hostsim_uavmot_matches_reference_golden(name):
    g = load_golden(name)
    replay(g["dets"], g["conf"], g["kalman_format"], want=g)


@pytest.mark.parametrize("name,frames", [("default", 8), ("misses", 16), ("crowd", 5), ("sparse3", 7)])
def test_hostsim_uavmot_with_list_arena_matches_reference_golden(name, frames):
    g = load_golden(name)
    replay(g["dets"], g["conf"], g["kalman_format"], arena_frames=frames, want=g)


def test_hostsim_uavmot_without_fast_scratch_matches_reference_golden(monkeypatch):
    """every work array in the state blob (the placement branches a workgroup without enough LDS takes): the centres of the AMF pass behind its vectors"""
    import ctypes as ct
    g = load_golden("crowd")
    ct.CDLL(hs.build()).hs_set_fast_bytes(0)
    try:
        replay(g["dets"][:6], g["conf"], want=dict(g, frames=g["frames"][:6], tracked=g["tracked"][:6], lost=g["lost"][:6]))
    finally:
        ct.CDLL(hs.build()).hs_set_fast_bytes(int(os.environ.get("Y7T_HOSTSIM_FAST_BYTES", "131072")))


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
    u = replay(g["dets"][:40], g["conf"])
    b = hs.run("bytetrack", g["dets"][:40])
    assert any([r[0] for r in x] != [r[0] for r in y] or not np.array_equal(np.array([r[1] for r in x]), np.array([r[1] for r in y])) for x, y in zip(u, b))


def test_hostsim_uavmot_pool_overflow_sets_status():
    trk = UAVHost("uavmot", cap_t=16)
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


def _ref_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_uavmot", os.path.join(GOLDEN, "make_golden_uavmot.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


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
    mg = _ref_module()
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
    mg = _ref_module()
    rng = np.random.default_rng(3000 + seed)
    nf, nobj = int(rng.integers(20, 50)), int(rng.integers(1, 120))
    extra = {"bounce": bool(rng.integers(0, 2)), "miss": float(rng.uniform(0.0, 0.4))}
    dets = synth.make_detections(nf, nobj, seq_idx=300 + seed, **extra)
    if seed % 3 == 0:
        dets = [np.zeros((0, 6), np.float32) if rng.random() < 0.15 else d for d in dets]
    conf = [0.2, 0.3, 0.4, 0.25][seed % 4]
    kform = "botsort" if seed % 5 == 4 else "default"
    ref = mg.run_reference(dets, conf, kform)
    want = dict(frames=[(np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float64).reshape(-1, 4),
                         np.array([r[2] for r in rows], np.float32), np.array([r[3] for r in rows], np.float32)) for rows, _, _ in ref],
                tracked=[t for _, t, _ in ref], lost=[lo for _, _, lo in ref])
    replay(dets, conf, kform, arena_frames=(7 if seed % 2 else 0), want=want)


@needs_ref
def test_hostsim_uavmot_update_without_detection_matches_live_reference():
    """frames without detections (update_without_detection, basetrack.py:489-537 -- ByteTrack's) between ordinary ones"""
    from yolov7_tracker_amd import synth
    mg = _ref_module()
    dets = list(synth.make_detections(30, 40, seq_idx=320, miss=0.2))
    dets[8:8] = [None, None]
    dets[20:20] = [None]
    ref = mg.run_reference(dets, 0.2)
    want = dict(frames=[(np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float64).reshape(-1, 4),
                         np.array([r[2] for r in rows], np.float32), np.array([r[3] for r in rows], np.float32)) for rows, _, _ in ref],
                tracked=[t for _, t, _ in ref], lost=[lo for _, _, lo in ref])
    assert len(want["frames"][8][0]) > 0
    replay(dets, 0.2, want=want)
