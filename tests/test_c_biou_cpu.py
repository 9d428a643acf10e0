"""C-BIoU without a GPU: the CPU build of the tracker workgroup programs (tests/_hostsim) with tracker kind 4 against the reference's golden vectors
(tests/golden/tracker_c_biou_*.npz, tests/golden/make_golden_c_biou.py) and, where the reference sources exist, against the live reference on random
scenes; the port's matching.buffered_iou_distance against the reference's."""
import functools

import numpy as np
import pytest

from tests import _hostsim as hs
from tests import tracker_case as tc

NAMES = tc.NAMES["c_biou"]
load_golden = functools.partial(tc.load_golden, "c_biou")


def replay(want, arena_frames=0):
    """the host build over the scene, every frame compared with `want` (a golden / the live reference's frames): tlwh exactly, C-BIoU has no Kalman filter"""
    return tc.replay_host(hs.HostSimTracker("c_biou", conf_thresh=want["conf"]), want, arena_frames, exact=True)


@pytest.mark.parametrize("name", NAMES)
def test_hostsim_c_biou_matches_reference_golden(name):
    g = load_golden(name)
    replay(g)


@pytest.mark.parametrize("name,frames", [("default", 8), ("misses", 16), ("crowd", 5), ("empty", 3)])
def test_hostsim_c_biou_with_list_arena_matches_reference_golden(name, frames):
    g = load_golden(name)
    replay(g, arena_frames=frames)


def test_hostsim_c_biou_misses_golden_exercises_the_buffer():
    """the 30 %-miss golden holds what the tracker's quirks need: re-found tracks (stale δ), a full 6-box buffer, a lost list that only grows by misses"""
    g = load_golden("misses")
    assert max(len(x) for x in g["lost"]) >= 20
    assert len(g["frames"]) == 300 and max(int(f[0].max()) for f in g["frames"] if len(f[0])) > 300


def test_hostsim_c_biou_update_without_detection():
    """an empty pool only advances the frame; a non-empty one is refused with Y7T_ERR_PREDICT (16), the state unchanged"""
    trk = hs.HostSimTracker("c_biou")
    assert trk.update(None) == []
    assert trk.update(np.zeros((0, 6), np.float32)) == []
    d = np.array([[10, 10, 60, 90, 0.9, 0], [200, 40, 260, 160, 0.8, 1]], np.float32)
    assert len(trk.update(d)) == 0      # frame 3: new tracks, not activated
    assert len(trk.update(d)) == 2
    lo = tc.layout(trk.cap_t, trk.cap_d)
    frame = lambda: int(trk.blob[lo["hdr_frame_id"]:lo["hdr_frame_id"] + 4].view(np.int32)[0])      # noqa: E731
    before, lists = frame(), tc.id_lists(trk)
    with pytest.raises(RuntimeError, match="status 16"):
        trk.update(None)
    assert frame() == before == 4 and tc.id_lists(trk) == lists


def test_hostsim_c_biou_pool_overflow_sets_status():
    trk = hs.HostSimTracker("c_biou", cap_t=16)
    from yolov7_tracker_amd import synth
    with pytest.raises(RuntimeError, match="capacity"):
        for d in synth.make_detections(5, 40, seq_idx=3):
            trk.update(d)


# ---- against the live reference (where its sources exist) ----
from oracle import ref_harness  # noqa: E402

needs_ref = pytest.mark.skipif(not ref_harness.available(), reason="reference sources not present")


@needs_ref
@pytest.mark.parametrize("seed", range(20))
def test_hostsim_c_biou_matches_live_reference(seed):
    from yolov7_tracker_amd import synth
    mg = tc.maker("c_biou")
    rng = np.random.default_rng(1000 + seed)
    nf, nobj = int(rng.integers(20, 70)), int(rng.integers(5, 140))
    extra = {"bounce": bool(rng.integers(0, 2)), "miss": float(rng.uniform(0.0, 0.4))}
    dets = synth.make_detections(nf, nobj, seq_idx=200 + seed, **extra)
    if seed % 3 == 0:
        dets = [np.zeros((0, 6), np.float32) if rng.random() < 0.15 else d for d in dets]
    conf = [0.2, 0.3, 0.4, 0.25][seed % 4]
    ref = mg.run_reference(dets, conf)
    replay(tc.want_from_reference(ref, dets=dets, conf=conf), arena_frames=(7 if seed % 2 else 0))


@needs_ref
def test_buffered_iou_distance_equals_reference(monkeypatch):
    """matching.buffered_iou_distance of the port: the same tlbr boxes in the same dtypes as the reference's, for detections built by either side and for
    tracks with extrapolated motion states; the IoU itself (a device op in the port) is restated by the oracle here"""
    from oracle import cnative
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker import matching as pm
    from yolov7_tracker_amd.tracker.c_biou_tracker import C_BIoUSTrack
    mg = tc.maker("c_biou")
    mod = mg.load_c_biou()
    rm = ref_harness.load_tracker().matching
    monkeypatch.setattr(pm, "_cost", lambda a, b: 1 - cnative.bbox_overlaps(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)))
    # tracks of a reference run (full buffers, extrapolated states, lost tracks) against the next frame's detections
    dets = synth.make_detections(60, 50, seq_idx=41, miss=0.3, bounce=True)
    mod.BaseTrack._count = 0
    trk = mod.C_BIoUTracker(ref_harness.make_opts(), frame_rate=30)
    for d in dets[:-1]:
        trk.update(d, None)
    tracks = trk.tracked_stracks + trk.lost_stracks
    last = dets[-1]
    ref_dets = [mod.C_BIoUSTrack(c, mod.C_BIoUSTrack.tlbr2tlwh(b), s) for c, b, s in zip(last[:, -1], last[:, :4], last[:, 4])]
    port_dets = [C_BIoUSTrack(c, C_BIoUSTrack.tlbr2tlwh(b), s) for c, b, s in zip(last[:, -1], last[:, :4], last[:, 4])]
    for r, p in zip(ref_dets, port_dets):
        for a in ("buffer_bbox1", "buffer_bbox2", "motion_state1", "motion_state2", "tlwh", "tlbr"):
            x, y = getattr(r, a), getattr(p, a)
            assert x.dtype == y.dtype and np.array_equal(x, y), a
    for level in (1, 2):
        want = rm.buffered_iou_distance(tracks, ref_dets, level=level)
        assert np.array_equal(pm.buffered_iou_distance(tracks, port_dets, level=level), want)
        assert np.array_equal(pm.buffered_iou_distance(tracks, ref_dets, level=level), want)
    assert pm.buffered_iou_distance([], port_dets).shape == (0, len(port_dets))
