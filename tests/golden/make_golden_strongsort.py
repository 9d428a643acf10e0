"""tests/golden/make_golden_strongsort.py -- regenerates the committed StrongSORT golden vectors (tracker_strongsort_*.npz).

Runs ONLY in the build container (needs the reference sources): it imports the reference's own tracker/strongsort.py through
oracle/ref_harness.py -- with two more stubs for what its constructor touches (reid_models.OSNet.osnet_x0_25, reid_models.load_model_tools) -- replaces
its two out-of-scope seams, `get_feature` (the ReID network) by the scene's feature function and `ECC.apply` (OpenCV findTransformECC) by the scene's
warp, and records what StrongSORT.update returns on seeded synthetic scenes: the rows, the ids of the tracked / lost lists after every frame and the
smoothed appearance vectors at the end.  Features are not stored: a file keeps the scene's parameters and tests regenerate them (scene_from_golden).

    python tests/golden/make_golden_strongsort.py [name,...]
"""
import importlib
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from yolov7_tracker_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_FEATURE_FLOATS = 32768      # final_features holds the vectors of the first tracks of the tracked list that fit (a file stays under 400 KB): final_slots_ids names them

CASES = [
    # name, n_frames, n_obj, seq_idx, feature kind, dim, extra make_detections / make_identity_features arguments, warps, gamma, conf_thresh, empty_every, none_every,
    # kalman_format (strongsort = the NSA filter: what tracker/track.py:70-71 sets for this tracker; default: the plain xyah filter the class also accepts)
    ("identity128", 60, 60, 30, "identity", 128, {"miss": 0.2}, True, 0.1, 0.2, 0, 0, "strongsort"),
    ("identity512", 50, 80, 31, "identity", 512, {"miss": 0.3}, True, 0.1, 0.2, 0, 0, "strongsort"),
    ("dim100", 40, 50, 32, "identity", 100, {"noise": 0.4}, False, 0.1, 0.2, 0, 0, "default"),          # the plain-form dimension (not a multiple of the k chunk)
    # box-size features: a dense candidate graph, ties.  The plain filter: with gamma 0.1 such features re-match a track to look-alike boxes hundreds of pixels away, the
    # track picks up a velocity of ~350 px a frame and then coasts as a stale Tracked entry for the rest of the scene, so whatever rounding difference its velocity carries
    # grows by that much every frame.  Recorded with the NSA filter (whose innovation covariance is worse conditioned) the CPU build met the reference's track 64 to
    # 1.5e-6 px at frame 36 and drifted 1.0e-5 px a frame from there: 3.2e-5 px at frame 39 against a tolerance of 3.0e-5 (tests/util.py), ids and lists equal throughout.
    ("boxfeat", 60, 60, 33, "boxfeat", 128, {}, False, 0.1, 0.2, 0, 0, "default"),
    ("crowd300", 20, 300, 34, "identity", 512, {"noise": 0.3}, True, 0.1, 0.2, 0, 0, "strongsort"),
    ("crowd500", 12, 500, 35, "identity", 128, {"noise": 0.3}, False, 0.1, 0.2, 0, 0, "strongsort"),
    ("gamma05", 60, 60, 36, "identity", 128, {}, False, 0.5, 0.2, 0, 0, "default"),
    ("conf04", 80, 60, 37, "identity", 128, {}, False, 0.1, 0.4, 0, 0, "strongsort"),
    ("empty", 60, 40, 38, "identity", 128, {}, False, 0.1, 0.2, 7, 0, "strongsort"),                       # every 7th frame has zero rows
    ("gaps", 60, 60, 39, "identity", 128, {"miss": 0.2}, True, 0.1, 0.2, 0, 5, "strongsort"),              # every 5th frame None -> update_without_detection
]


def make_scene(nf, nobj, seq, kind, dim, extra, warps, empty_every=0, none_every=0, size=1280):
    """-> (dets per frame (None: update_without_detection), feature_fn(boxes) -> (k, dim) float32, warps (nf, 2, 3) or None)"""
    if kind == "identity":
        dets, fn = synth.make_identity_features(nf, nobj, size, seq_idx=seq, dim=dim, **extra)
    else:
        dets = synth.make_detections(nf, nobj, size, seq_idx=seq, **extra)
        fn = lambda b, _d=dim: synth.make_features(b, dim=_d)      # noqa: E731
    if empty_every:
        dets = [np.zeros((0, 6), np.float32) if i % empty_every == empty_every - 1 else d for i, d in enumerate(dets)]
    if none_every:
        dets = [None if i % none_every == none_every - 1 else d for i, d in enumerate(dets)]
    return dets, fn, (synth.make_warps(nf, seq_idx=seq) if warps else None)


def scene_from_golden(g):
    """the scene a golden file was recorded on, regenerated from its parameters (and checked against the recorded detections)"""
    nf, nobj, seq = (int(v) for v in g["scene"])
    extra = {k[5:]: float(g[k]) for k in g.files if k.startswith("feat_") and k not in ("feat_kind", "feat_dim")}
    dets, fn, warps = make_scene(nf, nobj, seq, str(g["feat_kind"]), int(g["feat_dim"]), extra, bool(g["has_warps"]), int(g["empty_every"]), int(g["none_every"]))
    assert np.array_equal(np.concatenate([d for d in dets if d is not None], 0), g["dets"]), "the regenerated scene is not the recorded one"
    assert [-1 if d is None else len(d) for d in dets] == g["det_counts"].tolist()
    return dets, fn, warps


def load_strongsort():
    """-> the reference's strongsort module.  Its import brings its OWN basetrack / matching / botsort modules; matching is replaced by the harness's
    (the np.float shim, lap and cython_bbox restated in oracle/cnative.py)."""
    class _Net:
        def cuda(self):
            return self

        def eval(self):
            return self

    with ref_harness._patched_modules([os.path.join(ref_harness.REF_ROOT, "tracker")]):
        osnet = types.ModuleType("reid_models.OSNet")
        osnet.osnet_x0_25 = lambda *a, **k: _Net()
        tools = types.ModuleType("reid_models.load_model_tools")
        tools.load_pretrained_weights = lambda *a, **k: None
        saved = {k: sys.modules.get(k) for k in ("reid_models.OSNet", "reid_models.load_model_tools")}
        sys.modules["reid_models.OSNet"], sys.modules["reid_models.load_model_tools"] = osnet, tools
        try:
            for name in ("basetrack", "matching", "botsort", "strongsort"):
                sys.modules.pop(name, None)
            mod = importlib.import_module("strongsort")
            for name in ("strongsort", "botsort"):
                sys.modules.pop(name, None)
        finally:
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
    mod.matching = ref_harness.load_tracker().matching
    mod.STrack.__init__.__globals__["matching"] = mod.matching      # (its basetrack's update_without_detection / remove_duplicate_stracks too)
    return mod


def run_reference(dets, feature_fn, warps=None, conf_thresh=0.2, gamma=0.1, kalman_format="default", track_buffer=30, mod=None, timing=None, quirks=None):
    """-> (per frame (rows, tracked ids, lost ids), the tracker); rows = [(id, tlwh float64, cls, score)] of the tracks update() returns.  A frame given
    as None goes through update_without_detection.  timing: a list that receives the seconds every update() took; quirks: one that
    receives per frame (stale Tracked entries of the tracked list, tracks in both lists)."""
    mod = mod or load_strongsort()
    next(c for c in mod.STrack.__mro__ if c.__name__ == "BaseTrack")._count = 0
    trk = mod.StrongSORT(ref_harness.make_opts(conf_thresh=conf_thresh, track_buffer=track_buffer, kalman_format=kalman_format), frame_rate=30, gamma=gamma)
    trk.get_feature = lambda tlbrs, ori_img: feature_fn(tlbrs)
    img = np.zeros((1, 1, 3), np.uint8)
    out = []
    for fi, d in enumerate(dets):
        w = np.eye(2, 3) if warps is None else np.asarray(warps[fi], dtype=np.float64).reshape(2, 3)
        trk.ECC.apply = (lambda raw_frame, detections=None, _w=w: _w)
        t0 = time.perf_counter()
        if d is None:
            cur = trk.update_without_detection(None, img)
        else:
            cur = trk.update(np.asarray(d, dtype=np.float32), img)
        if timing is not None:
            timing.append(time.perf_counter() - t0)
        rows = [(int(t.track_id), np.asarray(t.tlwh, dtype=np.float64).copy(), float(t.cls), float(t.score)) for t in cur]
        out.append((rows, [int(t.track_id) for t in trk.tracked_stracks], [int(t.track_id) for t in trk.lost_stracks]))
        if quirks is not None:      # the index quirk's traces: entries of the tracked list this frame's update did not touch but left Tracked; tracks in both lists
            lost_ids = set(int(t.track_id) for t in trk.lost_stracks)
            quirks.append((0 if d is None else sum(1 for t in trk.tracked_stracks if t.state == mod.TrackState.Tracked and t.frame_id != trk.frame_id),
                           sum(1 for t in trk.tracked_stracks if int(t.track_id) in lost_ids)))
    return out, trk


def flat_lists(lists):
    return np.array([len(x) for x in lists], np.int32), np.array([i for x in lists for i in x], np.int32)


def main(only=None):
    import scipy
    mod = load_strongsort()
    for name, nf, nobj, seq, kind, dim, extra, has_warps, gamma, conf, empty, none, kform in CASES:
        if only and name not in only:
            continue
        dets, fn, warps = make_scene(nf, nobj, seq, kind, dim, extra, has_warps, empty, none)
        times, quirks = [], []
        ref, trk = run_reference(dets, fn, warps, conf, gamma, kform, mod=mod, timing=times, quirks=quirks)
        fr, ids, tlwh, cls, score = [], [], [], [], []
        for f, (rows, _, _) in enumerate(ref):
            for r in rows:
                fr.append(f); ids.append(r[0]); tlwh.append(r[1]); cls.append(r[2]); score.append(r[3])
        tc, tl = flat_lists([x[1] for x in ref])
        lc, ll = flat_lists([x[2] for x in ref])
        keep = trk.tracked_stracks[:max(1, MAX_FEATURE_FLOATS // dim)]
        feats = np.array([t.features[-1] for t in keep])
        assert feats.dtype == np.float32 and all(len(t.features) == 1 for t in trk.tracked_stracks)
        path = os.path.join(HERE, "tracker_strongsort_%s.npz" % name)
        np.savez_compressed(path, tracker=np.array("strongsort"), det_counts=np.array([-1 if d is None else len(d) for d in dets], np.int32),
                            dets=np.concatenate([d for d in dets if d is not None], 0).astype(np.float32), frame=np.array(fr, np.int32),
                            track_id=np.array(ids, np.int32), tlwh=np.array(tlwh, np.float64).reshape(-1, 4), cls=np.array(cls, np.float32),
                            score=np.array(score, np.float32), tracked_counts=tc, tracked_ids=tl, lost_counts=lc, lost_ids=ll, conf_thresh=np.array(conf),
                            gamma=np.array(gamma), kalman_format=np.array(kform), warps=warps if warps is not None else np.zeros((0, 2, 3)),
                            has_warps=np.array(has_warps), numpy_version=np.array(np.__version__), scipy_version=np.array(scipy.__version__),
                            scene=np.array([nf, nobj, seq], np.int64), feat_kind=np.array(kind), feat_dim=np.array(dim), empty_every=np.array(empty),
                            none_every=np.array(none), final_slots_ids=np.array([int(t.track_id) for t in keep], np.int32), final_features=feats,
                            ref_ms_per_frame=np.array(1e3 * float(np.median(times))), stale_counts=np.array([q[0] for q in quirks], np.int32),
                            both_counts=np.array([q[1] for q in quirks], np.int32), **{"feat_" + k: np.array(v) for k, v in extra.items()})
        print(name, "rows", len(ids), "max id", max(ids) if ids else 0, "tracked / lost at the end", tc[-1], lc[-1], "reference ms per frame (median) %.2f" % (1e3 * np.median(times)),
              "largest frame %d x %d" % (max(a + b for a, b in zip(tc, lc)), max(len(d) for d in dets if d is not None)), "stale / both-lists entries over the frames", sum(q[0] for q in quirks), sum(q[1] for q in quirks), "bytes", os.path.getsize(path), flush=True)


if __name__ == "__main__":
    assert ref_harness.available(), "needs the reference sources"
    main(sys.argv[1].split(",") if len(sys.argv) > 1 else None)
