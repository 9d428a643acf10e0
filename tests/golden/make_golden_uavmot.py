"""tests/golden/make_golden_uavmot.py -- regenerates the committed UAVMOT golden vectors (tracker_uavmot_*.npz).

Runs ONLY in the build container (needs the reference sources): it imports the reference's own tracker/uavmot.py through
oracle/ref_harness.py (its unused ReID Extractor and torchvision.ops are stubbed there) and records what UAVMOT.update returns on
seeded synthetic scenes, in the format of make_golden_c_biou.py's goldens, plus the ids of the tracked / lost lists after every frame.

    python tests/golden/make_golden_uavmot.py [name,...]
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from yolov7_tracker_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    # name, n_frames, n_obj, seq_idx, extra make_detections arguments, conf_thresh, empty_every (frames with zero rows), kalman_format
    ("default", 100, 80, 0, {}, 0.2, 0, "default"),                          # the tracker CLI's synthetic sequence (--dataset synthetic --synthetic_dets)
    ("misses", 200, 60, 42, {"miss": 0.3, "bounce": True}, 0.2, 0, "default"),   # long lost lists: the second association's index quirk marks many of them
    ("sparse1", 150, 1, 43, {"miss": 0.15, "bounce": True}, 0.2, 0, "default"),   # one object: the "(0, 0) only" gate keeps the 0.7 solve
    ("sparse3", 150, 3, 44, {"miss": 0.2, "bounce": True}, 0.2, 0, "default"),    # two or three objects: both branches of the gate
    ("crowd", 20, 500, 45, {}, 0.2, 0, "default"),                           # large components, ties, many neighbours within 400 px
    ("empty", 60, 40, 46, {}, 0.2, 7, "default"),                            # frames with zero rows
    ("conf04", 80, 60, 47, {}, 0.4, 0, "default"),                           # another detection threshold
    ("botsort", 100, 60, 48, {"bounce": True}, 0.2, 0, "botsort"),           # kalman_format botsort (xywh means, floor-divided centres)
]


def load_uavmot():
    """-> the reference's uavmot module.  Its import brings its OWN basetrack / matching modules; matching is replaced by the harness's
    (the np.float shim, lap and cython_bbox restated in oracle/cnative.py)."""
    with ref_harness._patched_modules([os.path.join(ref_harness.REF_ROOT, "tracker")]):
        for name in ("basetrack", "matching", "uavmot"):
            sys.modules.pop(name, None)
        mod = importlib.import_module("uavmot")
        sys.modules.pop("uavmot", None)
    mod.matching = ref_harness.load_tracker().matching
    mod.STrack.__init__.__globals__["matching"] = mod.matching      # (its basetrack's update_without_detection / remove_duplicate_stracks too)
    return mod


def scene(nf, nobj, seq, extra, empty_every):
    dets = synth.make_detections(nf, nobj, seq_idx=seq, **extra)
    if empty_every:
        dets = [np.zeros((0, 6), np.float32) if i % empty_every == empty_every - 1 else d for i, d in enumerate(dets)]
    return dets


def run_reference(dets, conf_thresh=0.2, kalman_format="default", track_buffer=30, mod=None):
    """-> per frame (rows, tracked ids, lost ids); rows = [(id, tlwh float64, cls, score)] of the tracks update() returns.
    A frame given as None goes through update_without_detection."""
    mod = mod or load_uavmot()
    next(c for c in mod.STrack.__mro__ if c.__name__ == "BaseTrack")._count = 0      # (uavmot.py imports STrack, not BaseTrack)
    trk = mod.UAVMOT(ref_harness.make_opts(conf_thresh=conf_thresh, track_buffer=track_buffer, kalman_format=kalman_format), frame_rate=30)
    out = []
    for d in dets:
        if d is None:
            cur = trk.update_without_detection(None, np.zeros((1, 1, 3), np.uint8))
        else:
            cur = trk.update(np.asarray(d, dtype=np.float32), np.zeros((1, 1, 3), np.uint8))
        rows = [(int(t.track_id), np.asarray(t.tlwh, dtype=np.float64).copy(), float(t.cls), float(t.score)) for t in cur]
        out.append((rows, [int(t.track_id) for t in trk.tracked_stracks], [int(t.track_id) for t in trk.lost_stracks]))
    return out


def flat_lists(lists):
    return np.array([len(x) for x in lists], np.int32), np.array([i for x in lists for i in x], np.int32)


def main(only=None):
    mod = load_uavmot()
    for name, nf, nobj, seq, extra, conf, empty, kform in CASES:
        if only and name not in only:
            continue
        dets = scene(nf, nobj, seq, extra, empty)
        ref = run_reference(dets, conf, kform, mod=mod)
        fr, ids, tlwh, cls, score = [], [], [], [], []
        for f, (rows, _, _) in enumerate(ref):
            for r in rows:
                fr.append(f); ids.append(r[0]); tlwh.append(r[1]); cls.append(r[2]); score.append(r[3])
        tc, tl = flat_lists([x[1] for x in ref])
        lc, ll = flat_lists([x[2] for x in ref])
        path = os.path.join(HERE, "tracker_uavmot_%s.npz" % name)
        np.savez_compressed(path, tracker=np.array("uavmot"), det_counts=np.array([len(d) for d in dets], np.int32),
                            dets=np.concatenate(dets, 0).astype(np.float32), frame=np.array(fr, np.int32), track_id=np.array(ids, np.int32),
                            tlwh=np.array(tlwh, np.float64).reshape(-1, 4), cls=np.array(cls, np.float32), score=np.array(score, np.float32),
                            tracked_counts=tc, tracked_ids=tl, lost_counts=lc, lost_ids=ll, conf_thresh=np.array(conf),
                            kalman_format=np.array(kform), numpy_version=np.array(np.__version__), scene=np.array([nf, nobj, seq], np.int64))
        print(name, "rows", len(ids), "max id", max(ids) if ids else 0, "lost at the end", lc[-1], "bytes", os.path.getsize(path), flush=True)


if __name__ == "__main__":
    assert ref_harness.available(), "needs the reference sources"
    main(sys.argv[1].split(",") if len(sys.argv) > 1 else None)
