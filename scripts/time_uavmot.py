"""Time the UAVMOT frame step (csrc/y7t_track_step.h: y7t_tracker_step_body_t<true>, the AMF pass included) on the GPU: per-frame update() latency
(launch + D2H of the returned rows), device-side step time with the detections resident in HBM (no host sync inside the loop: one launch per frame), the
same frames through y7t_tracker_step_frames (16 frames per launch, the index lists in LDS), and the size of the lost list at the end, at 80 and 500
objects over 300 frames.  With the reference sources present (build machine) it also reports the reference's CPU time per frame on the same scenes
(fewer frames at 500 objects: seconds per frame).  Reports numbers, gates nothing.

    python scripts/time_uavmot.py            # GPU + (if present) the reference
    python scripts/time_uavmot.py --cpu      # the reference only
"""
import os
import sys
import time
import types

import numpy as np  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolov7_tracker_amd import synth  # noqa: E402

SCENES = [(80, 300), (500, 300)]
GROUP = 16


def opts(**kw):
    o = types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="default", img_size=1280, iou_thresh=0.5)
    o.__dict__.update(kw)
    return o


def scene(nobj, nf):
    return synth.make_detections(nf, nobj, seq_idx=0, bounce=True)


def time_gpu():
    import torch
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.uavmot import UAVMOT
    for nobj, nf in SCENES:
        dets = scene(nobj, nf)
        ddev = [torch.from_numpy(d).cuda() for d in dets]
        for threads in (256, 512):
            BaseTrack._count = 0
            t = UAVMOT(opts(tracker_threads=threads))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for d in dets:
                t.update(d, None)
            torch.cuda.synchronize()
            lat = (time.perf_counter() - t0) / nf
            n_lost = len(t.lost_stracks)
            BaseTrack._count = 0
            t = UAVMOT(opts(tracker_threads=threads))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for d in ddev:
                t._launch(d)
            e1.record()
            torch.cuda.synchronize()
            step = e0.elapsed_time(e1) * 1e3 / nf
            BaseTrack._count = 0
            t = UAVMOT(opts(tracker_threads=threads))
            outs = [torch.zeros((t.cap_t + 1, 8), dtype=torch.float64, device="cuda") for _ in range(nf)]
            tables = [t.frames_table(ddev[f0:f0 + GROUP], outs[f0:f0 + GROUP]) for f0 in range(0, nf, GROUP)]
            torch.cuda.synchronize()
            e0.record()
            for tab in tables:
                t._launch_frames(tab)
            e1.record()
            torch.cuda.synchronize()
            frames = e0.elapsed_time(e1) * 1e3 / nf
            print("uavmot n_obj=%d frames=%d threads=%d  update() latency %.1f us/frame   device step %.1f us/frame   step_frames (%d per launch) %.1f us/frame"
                  "   lost list at the end %d" % (nobj, nf, threads, lat * 1e6, step, GROUP, frames, n_lost), flush=True)


def time_reference():
    from oracle import ref_harness
    if not ref_harness.available():
        print("reference sources not present: no CPU reference timing")
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("mg", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                                     "make_golden_uavmot.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mod = mg.load_uavmot()
    for nobj, nf in SCENES:
        nf = nf if nobj <= 100 else 10
        dets = scene(nobj, nf)
        next(c for c in mod.STrack.__mro__ if c.__name__ == "BaseTrack")._count = 0
        trk = mod.UAVMOT(ref_harness.make_opts(), frame_rate=30)
        t0 = time.perf_counter()
        for d in dets:
            trk.update(d, None)
        dt = (time.perf_counter() - t0) / nf
        print("reference (CPU) n_obj=%d frames=%d  %.2f ms/frame   lost list at the end %d" % (nobj, nf, dt * 1e3, len(trk.lost_stracks)))


if __name__ == "__main__":
    if "--cpu" not in sys.argv:
        time_gpu()
    time_reference()
