"""Time the C-BIoU frame step (csrc/y7t_track_cbiou.h) on the GPU: per-frame update() latency (launch + D2H of the returned rows), device-side step time
with the detections resident in HBM (no host sync inside the loop), and the size of the lost list at the end, at 80 and 500 objects over 300 frames.
With the reference sources present (build machine) it also reports the reference's CPU time per frame on the same scenes.  Reports numbers, gates nothing.

    python scripts/time_c_biou.py            # GPU + (if present) the reference
    python scripts/time_c_biou.py --cpu      # the reference only
"""
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolov7_tracker_amd import synth  # noqa: E402

SCENES = [(80, 300), (500, 300)]


def opts(**kw):
    o = types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="default", img_size=1280, iou_thresh=0.5)
    o.__dict__.update(kw)
    return o


def scene(nobj, nf):
    return synth.make_detections(nf, nobj, seq_idx=0, bounce=True)


def time_gpu():
    import torch
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.c_biou_tracker import C_BIoUTracker
    for nobj, nf in SCENES:
        dets = scene(nobj, nf)
        ddev = [torch.from_numpy(d).cuda() for d in dets]
        for threads in (256, 512):
            BaseTrack._count = 0
            t = C_BIoUTracker(opts(tracker_threads=threads))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for d in dets:
                t.update(d, None)
            torch.cuda.synchronize()
            lat = (time.perf_counter() - t0) / nf
            n_lost = len(t.lost_stracks)
            BaseTrack._count = 0
            t = C_BIoUTracker(opts(tracker_threads=threads))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for d in ddev:
                t._launch(d)
            e1.record()
            torch.cuda.synchronize()
            print("c_biou n_obj=%d frames=%d threads=%d  update() latency %.1f us/frame   device step %.1f us/frame   lost list at the end %d"
                  % (nobj, nf, threads, lat * 1e6, e0.elapsed_time(e1) * 1e3 / nf, n_lost))


def time_reference():
    from oracle import ref_harness
    if not ref_harness.available():
        print("reference sources not present: no CPU reference timing")
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("mg", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                                     "make_golden_c_biou.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mod = mg.load_c_biou()
    for nobj, nf in SCENES:
        dets = scene(nobj, nf)
        mod.BaseTrack._count = 0
        trk = mod.C_BIoUTracker(ref_harness.make_opts(), frame_rate=30)
        t0 = time.perf_counter()
        for d in dets:
            trk.update(d, None)
        dt = (time.perf_counter() - t0) / nf
        print("reference (CPU) n_obj=%d frames=%d  %.2f ms/frame   lost list at the end %d" % (nobj, nf, dt * 1e3, len(trk.lost_stracks)))


if __name__ == "__main__":
    if "--cpu" not in sys.argv:
        time_gpu()
    time_reference()
