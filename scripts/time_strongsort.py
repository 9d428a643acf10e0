"""Time the StrongSORT frame (csrc/y7t_track_strongsort.h: k_ss_appearance, k_tracker_step_strongsort<MAXT>, k_ss_store) on the GPU, at 80 and 500 objects with
512-wide identity features, at 256 / 512 / 1024 threads: the median over 200 frames, after 40 warm-up frames, of
  * the whole frame on the device (an event pair around each frame's three launches; detections, features and warps resident in HBM, no host sync in the loop),
  * update() as a caller sees it (host clock: staging, the three launches, D2H of the rows and both status words),
and beside it the DeepSORT frame (k_ds_normalize + k_embed_dist + the step + k_ds_store) on the same scenes at the library's default thread count.
The three launches one by one come from a kernel trace of the same loop:

    python scripts/time_strongsort.py                                        # the table above
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/time_strongsort.py --trace-run --objs 500
    python scripts/time_strongsort.py --parse DIR                            # median us per launch of each kernel of that trace (warm-up frames dropped)
    python scripts/time_strongsort.py --cpu                                  # the reference's CPU time per frame on the same scenes (needs its sources)

Reports numbers, gates nothing."""
import argparse
import csv
import glob
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolov7_tracker_amd import synth  # noqa: E402

DIM, WARM, FRAMES = 512, 40, 200
THREADS = (256, 512, 1024)


def opts(**kw):
    o = types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="strongsort", img_size=1280, iou_thresh=0.5)
    o.__dict__.update(kw)
    return o


def scene(nobj, nf=WARM + FRAMES):
    """-> (dets, features of every row (zeros at or below conf_thresh), warps)"""
    dets, fn = synth.make_identity_features(nf, nobj, 1280, seq_idx=50, dim=DIM, miss=0.1, bounce=True)
    feats = []
    for d in dets:
        f = np.zeros((max(len(d), 1), DIM), np.float32)
        keep = d[:, 4] > np.float32(0.2)
        if keep.any():
            f[keep] = fn(d[keep, :4])
        feats.append(f)
    return dets, fn, feats, synth.make_warps(nf, seq_idx=50)


def median_us(events):
    return float(np.median([a.elapsed_time(b) for a, b in events])) * 1e3


def time_gpu(objs, trace_run=False):
    import torch
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.strongsort import StrongSORT
    from yolov7_tracker_amd.tracker.deepsort import DeepSORT
    for nobj in objs:
        dets, fn, feats, warps = scene(nobj)
        ddev = [torch.from_numpy(d).cuda() for d in dets]
        fdev = [torch.from_numpy(f).cuda() for f in feats]
        wdev = [torch.from_numpy(np.ascontiguousarray(w.reshape(6))).cuda() for w in warps]
        for threads in THREADS:
            BaseTrack._count = 0
            t = StrongSORT(opts(tracker_threads=threads), gamma=0.1)
            out = torch.zeros((t.cap_t + 1, 8), dtype=torch.float64, device="cuda")
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in dets]
            torch.cuda.synchronize()
            for i in range(len(dets)):
                ev[i][0].record()
                t._launch(ddev[i], fdev[i], warp=wdev[i], out=out)
                ev[i][1].record()
            torch.cuda.synchronize()
            assert t._status() == 0 and t._feature_status() == 0
            s = t._snapshot()
            line = "strongsort n_obj=%d dim=%d threads=%d  frame on the device %.1f us (median of %d)   tracked / lost at the end %d / %d" % (
                nobj, DIM, threads, median_us(ev[WARM:]), len(dets) - WARM, s["hdr_n_tracked"], s["hdr_n_lost"])
            if not trace_run:
                BaseTrack._count = 0
                t = StrongSORT(opts(tracker_threads=threads), gamma=0.1)
                t.get_feature = lambda tlbrs, ori_img: fn(tlbrs)
                lat = []
                for i, d in enumerate(dets):
                    t0 = time.perf_counter()
                    t.update(d, None, warp=warps[i])
                    lat.append(time.perf_counter() - t0)
                line += "   update() %.1f us (the feature lookup of the scene included)" % (1e6 * float(np.median(lat[WARM:])))
            print(line, flush=True)
        if trace_run:
            continue
        BaseTrack._count = 0
        t = DeepSORT(opts(kalman_format="default"))
        out = torch.zeros((t.cap_t + 1, 8), dtype=torch.float64, device="cuda")
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in dets]
        torch.cuda.synchronize()
        for i in range(len(dets)):
            ev[i][0].record()
            t._launch(ddev[i], fdev[i], out=out)
            ev[i][1].record()
        torch.cuda.synchronize()
        print("deepsort   n_obj=%d dim=%d threads=default  frame on the device %.1f us (median of %d)" % (nobj, DIM, median_us(ev[WARM:]), len(dets) - WARM), flush=True)


def parse_trace(folder):
    """median duration of every kernel of a rocprofv3 kernel trace whose name mentions the StrongSORT launches (the first WARM launches of each dropped)"""
    rows = {}
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"]
            if "k_ss_" in name or "strongsort" in name:
                rows.setdefault(name.split("(")[0], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for name, v in sorted(rows.items()):
        v.sort()
        runs = 1 if "k_tracker_step_strongsort" in name else len(THREADS)      # (a step instance serves one thread count, the other kernels all three, one after the other)
        per = max(1, len(v) // runs)
        d = []
        for k in range(0, len(v), per):      # (drop each run's warm-up)
            d += [b - a for a, b in v[k:k + per][WARM:]]
        print("%-60s %6d launches   median %.1f us" % (name, len(v), float(np.median(d)) / 1e3))


def time_reference(objs):
    from oracle import ref_harness
    if not ref_harness.available():
        print("reference sources not present: no CPU reference timing")
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("mg", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                                     "make_golden_strongsort.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mod = mg.load_strongsort()
    for nobj in objs:
        nf = WARM + FRAMES if nobj <= 100 else 60
        dets, fn, _, warps = scene(nobj, nf)
        times = []
        mg.run_reference(dets, fn, warps, 0.2, 0.1, "strongsort", mod=mod, timing=times)
        print("reference (CPU, features stubbed: tracker-only time) n_obj=%d dim=%d frames=%d  median %.2f ms/frame" % (nobj, DIM, nf, 1e3 * float(np.median(times[10:]))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--objs", type=int, nargs="+", default=[80, 500])
    ap.add_argument("--trace-run", action="store_true", help="only the device loop (for a run under rocprofv3 --kernel-trace)")
    ap.add_argument("--parse", metavar="DIR")
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    if a.parse:
        parse_trace(a.parse)
    elif a.cpu:
        time_reference(a.objs)
    else:
        time_gpu(a.objs, a.trace_run)
