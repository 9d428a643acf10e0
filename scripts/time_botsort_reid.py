"""Time the frame of BoT-SORT with its appearance branch (csrc/y7t_track_botsort_reid.h: k_br_prepare, k_tracker_step_botsort_reid<MAXT>, k_br_store) on the GPU at
80 objects / dim 128, 500 objects / dim 128 and 500 objects / dim 512, and the state-path BoT-SORT step (k_tracker_step<PLAIN>) on the same scenes from the same
build, alternating the two trackers frame by frame in one loop: the median over 200 frames, after 40 warm-up frames, of an event pair around each frame's launches
(detections, features and warps resident in HBM, no host sync in the loop), at the library's default thread count and at 512 threads.  Beside the added time it
prints the frame's count of cosines (the pairs at or under theta_iou: the feature state's counter) and tracks x detections, so that a reader sees what the
added time follows; and the reference's CPU milliseconds per frame recorded in the goldens (tests/golden/tracker_botsort_reid_*.npz: other, smaller scenes).

    python scripts/time_botsort_reid.py > profiles/botsort_reid_timing.txt
    python scripts/time_botsort_reid.py --cpu          # the reference's CPU time per frame on these scenes (needs its sources)

Reports numbers, gates nothing."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolov7_tracker_amd import synth  # noqa: E402

WARM, FRAMES = 40, 200
CASES = [(80, 128), (500, 128), (500, 512)]


def opts(**kw):
    o = types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="botsort", img_size=1280, iou_thresh=0.5)
    o.__dict__.update(kw)
    return o


def scene(nobj, dim, nf=WARM + FRAMES):
    """-> (dets, feature function, features of every row (zeros below conf_thresh), warps)"""
    dets, fn = synth.make_identity_features(nf, nobj, 1280, seq_idx=50, dim=dim, miss=0.1, bounce=True)
    feats = []
    for d in dets:
        f = np.zeros((max(len(d), 1), dim), np.float32)
        keep = d[:, 4] >= np.float32(0.2)
        if keep.any():
            f[keep] = fn(d[keep, :4])
        feats.append(f)
    return dets, fn, feats, synth.make_warps(nf, seq_idx=50)


def time_gpu(cases):
    import torch
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.botsort import BoTSORT
    print("# frames: %d timed after %d warm-up; times are medians of per-frame device event pairs, the two trackers alternate frame by frame in one loop" % (FRAMES, WARM))
    for nobj, dim in cases:
        dets, fn, feats, warps = scene(nobj, dim)
        ddev = [torch.from_numpy(d).cuda() for d in dets]
        fdev = [torch.from_numpy(f).cuda() for f in feats]
        wdev = [torch.from_numpy(np.ascontiguousarray(w.reshape(6))).cuda() for w in warps]
        for threads in (0, 512):
            BaseTrack._count = 0
            a = BoTSORT(opts(tracker_threads=threads), use_apperance_model=True)
            b = BoTSORT(opts(tracker_threads=threads))
            out = torch.zeros((a.cap_t + 1, 8), dtype=torch.float64, device="cuda")
            mk = lambda: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in dets]      # noqa: E731
            ea, eb = mk(), mk()
            counts = torch.zeros((len(dets), 16), dtype=torch.int32, device="cuda")
            pools = torch.zeros((len(dets), 2), dtype=torch.int32, device="cuda")
            off = a._layout["hdr_n_tracked"]
            torch.cuda.synchronize()
            for i in range(len(dets)):
                pools[i].copy_(a._state[off:off + 8].view(torch.int32))      # tracked / lost before the frame (device-side copies: nothing is read back in the loop)
                ea[i][0].record()
                a._launch(ddev[i], fdev[i], warp=wdev[i], out=out)
                ea[i][1].record()
                counts[i].copy_(a._feat[:64].view(torch.int32))
                eb[i][0].record()
                b._launch(ddev[i], warp=wdev[i], out=out)
                eb[i][1].record()
            torch.cuda.synchronize()
            assert a._status() == 0 and a._feature_status() == 0 and b._status() == 0
            ta = np.array([x.elapsed_time(y) for x, y in ea[WARM:]]) * 1e3
            tb = np.array([x.elapsed_time(y) for x, y in eb[WARM:]]) * 1e3
            c, p = counts.cpu().numpy()[WARM:], pools.cpu().numpy()[WARM:]
            nd = np.array([len(d) for d in dets[WARM:]])
            dense = (p.sum(1) * nd).astype(np.float64)
            print("n_obj=%d dim=%d threads=%s   with the appearance branch %.1f us   state path %.1f us   added %.1f us   cosines per frame median %d (min %d, max %d)   "
                  "tracks x detections median %d   added us per cosine %.3f   pairs gated by theta_emb per frame median %d" % (
                      nobj, dim, threads or "default", np.median(ta), np.median(tb), np.median(ta) - np.median(tb), np.median(c[:, 7]), c[:, 7].min(), c[:, 7].max(),
                      np.median(dense), (np.median(ta) - np.median(tb)) / max(np.median(c[:, 7]), 1), np.median(c[:, 12])), flush=True)
            # does the added time follow the cosines? the quarter of the frames with the fewest against the quarter with the most
            order = np.argsort(c[:, 7], kind="stable")
            q = max(len(order) // 4, 1)
            lo, hi = order[:q], order[-q:]
            print("    frames with the fewest cosines (median %d): added %.1f us;   with the most (median %d): added %.1f us" % (
                np.median(c[lo, 7]), np.median(ta[lo] - tb[lo]), np.median(c[hi, 7]), np.median(ta[hi] - tb[hi])), flush=True)
    print("# the reference on the CPU (tracker only, features stubbed), ms per frame, as recorded in tests/golden/tracker_botsort_reid_<name>.npz:")
    gold = os.path.join(ROOT, "tests", "golden")
    for f in sorted(os.listdir(gold)):
        if f.startswith("tracker_botsort_reid_") and f.endswith(".npz"):
            g = np.load(os.path.join(gold, f))
            print("#   %-14s %3d objects dim %3d: %.2f ms" % (f[21:-4], int(g["scene"][1]), int(g["feat_dim"]), float(g["ref_ms_per_frame"])))


def time_reference(cases):
    from oracle import ref_harness
    if not ref_harness.available():
        print("reference sources not present: no CPU reference timing")
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("mg", os.path.join(ROOT, "tests", "golden", "make_golden_botsort_reid.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    for nobj, dim in cases:
        nf = WARM + FRAMES if nobj <= 100 else 40
        dets, fn, _, warps = scene(nobj, dim, nf)
        times = []
        mg.run_reference(dets, fn, warps, 0.2, timing=times)
        print("reference (CPU, features stubbed: tracker-only time) n_obj=%d dim=%d frames=%d  median %.2f ms/frame" % (nobj, dim, nf, 1e3 * float(np.median(times[10:]))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    if a.cpu:
        time_reference(CASES)
    else:
        time_gpu(CASES)
