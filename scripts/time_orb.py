"""Time the feature-based camera-motion estimate (csrc/y7t_orb.hip) on the GPU at 1920x1080 source frames, downscale 2, max_keypoints 8192, with 0 and with 500
detection boxes masked out: the median over 30 repetitions, after 5 warm-up ones, of an event pair around
  * y7t_orb_extract_u8 (seven launches: uint8 BGR frame resident in HBM -> keypoints and descriptors),
  * y7t_orb_estimate (four launches: matching, filters, 2000 hypotheses, select + refine),
  * both, which is what a frame costs,
  * GMC.apply as a caller sees it (host clock: H2D of the frame, extract, estimate, D2H of the matrix),
then, with --stages, every kernel on its own from one torch.profiler trace of 10 frames (mean device time per launch), and the keypoint / match / inlier
counts of the scene.  The frames are synth.make_corner_frames under a planted warp of 0.002 rad, (3, -2) px.  Beside it: the ECC estimate of scripts/time_ecc.py
on the same machine is 298 us at this size (profiles/ecc_timing.txt).

    python scripts/time_orb.py --stages | tee profiles/orb_timing.txt

Reports numbers, gates nothing."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolov7_tracker_amd import synth  # noqa: E402

WARM, REPS = 5, 30
SIZE, DS, CAP = (1080, 1920), 2, 8192


def median_us(fn, torch):
    ev = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev[WARM:]])) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", action="store_true", help="per-kernel device times from a torch.profiler trace")
    args = ap.parse_args()
    import torch
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker.gmc import GMC
    _lib.require_gpu()
    L = _lib.load()
    H, W = SIZE
    h, w = H // DS, W // DS
    frames, _ = synth.make_corner_frames(2, SIZE, 9, steps=[(0.002, 3.0, -2.0)])
    d0, d1 = torch.from_numpy(frames[0]).cuda(), torch.from_numpy(frames[1]).cuda()
    nb = ctypes.c_size_t()
    _lib.check(L.y7t_orb_workspace_bytes(h, w, CAP, ctypes.byref(nb)))
    ws = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_orb_state_bytes(CAP, ctypes.byref(nb)))
    s0, s1 = (torch.empty(nb.value, dtype=torch.uint8, device="cuda") for _ in range(2))
    out = torch.empty(12, dtype=torch.float64, device="cuda")
    for n_dets in (0, 500):
        dets_np = synth.make_detections(1, 600, W, seq_idx=9)[0][:n_dets] if n_dets else None
        if dets_np is not None:
            dets_np[:, [1, 3]] *= H / W
            assert len(dets_np) == n_dets
        dets = torch.from_numpy(dets_np).cuda() if n_dets else None

        def extract(src=d1, dst=s1):
            _lib.check(L.y7t_orb_extract_u8(_lib.ptr(src), H, W, DS, _lib.ptr(dets) if n_dets else None, n_dets, CAP, _lib.ptr(ws), _lib.ptr(dst), _lib.stream_ptr()))

        def estimate():
            _lib.check(L.y7t_orb_estimate(_lib.ptr(s0), _lib.ptr(s1), h, w, DS, CAP, _lib.ptr(ws), _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + 48), _lib.stream_ptr()))

        def both():
            extract()
            estimate()

        extract(d0, s0)
        t_ext, t_est, t_both = median_us(extract, torch), median_us(estimate, torch), median_us(both, torch)
        st = out.cpu().numpy()
        g = GMC('features')
        g.apply(frames[0], dets_np)
        host = []
        for i in range(WARM + REPS):      # (alternating frames: a frame against itself has zero deviation, and the one-sided test then passes nothing)
            t = time.perf_counter()
            g.apply(frames[(i + 1) & 1], dets_np)
            host.append(time.perf_counter() - t)
        print("%dx%d -> plane %dx%d, %d detections: extract %.1f us, estimate %.1f us, a frame (both) %.1f us; GMC.apply from a host frame %.1f us; "
              "%d / %d keypoints, %d good matches, %d inliers, flag %d, truncated %d; warp %s"
              % (W, H, w, h, n_dets, t_ext, t_est, t_both, np.median(host[WARM:]) * 1e6, st[6], st[7], st[8], st[9], st[10], st[11], np.round(st[:6], 5).tolist()), flush=True)
        if args.stages:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for i in range(10):
                    both()
                torch.cuda.synchronize()
            rows = [(e.key, e.count, (getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) / max(e.count, 1))
                    for e in prof.key_averages() if "k_orb" in e.key]
            for key, count, us in sorted(rows):
                print("    %-60s %3d launches, %8.1f us each" % (key[:60], count, us), flush=True)
            print("    sum of the kernels of a frame: %.1f us" % sum(us * count / 10.0 for _, count, us in rows), flush=True)


if __name__ == "__main__":
    main()
