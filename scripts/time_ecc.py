"""Time the camera-motion estimate (csrc/y7t_ecc.hip: k_ecc_prepare, k_ecc_iter) on the GPU at 1920x1080 and 1280x1280 source frames, downscale 2: the median
over 30 repetitions, after 5 warm-up ones, of an event pair around
  * the prepare launch (uint8 BGR frame resident in HBM -> the half-resolution {I, gx, gy} plane),
  * one Gauss-Newton iteration: (align with 21 fixed iterations - align with 1) / 20, eps < 0,
  * a whole estimate with the reference's criteria (100 iterations, eps 1e-5): every launch of y7t_ecc_align, the finished ones included,
  * GMC.apply as a caller sees it (host clock: H2D of the frame, prepare, align, D2H of the matrix),
and beside it the NumPy float64 restatement (tests/ecc_np.py) on the CPU for the same frames (host clock, one run).  The frames are the analytic scene of
synth.camera_background and its copy under a planted warp of 0.002 rad, (3, -2) px.

    python scripts/time_ecc.py            # the table
    python scripts/time_ecc.py --no-cpu   # without the CPU column

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
SIZES = ((1080, 1920), (1280, 1280))


def scene(size):
    f0 = synth.render_camera_frame(size, synth.euclidean_warp(0.0, 0.0, 0.0), 9)
    inv = np.linalg.inv(np.vstack([synth.euclidean_warp(0.002, 3.0, -2.0), [0.0, 0.0, 1.0]]))[:2]
    return f0, synth.render_camera_frame(size, inv, 9)


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
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker.gmc import GMC
    _lib.require_gpu()
    L = _lib.load()
    for size in SIZES:
        H, W = size
        h, w = H // 2, W // 2
        f0, f1 = scene(size)
        d0, d1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
        p0, p1 = (torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        nb = ctypes.c_size_t()
        _lib.check(L.y7t_ecc_workspace_bytes(h, w, ctypes.byref(nb)))
        ws = torch.empty(nb.value // 8 + 1, dtype=torch.float64, device="cuda")
        out = torch.empty(10, dtype=torch.float64, device="cuda")

        def prepare(src=d1, dst=p1):
            _lib.check(L.y7t_ecc_prepare_u8(_lib.ptr(src), H, W, 2, _lib.ptr(dst), _lib.stream_ptr()))

        def align(k=100, eps=1e-5):
            _lib.check(L.y7t_ecc_align(_lib.ptr(p0), _lib.ptr(p1), h, w, 1, k, eps, _lib.ptr(ws), _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + 48), _lib.stream_ptr()))

        prepare(d0, p0)
        t_prep = median_us(prepare, torch)
        t1, t21 = median_us(lambda: align(1, -1.0), torch), median_us(lambda: align(21, -1.0), torch)
        t_all = median_us(align, torch)
        st = out.cpu().numpy()
        g = GMC('ecc')
        g.apply(f0)
        host = []
        for i in range(WARM + REPS):
            t = time.perf_counter()
            g.apply(f1)
            host.append(time.perf_counter() - t)
        print("%dx%d -> plane %dx%d: prepare %.1f us, one iteration %.1f us, whole estimate %.1f us (%d iterations, flag %d, rho %.6f, %d launches), "
              "GMC.apply from a host frame %.1f us" % (W, H, w, h, t_prep, (t21 - t1) / 20.0, t_all, st[6], st[7], st[8], 103, np.median(host[WARM:]) * 1e6), flush=True)
        if not args.no_cpu:
            from tests import ecc_np
            t = time.perf_counter()
            P0, P1 = ecc_np.prepare(f0), ecc_np.prepare(f1)
            tp = time.perf_counter() - t
            t = time.perf_counter()
            r = ecc_np.align(P0[..., 0], P1)
            ta = time.perf_counter() - t
            print("    NumPy float64 restatement on the CPU: prepare %.1f ms per frame, estimate %.1f ms (%d iterations = %.1f ms each); parameters differ from the device's by %.2g"
                  % (tp / 2 * 1e3, ta * 1e3, r[1], ta / r[1] * 1e3, np.abs(np.array([np.arctan2(st[3], st[0]), st[2], st[5]]) - r[5]).max()), flush=True)


if __name__ == "__main__":
    main()
