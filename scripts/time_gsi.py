"""GSI on the device: the device time of the interpolation and of the smoother on one synthetic sequence -- 300 objects of synth's scene generator over 600 frames
with its 10 % misses, so the tracks have the length mix of synth's scenes (objects drift out of the image) -- and of the smoother on single tracks of 64, 256,
1024 and 4096 rows; and, in the same run, the NumPy + LAPACK restatement (tests/gsi_np.py) on the host CPU, and scikit-learn's GaussianProcessRegressor where it
can be imported.

    python scripts/time_gsi.py [--out profiles/gsi_timing.txt]

Device times are HIP events around `reps` back-to-back calls after a warm-up of every shape (tables already on the device).  One workgroup takes one track, so
the single-track lines show one compute unit's time for a system of that size; the FLOP rate quoted is n^3 / 3 over the whole call."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sequence(n_frames=600, n_obj=300, seed=0):
    from yolov7_tracker_amd import synth
    rng = np.random.RandomState(seed)
    rows = []
    for f, gt in enumerate(synth.make_ground_truth(n_frames, n_obj, 1280, 0)):
        gt = gt[gt[:, 6] > 0]
        rows.append(np.column_stack([np.full(len(gt), f + 1.0), gt[:, 0], gt[:, 1:5] + rng.normal(0, 1.5, (len(gt), 4)), gt[:, 5]]))
    return np.concatenate(rows, 0)


def single(n, seed=0):
    rng = np.random.RandomState(seed)
    f = np.arange(1, n + 1, dtype=np.float64)
    box = np.column_stack([300 + 1.1 * f + 20 * np.sin(f / 23), 200 - 0.4 * f, 40 + 0 * f, 90 + 0 * f]) + rng.normal(0, 1.5, (n, 4))
    return np.column_stack([f, box]), np.array([0, n], np.int32)


def device_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gsi_timing.txt"))
    ap.add_argument("--tau", type=float, default=10)
    o = ap.parse_args()
    import torch
    from tests import gsi_np
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker import gsi
    L = _lib.load()
    st = _lib.stream_ptr()
    lines = ["GSI timing: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), ""]

    def smooth_call(model, runs, off, ls, longest):
        t, oo, l = torch.from_numpy(runs).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(ls, np.float64)).cuda()
        cols = torch.zeros((len(runs), 4), dtype=torch.float64, device="cuda")
        status = torch.zeros(len(off) - 1, dtype=torch.int32, device="cuda")
        fn = lambda: _lib.check(L.y7t_gsi_smooth(model.ptr, t.data_ptr(), oo.data_ptr(), l.data_ptr(), len(off) - 1, int(longest), 1e-10, cols.data_ptr(), status.data_ptr(), st))
        return fn, cols, status

    # ---- the sequence ----
    rows = sequence()
    rows_o, ids, off_in = gsi.order_rows(rows)
    runs_in = np.ascontiguousarray(rows_o[:, [0, 2, 3, 4, 5]])
    n_after = gsi.lengths_after(runs_in[:, 0], off_in, 20)
    model = gsi.DeviceGSI(len(ids), int(n_after.sum()), int(n_after.max()))
    res = model.interpolate(runs_in, off_in, 20)
    assert res["status"] == 0 and np.array_equal(np.diff(res["offsets"]), n_after)
    ls = gsi.length_scales(n_after, o.tau)
    t_in, o_in = torch.from_numpy(runs_in).cuda(), torch.from_numpy(off_in).cuda()
    off2 = torch.zeros(len(ids) + 1, dtype=torch.int32, device="cuda")
    interp = lambda: _lib.check(L.y7t_gsi_interpolate(model.ptr, t_in.data_ptr(), o_in.data_ptr(), len(ids), 20, model._runs.data_ptr(), off2.data_ptr(), model._src.data_ptr(),
                                                      model._head.data_ptr(), model._head.data_ptr() + 4, st))
    ms_i = device_ms(interp, 20)
    fn, cols, status = smooth_call(model, res["runs"], res["offsets"], ls, n_after.max())
    ms_s = device_ms(fn, 5)
    assert not status.cpu().numpy().any()
    q = np.percentile(n_after, [0, 25, 50, 75, 100]).astype(int)
    lines += ["sequence: %d tracks, %d rows -> %d rows after interpolation; track lengths min / quartiles / max %s; %d tracks beyond 128 rows (HBM pool)"
              % (len(ids), len(runs_in), int(n_after.sum()), " ".join(map(str, q)), int((n_after > 128).sum())),
              "  device interpolation (3 launches)          %9.3f ms" % ms_i,
              "  device smoother (all tracks)               %9.3f ms" % ms_s]
    t0 = time.perf_counter()
    want = gsi_np.smooth(res["runs"], res["offsets"], o.tau)
    cpu_s = time.perf_counter() - t0
    assert np.abs(cols.cpu().numpy() - want).max() < 1e-3      # (two float64 orders: 1e-4 at these lengths)
    lines += ["  NumPy + LAPACK float64 on the host CPU      %9.3f ms   (%.1f x the device smoother)" % (cpu_s * 1e3, cpu_s * 1e3 / ms_s),
              "  largest |device - NumPy| over the sequence  %9.3g px" % float(np.abs(cols.cpu().numpy() - want).max())]
    t0 = time.perf_counter()
    gsi_np.interpolate(runs_in, off_in, 20)
    lines += ["  NumPy interpolation (a Python loop)         %9.3f ms" % ((time.perf_counter() - t0) * 1e3)]
    try:
        from sklearn.gaussian_process import GaussianProcessRegressor as GPR
        from sklearn.gaussian_process.kernels import RBF
        t0 = time.perf_counter()
        for k in range(len(ids)):
            lo, hi = int(res["offsets"][k]), int(res["offsets"][k + 1])
            t = res["runs"][lo:hi, :1]
            for c in range(4):
                GPR(RBF(float(ls[k]), "fixed")).fit(t, res["runs"][lo:hi, 1 + c:2 + c]).predict(t)
        lines += ["  scikit-learn, one fit per track and column  %9.3f ms" % ((time.perf_counter() - t0) * 1e3)]
    except ImportError:
        lines += ["  scikit-learn: not installed here"]
    lines += [""]

    # ---- single tracks: one workgroup, one compute unit ----
    lines += ["single tracks (one workgroup each):  rows   len_scale   device ms   GFLOP/s (n^3/3)   NumPy+LAPACK ms   |device - NumPy| px"]
    for n in (64, 256, 1024, 4096):
        runs, off = single(n)
        m1 = gsi.DeviceGSI(1, n, n)
        l1 = gsi.length_scales([n], o.tau)
        fn, cols, status = smooth_call(m1, runs, off, l1, n)
        ms = device_ms(fn, 3 if n >= 1024 else 20)
        assert not status.cpu().numpy().any()
        t0 = time.perf_counter()
        want = gsi_np.smooth_track(runs[:, 0], runs[:, 1:], float(l1[0]))
        cpu = (time.perf_counter() - t0) * 1e3
        lines += ["                                    %5d   %9.4g   %9.3f   %15.2f   %15.3f   %9.3g" % (n, l1[0], ms, n ** 3 / 3 / (ms * 1e-3) / 1e9, cpu,
                                                                                                             float(np.abs(cols.cpu().numpy() - want).max()))]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(o.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
