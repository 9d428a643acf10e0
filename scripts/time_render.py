"""Annotated frames on the device: the time of the overlay (y7t_render_draw), of the JPEG encoder (y7t_jpeg_encode: its three launches) and of encode + the copy to
the host, per frame, at 1920 x 1080 and 1280 x 1280, with 80 and with 500 tracks a frame, in batches of 1 and of 8 -- and, in the same run, Pillow's encoder
(libjpeg) at the same quality and subsampling on one core of the host CPU, with the JPEG sizes of both.

    python scripts/time_render.py [--out profiles/render_timing.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_render.py --once      # one pass of every shape for a kernel trace; writes nothing
    python scripts/time_render.py --kernel-stats DIR                                     # append the per-kernel times of that trace to --out

Device times are HIP events around `reps` back-to-back calls after a warm-up of every shape (frames and track rows already on the device); encode + D2H is a host
clock around DeviceRenderer.encode, which ends in a synchronise.  The frames are synth's scenes resized by repetition: JPEG time and size depend on the content."""
import argparse
import csv
import glob
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1080, 1920), (1280, 1280)]


def frames_for(H, W, B):
    from yolov7_tracker_amd import synth
    base = synth.make_frames(B, 80, 640, seq_idx=1)
    return np.stack([np.tile(f, (H // f.shape[0] + 1, W // f.shape[1] + 1, 1))[:H, :W] for f in base]).astype(np.uint8)


def tracks_for(H, W, B, n, seed=0):
    rng = np.random.RandomState(seed)
    out = []
    for b in range(B):
        w, h = rng.uniform(20, 200, n), rng.uniform(30, 300, n)
        x, y = rng.uniform(-20, W - 20, n), rng.uniform(-20, H - 20, n)
        out.append([(x[i], y[i], w[i], h[i], i + 1, b"%d-%d" % (i % 10, i + 1)) for i in range(n)])
    return out


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


def kernel_stats(directory):
    """the four kernels' lines out of a trace: every dispatch from the SQLite file newer rocprofv3 versions write (view `kernels`), or the averages of a stats csv"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        db = sqlite3.connect(path)
        for name, gx, gy, gz, wx, ns in db.execute("select name, grid_x, grid_y, grid_z, workgroup_x, duration from kernels order by start"):
            short = name.split("(")[0]
            if short in ("k_render_draw", "k_jpeg_blocks", "k_jpeg_entropy", "k_jpeg_pack"):
                rows.append("  %-16s %6d x %4d x %d workgroups of %3d  %9.1f us" % (short, gx // wx, gy, gz, wx, ns / 1e3))
    if rows:
        return rows
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if r["Name"].split("(")[0] in ("k_render_draw", "k_jpeg_blocks", "k_jpeg_entropy", "k_jpeg_pack"):
                rows.append("  %-16s calls %5s  average %10.1f us  min %10.1f us  max %10.1f us" % (r["Name"].split("(")[0], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                                                  float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_timing.txt"))
    ap.add_argument("--once", action="store_true", help="one call of every shape at batch 8 with 80 tracks, for a kernel trace")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 --kernel-trace --stats output directory of a --once run: append its per-kernel lines to --out")
    ap.add_argument("--reps", type=int, default=20)
    o = ap.parse_args()
    if o.kernel_stats:
        rows = kernel_stats(o.kernel_stats)
        with open(o.out, "a") as fh:
            fh.write("\nper dispatch, from a kernel trace (a run of its own) of one pass at batch 8 with 80 tracks a frame: 1920 x 1080 at 4:2:0, at 4:4:4, then 1280 x 1280 at 4:2:0, at 4:4:4:\n"
                     + ("\n".join(rows) if rows else "  not measured: the trace holds none of the kernels") + "\n")
        return
    import torch
    from PIL import Image
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker.render import DeviceRenderer, pack_tracks
    _lib.require_gpu()
    L = _lib.load()
    lines = ["annotated frames on one MI355X (%s): device times are HIP events over %d back-to-back calls after a warm-up; ms per FRAME" % (torch.cuda.get_device_name(0), o.reps),
             "encode = y7t_jpeg_encode (k_jpeg_blocks, k_jpeg_entropy, k_jpeg_pack), quality 95; encode + D2H = DeviceRenderer.encode on a host clock (it ends in a synchronise)",
             "Pillow = Image.save(JPEG, quality=95, the same subsampling) of the same annotated frame on one host core, in the same run", ""]
    for H, W in SHAPES:
        for sub in ("420", "444"):
            for B in ((8,) if o.once else (1, 8)):
                frames = torch.from_numpy(frames_for(H, W, B)).cuda()
                r = DeviceRenderer(H, W, quality=95, subsampling=sub, max_batch=B)
                for n in ((80,) if o.once else (80, 500)):
                    tracks = tracks_for(H, W, B, n)
                    rows, offsets = pack_tracks(tracks)
                    d_rows, d_off = torch.from_numpy(rows.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(offsets).cuda()
                    out = torch.empty_like(frames)

                    def draw():
                        _lib.check(L.y7t_render_draw(_lib.ptr(frames), B, H, W, _lib.ptr(d_rows), _lib.ptr(d_off), _lib.ptr(out), _lib.stream_ptr()))

                    def encode():
                        _lib.check(L.y7t_jpeg_encode(_lib.ptr(r._obj), _lib.ptr(out), B, _lib.ptr(r._out), r._out_bytes, _lib.ptr(r._lens), _lib.stream_ptr()))

                    if o.once:
                        draw(); encode(); torch.cuda.synchronize()
                        continue
                    t_draw, t_enc = device_ms(draw, o.reps) / B, device_ms(encode, o.reps) / B
                    files = r.encode(out)
                    t0 = time.perf_counter()
                    for _ in range(o.reps):
                        r.encode(out)
                    t_d2h = (time.perf_counter() - t0) / o.reps / B * 1e3
                    host = out.cpu().numpy()
                    t0 = time.perf_counter()
                    sizes = []
                    for b in range(B):
                        f = io.BytesIO()
                        Image.fromarray(np.ascontiguousarray(host[b][..., ::-1])).save(f, "JPEG", quality=95, subsampling={"420": 2, "444": 0}[sub])
                        sizes.append(f.tell())
                    t_pil = (time.perf_counter() - t0) / B * 1e3
                    lines.append("%4d x %-4d %s batch %d, %3d tracks: draw %7.3f  encode %7.3f  encode + D2H %7.3f  | Pillow %7.2f   | bytes a frame: ours %8d  Pillow %8d"
                                 % (W, H, sub, B, n, t_draw, t_enc, t_d2h, t_pil, sum(len(f) for f in files) // B, sum(sizes) // B))
                    print(lines[-1], flush=True)
                del r
    if not o.once:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        open(o.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
