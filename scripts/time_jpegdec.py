"""Time the device JPEG decoder (tracker/jpeg_decode.py, csrc/y7t_jpegdec.hip) against what it replaces -> profiles/jpegdec_timing.txt.

    python scripts/time_jpegdec.py [--out profiles/jpegdec_timing.txt] [--reps 10]

1920 x 1080, 4:2:0, quality 75 and 95, with and without restart markers, batch 1 / 8 / 80: the device decode alone (files resident), decode + H2D of the files'
bytes, H2D of the raw frames (today's path after the host decode), Pillow's decode on one host core in the same run; the time per subsequence length at quality
95, from which the default is chosen; and the synchronisation launches real streams needed.  Medians of `reps` timed calls after 2 warm-up calls, device events."""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(h, w, seed):
    """a frame with structure at every scale: smooth gradients, blocks, edges and some noise (a synthetic stand-in for a street scene)"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([128 + 100 * np.sin(x / 97 + c) * np.cos(y / 61 - c) for c in range(3)], -1)
    small = rng.randint(0, 256, (h // 24 + 1, w // 24 + 1, 3)).astype(np.float32)
    img = 0.6 * img + 0.4 * np.kron(small, np.ones((24, 24, 1), np.float32))[:h, :w]
    img += rng.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def median_ms(fn, reps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegdec_timing.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 80])
    opts = ap.parse_args()
    import torch
    from PIL import Image
    from yolov7_tracker_amd.tracker import jpeg_decode
    H, W = 1080, 1920
    lines = ["JPEG decode on the device, %d x %d, 4:2:0 (scripts/time_jpegdec.py; medians of %d calls; us per frame)" % (W, H, opts.reps), ""]
    frames = [scene(H, W, s) for s in range(8)]

    def files_for(quality, restart, n):
        out = []
        for f in frames:
            b = io.BytesIO()
            Image.fromarray(f).save(b, "JPEG", quality=quality, subsampling=2, **({"restart_marker_blocks": restart} if restart else {}))
            out.append(b.getvalue())
        return [out[i % len(out)] for i in range(n)]

    def pillow_ms(files):
        t = time.perf_counter()
        for f in files[:8]:
            np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        return (time.perf_counter() - t) * 1e3 / min(len(files), 8)

    lines.append("%-28s %6s %10s %12s %12s %12s %10s %8s" % ("case", "batch", "bytes/file", "decode", "decode+H2D", "H2D raw", "Pillow", "launches"))
    for quality in (75, 95):
        for restart in (0, 120):
            for B in opts.batches:
                files = files_for(quality, restart, B)
                dec = jpeg_decode.DeviceJpegDecoder(H, W, 3, "420", max_batch=B, max_file_bytes=max(len(f) for f in files))
                dev, descs = dec.upload(files)
                out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
                t_dec = median_ms(lambda: dec.decode_uploaded(dev, descs, out=out), opts.reps)

                def both():
                    d, ds = dec.upload(files)
                    dec.decode_uploaded(d, ds, out=out)
                t_both = median_ms(both, opts.reps)
                raw = torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory()
                t_raw = median_ms(lambda: out.copy_(raw, non_blocking=True), opts.reps)
                rounds = int(dec.rounds(B).max())
                lines.append("%-28s %6d %10d %9.1f us %9.1f us %9.1f us %7.2f ms %8d" % (
                    "q%d %s" % (quality, "restart every %d MCUs" % restart if restart else "no restart markers"), B, int(np.mean([len(f) for f in files])),
                    1e3 * t_dec / B, 1e3 * t_both / B, 1e3 * t_raw / B, pillow_ms(files), rounds))
                del dec, dev, out, raw
    lines += ["", "(decode+H2D includes writing the files into the pinned buffer on the host; launches: the last synchronisation launch that found work, plus one)", "",
              "subsequence length, quality 95, no restart markers, batch 8 (decode alone, us per frame):"]
    files = files_for(95, 0, 8)
    best = None
    for S in (32, 64, 128, 256, 512):
        dec = jpeg_decode.DeviceJpegDecoder(H, W, 3, "420", max_batch=8, max_file_bytes=max(len(f) for f in files), subseq_bytes=S)
        dev, descs = dec.upload(files)
        out = torch.empty((8, H, W, 3), dtype=torch.uint8, device="cuda")
        t = 1e3 * median_ms(lambda: dec.decode_uploaded(dev, descs, out=out), opts.reps) / 8
        lines.append("  subseq_bytes %4d: %8.1f us   launches that found work %d of %d" % (S, t, int(dec.rounds(8).max()), -(-(-(-max(int(d["scan_len"]) for d in descs) // S)) // 256)))
        best = (t, S) if best is None or t < best[0] else best
        del dec, dev, out
    lines.append("  fastest: subseq_bytes %d (the library's default is %d)" % (best[1], jpeg_decode.SUBSEQ_DEFAULT))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(opts.out), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
