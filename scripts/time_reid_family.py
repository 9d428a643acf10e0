"""Time the OSNet family's embedding paths on the device: microseconds per crop of the general fp16 path (ReIDExtractor(half=True)), of the fp32 op list on the
same crops in the same run (the baseline), and -- for osnet_x0_25 at 128 x 64 -- of the fused kernel.

    python scripts/time_reid_family.py [--out profiles/osnet_family_timing.txt] [--window 0.3] [--repeats 3] [--nets osnet_x0_25,...]

Method: crops are boxes of one seeded 1280 x 1280 frame (the crop sampler is part of every path); per configuration every path is warmed up with two calls, then
the paths ALTERNATE `repeats` times, each turn issuing calls back to back for at least `window` seconds (at least 3 calls) between two device synchronisations
(host clock).  Reported: the median turn, and the fastest and slowest turn as the spread.  The arena holds at most 128 crops (what the trackers configure), so 500
crops are four calls into the library per embedding call -- as in a tracker run."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolov7_tracker_amd import synth  # noqa: E402
from yolov7_tracker_amd.tracker import reid  # noqa: E402

SIZES = [(128, 64), (256, 128), (128, 256)]       # H x W: DeepSORT / BoT-SORT, torchreid's, StrongSORT's
COUNTS = [80, 500]


def turn(ex, frame, boxes, window):
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while calls < 3 or time.perf_counter() - t0 < window:
        ex.features_for_boxes(frame, boxes)
        calls += 1
        if calls >= 3 and calls % 4 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nets", default=",".join(reid.OSNET_NAMES))
    ap.add_argument("--max_crops", type=int, default=128)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    frame = torch.from_numpy(synth.make_frames(1, 40, 1280, seq_idx=1)[0]).cuda()
    H, W = int(frame.shape[0]), int(frame.shape[1])
    rng = np.random.default_rng(0)
    xy = rng.uniform(0, [W - 260, H - 420], (max(COUNTS), 2))
    wh = rng.uniform([30, 60], [250, 400], (max(COUNTS), 2))
    all_boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    say("# %s, frame %d x %d, window %.2f s x %d alternating turns, arena of %d crops" % (torch.cuda.get_device_name(0), H, W, a.window, a.repeats, a.max_crops))
    say("# us per crop: median turn [fastest .. slowest]; speed-up = fp32 op list / fp16 path (medians)")
    say("%-15s %-8s %5s  %-28s %-28s %-28s %s" % ("network", "HxW", "crops", "fp16 path", "fp32 op list", "fused kernel", "speed-up"))
    for name in a.nets.split(","):
        width, ibn = reid.OSNET_NAMES[name]
        for (h, w) in SIZES:
            paths = [("half", reid.ReIDExtractor(None, width=width, ibn=ibn, size=(w, h), max_crops=a.max_crops, seed=1, half=True)),
                     ("fp32", reid.ReIDExtractor(None, width=width, ibn=ibn, size=(w, h), max_crops=a.max_crops, seed=1, fused=False))]
            if name == "osnet_x0_25" and (h, w) == (128, 64):
                paths.append(("fused", reid.ReIDExtractor(None, size=(w, h), max_crops=a.max_crops, seed=1)))
                assert paths[-1][1].fused
            assert paths[0][1].half and not paths[1][1].half and not paths[1][1].fused
            for n in COUNTS:
                boxes = all_boxes[:n]
                for _, ex in paths:
                    ex.features_for_boxes(frame, boxes)
                    ex.features_for_boxes(frame, boxes)
                t = {k: [] for k, _ in paths}
                for _ in range(a.repeats):
                    for k, ex in paths:
                        t[k].append(turn(ex, frame, boxes, a.window) / n * 1e6)
                cell = lambda k: "%9.2f [%8.2f .. %8.2f]" % (float(np.median(t[k])), min(t[k]), max(t[k])) if k in t else "-"
                say("%-15s %-8s %5d  %-28s %-28s %-28s %.2fx" % (name, "%dx%d" % (h, w), n, cell("half"), cell("fp32"), cell("fused"), float(np.median(t["fp32"]) / np.median(t["half"]))))
            del paths
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
