"""Time the detector launch list alone (y7t_det_forward_ops over the whole plan: no input layout, no decode / NMS) for the five graphs beyond w6 / tiny -- yolov7,
yolov7x (640 x 640), yolov7-e6, -d6, -e6e (1280 x 1280) -- at batch 8 and batch 1 on one GPU, with HIP events after a warm-up, and print the census of kernel
names of each launch list.  Seeded weights (BatchNorm statistics calibrated on a small image: the values do not matter for the time).  Reports numbers, gates nothing.

    python scripts/time_family.py [--iters 20] [--warmup 3] [graph ...]
"""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRAPHS = (("yolov7", 640), ("yolov7x", 640), ("yolov7-e6", 1280), ("yolov7-d6", 1280), ("yolov7-e6e", 1280))


def main():
    import torch
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.detector import arch, graph, model, weights
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    L = _lib.load()
    for name, size in GRAPHS:
        if a.graphs and name not in a.graphs:
            continue
        spec = arch.ARCHS[name](80)
        nodes, _ = graph.parse(spec)
        sd = weights.calibrate_bn(nodes, weights.random_state_dict(graph.lower(nodes, 128, 128, 1).wlayout, 0, bn_bias_mean=2.0), hw=(128, 128), seed=0)
        for B in (8, 1):
            det = model.Detector(spec, sd, img_size=(size, size), max_batch=B)
            p = det.plan
            img = torch.rand((B, 3, size, size), generator=torch.Generator().manual_seed(0)).cuda()
            det(img)
            names = det.launch_list(B)
            s = _lib.stream_ptr()
            for _ in range(a.warmup):
                _lib.check(L.y7t_det_forward_ops(p.handle, B, 0, -1, s))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                _lib.check(L.y7t_det_forward_ops(p.handle, B, 0, -1, s))
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            t = p.ops["type"]
            add_elems = sum(int(o["H"]) * int(o["W"]) * int(o["Cin"]) for o in p.ops if int(o["type"]) == 3)
            print("%-11s %4d x %-4d batch %d: launch list %8.3f ms = %7.3f ms/frame, %6.1f GFLOP/frame, %5.1f TFLOP/s; %d ops (%d conv, %d pool, %d add, %d upsample)%s"
                  % (name, size, size, B, ms, ms / B, det.gflop_per_frame, det.gflop_per_frame * B / ms, len(p.ops), int((t == 0).sum()), int((t == 2).sum()),
                     int((t == 3).sum()), int((t == 1).sum()), "; adds: %.1f M elements/frame" % (add_elems / 1e6) if add_elems else ""), flush=True)
            fam = collections.Counter(n.split(" ")[0] for n in names)
            print("    kernels: " + ", ".join("%s x %d" % kv for kv in sorted(fam.items())), flush=True)
            del det, p
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
