"""What non_max_suppression's options cost on the device (y7t_det_postprocess_ex), HIP events around Detector.postprocess, 30 calls each:
  * `classes` and `agnostic` on the candidates of scripts/time_nms.py's batch-1 configuration (yolov7-w6 @ 1280, nc = 10, ~2000 candidates from the fused Detect
    epilogues): rank sort + NMS with and without the options;
  * `multi_label` at conf 0.001 on yolov7-tiny (nc = 80) heads @ 640 against the best-class pass on the same heads (decode pass + rank sort + NMS).  The heads are
    planted: N(0, 1.5) logits, class logits 3 lower, objectness shifted so that about 20000 (anchor, class) pairs pass -- under the candidate capacity of 32768.
    python scripts/time_nms_opts.py"""
import os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from yolov7_tracker_amd import synth
from yolov7_tracker_amd.detector import arch, model


def timed(det, out, conf, reps=30, **kw):
    det.postprocess(out, conf, 0.45, None, **kw)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(); det.postprocess(out, conf, 0.45, None, **kw); e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    ps = det.plan.post[out.pset]
    return us[len(us) // 2], us[0], int(ps.cand[0]), int(ps.ndets[0])


frames_host = synth.make_frames(1, 80, 1280, seq_idx=0)
sd = bench.conditioned_state_dict(types.SimpleNamespace(arch="yolov7-w6", img=1280), 10, frames_host)
det = model.Detector(arch.yolov7_w6(10), sd, img_size=(1280, 1280), max_batch=1, seed=0)
frames = torch.from_numpy(frames_host).cuda()
bench.plant_objectness_bias(det, frames)
out = det.forward(frames, fuse_decode=0.01)
for name, kw in (("defaults (y7t_det_postprocess)", {}), ("classes=[0..4]", {"classes": [0, 1, 2, 3, 4]}), ("classes=[3]", {"classes": [3]}), ("agnostic", {"agnostic": True}),
                 ("classes=[0..4] + agnostic", {"classes": [0, 1, 2, 3, 4], "agnostic": True}), ("defaults again", {})):
    med, lo, cand, nd = timed(det, out, 0.01, **kw)
    print("w6 B=1 fused  %-32s candidates %5d  kept %3d  rank sort + NMS: median %.1f us, min %.1f us" % (name, cand, nd, med, lo), flush=True)
del det

det = model.Detector(arch.yolov7_tiny(80), None, img_size=(640, 640), max_batch=1, max_cand=32768, seed=0)
g = torch.Generator().manual_seed(5)
out = det(torch.rand((1, 3, 640, 640), generator=g))[0]
no = det.plan.det["no"]
raw = [torch.randn(det.head_tensor(l, 1).shape, generator=g) * 1.5 for l in range(len(det.plan.heads))]
flat = torch.cat([r.view(-1, no) for r in raw]).double()
cls = torch.sigmoid(flat[:, 5:] - 3.0)
lo_s, hi_s = -20.0, 5.0
for _ in range(40):                                        # the pair count is monotone in the shift
    mid = (lo_s + hi_s) / 2
    obj = torch.sigmoid(flat[:, 4] + mid)
    pairs = int(((cls * obj[:, None] > 0.001) & (obj[:, None] > 0.001)).sum())
    lo_s, hi_s = (lo_s, mid) if pairs >= 20000 else (mid, hi_s)
for l, r in enumerate(raw):
    v = r.view(r.shape[:3] + (3, no))
    v[..., 5:] -= 3.0
    v[..., 4] += lo_s
    det.head_tensor(l, 1).copy_(r.cuda())
for name, kw in (("best class", {}), ("multi_label", {"multi_label": True}), ("multi_label + agnostic", {"multi_label": True, "agnostic": True}), ("best class again", {})):
    med, lo, cand, nd = timed(det, out, 0.001, **kw)
    print("tiny nc=80 @640 conf 0.001  %-24s candidates %5d (capacity %d)  kept %3d  decode + rank sort + NMS: median %.1f us, min %.1f us"
          % (name, cand, det.max_cand, nd, med, lo), flush=True)
