"""What augmented inference (Detector.forward_augment: three passes at scales 1, 0.83, 0.67 + one NMS over the union, models/yolo.py:301-317) costs on the device beside
the plain forward, yolov7-w6 @ 1280 x 1280 (nc = 10, uint8 frames, planted objectness so that a plain forward has ~2000 candidates), batch 1 and batch 8.
HIP events, 30 repetitions after warm-up, median and minimum:
  * plain: forward with the fused Detect decode + rank sort + NMS (the tracking path), and forward with plain heads + decode pass + rank sort + NMS;
  * augmented: forward_augment + postprocess, and the same chain with events between its pieces -- the two scale launches, the three forwards, the three
    appending decode passes, the NMS;
  * k_tta_scale_layout alone: achieved bytes/s against its algorithmic bytes (every source pixel read once, every layout element written once).
The FLOP ratio of the three sizes is 1 + (1088 / 1280)^2 + (896 / 1280)^2 = 2.21; the time ratio is what this prints.
    python scripts/time_tta.py [out.txt]      # appends its lines to out.txt (default profiles/tta_timing.txt)"""
import ctypes, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from yolov7_tracker_amd import _lib, synth
from yolov7_tracker_amd.detector import arch, model

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tta_timing.txt")
REPS = 30
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stat(us):
    us = sorted(us)
    return us[len(us) // 2], us[0]


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return stat([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])


def pieces(det, frames, reps=REPS):
    """forward_augment + postprocess step by step (the calls of Detector.forward_augment, in its order), an event after every piece -> name -> (median, min) us"""
    B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    gs = int(det.stride.max())
    sizes = [model.tta_pass_sizes(H, W, float(r), gs) for r in (1, 0.83, 0.67)]
    out = det.forward_augment(frames)      # plans and the augmented set exist
    aug, s = out.aug, _lib.stream_ptr()
    acc = {}
    for rep in range(reps + 3):
        marks = [("start", torch.cuda.Event(enable_timing=True))]
        marks[0][1].record()
        row_base = 0
        for i, (ratio, flip, ((hs, ws), pad)) in enumerate(zip((1, 0.83, 0.67), (0, 3, 0), sizes)):
            det._select(pad)
            p = det.plan
            if i == 0:
                first = det._front(frames, True, B, H, W, None, 0)
            else:
                _lib.check(det._L.y7t_tta_scale_layout(_lib.ptr(frames), 1, B, H, W, flip, hs, ws, pad[0], pad[1], int(p.reorg), _lib.ptr(p.arena), p.in_ld, s))
                first = 0
                marks.append(("scale %.2f" % ratio, torch.cuda.Event(enable_timing=True))); marks[-1][1].record()
            det._run_ops(B, first, -1, None, 0)
            marks.append(("forward %.2f (%dx%d)" % (ratio, pad[0], pad[1]), torch.cuda.Event(enable_timing=True))); marks[-1][1].record()
            tp = _lib.TtaPass(float(ratio), flip, float(W if flip == 3 else 0), row_base)
            _lib.check(det._L.y7t_det_decode_append(p.head_ptrs, p.ny, p.nx, p.strides, p.anchors, len(p.heads), p.det["na"], p.det["no"], B, 0.01, aug.cap, model.MAX_NMS, 0,
                                                    ctypes.byref(tp), int(i == 0), _lib.ptr(aug.ws), aug.ws.numel(), s))
            marks.append(("decode_append %.2f" % ratio, torch.cuda.Event(enable_timing=True))); marks[-1][1].record()
            row_base += aug.rows[i]
        det._select(sizes[0][1])
        det.postprocess(out, 0.01, 0.45, None)
        marks.append(("rank sort + NMS over the union", torch.cuda.Event(enable_timing=True))); marks[-1][1].record()
        torch.cuda.synchronize()
        if rep >= 3:
            for (_, a), (name, b) in zip(marks, marks[1:]):
                acc.setdefault(name, []).append(a.elapsed_time(b) * 1e3)
            acc.setdefault("all pieces", []).append(marks[0][1].elapsed_time(marks[-1][1]) * 1e3)
    return {k: stat(v) for k, v in acc.items()}, int(aug.cand[:B].max()), int(aug.ndets[0])


for B in (1, 8):
    frames_host = synth.make_frames(B, 80, 1280, seq_idx=0)
    sd = bench.conditioned_state_dict(types.SimpleNamespace(arch="yolov7-w6", img=1280), 10, frames_host[:1])
    det = model.Detector(arch.yolov7_w6(10), sd, img_size=(1280, 1280), max_batch=B, seed=0)
    frames = torch.from_numpy(frames_host).cuda()
    bench.plant_objectness_bias(det, frames)
    say("== yolov7-w6 @ 1280 x 1280, nc = 10, uint8 frames, batch %d, conf 0.01, %d repetitions: median / min in us" % (B, REPS))
    fused = timed(lambda: det.postprocess(det.forward(frames, fuse_decode=0.01), 0.01, 0.45, None))
    cand = int(det.plan.post[0].cand[:B].max())
    plain = timed(lambda: det.postprocess(det.forward(frames), 0.01, 0.45, None))
    say("plain forward, fused Detect decode + rank sort + NMS       %9.1f / %9.1f   (candidates per frame up to %d)" % (fused + (cand,)))
    say("plain forward, plain heads + decode pass + rank sort + NMS  %9.1f / %9.1f" % plain)
    whole = timed(lambda: det.postprocess(det.forward_augment(frames), 0.01, 0.45, None))
    parts, acand, nd = pieces(det, frames)
    say("augmented: forward_augment + postprocess                   %9.1f / %9.1f   (union candidates per frame up to %d, kept %d)" % (whole + (acand, nd)))
    for name, v in parts.items():
        say("    %-52s %9.1f / %9.1f" % ((name,) + v))
    say("time ratio augmented / plain (plain heads): %.2f; augmented / plain (fused decode): %.2f; FLOP ratio of the three sizes: %.2f"
        % (whole[0] / plain[0], whole[0] / fused[0], 1 + (1088 / 1280) ** 2 + (896 / 1280) ** 2))
    # the scale + layout kernel alone, both scaled passes, uint8 and float32 sources: algorithmic bytes = the source once + the layout tensor once
    f32 = (frames[..., [2, 1, 0]].permute(0, 3, 1, 2).float() / 255.0).contiguous()
    for kind, src, src_bytes in (("u8", frames, B * 1280 * 1280 * 3), ("f32", f32, B * 3 * 1280 * 1280 * 4)):
        for ratio in (0.83, 0.67):
            (hs, ws), pad = model.tta_pass_sizes(1280, 1280, ratio, 64)
            det._select(pad)
            p = det.plan
            med, lo = timed(lambda: _lib.check(det._L.y7t_tta_scale_layout(_lib.ptr(src), int(kind == "u8"), B, 1280, 1280, 3, hs, ws, pad[0], pad[1], int(p.reorg),
                                                                           _lib.ptr(p.arena), p.in_ld, _lib.stream_ptr())))
            nbytes = src_bytes + B * (pad[0] // 2) * (pad[1] // 2) * 16 * 2
            say("k_tta_scale_layout<%s> ratio %.2f flip 3 -> %dx%d in %dx%d: %8.1f / %8.1f us, %.1f MB algorithmic, %.0f GB/s at the median (event-timed single launch: launch overhead included)"
                % (kind, ratio, hs, ws, pad[0], pad[1], med, lo, nbytes / 1e6, nbytes / med / 1e3))
    del det
    torch.cuda.empty_cache()

with open(OUT, "a") as f:
    f.write("\n".join(lines) + "\n")
