#!/usr/bin/env python
"""bench.py -- end-to-end fps (detect + track) of the hot path on N MI355X GPUs of one node.

Workload (BASELINE.json configs[1]): YOLOv7-w6 @ 1280x1280 (nc=10, VisDrone) + ByteTrack, one synthetic
VisDrone-shape sequence per GPU, ~80 objects per frame.  A "step" is one pass of the hot path over one batch of
`--batch` consecutive frames of the sequence, frames already resident in HBM as uint8 BGR:

    input layout (BGR->RGB, /255, ReOrg, fp16 NHWC)  ->  107 MFMA implicit-GEMM convs (+ SPPCSPC pools, upsamples)
    ->  Detect decode + candidate filter + rank sort + bitmask NMS + scale_coords/round      [stream C, on a staged copy of the heads]
    ->  ByteTrack frame step (multi_predict, 3 x IoU cost + LAPJV, Kalman updates, list bookkeeping), one fused
        kernel per frame, strictly in frame order                                              [stream B, waits on C]

No trained checkpoint ships with the reference, so weights are seeded random (BN statistics calibrated at init) and
-- exactly as SURVEY.md section 8d prescribes -- the tracker is fed the synthetic ground-truth detections of the same
scene while decode+NMS run on the detector's real output (the Detect objectness bias is planted so that ~2000 anchors
per frame pass conf_thres = 0.01, a typical VisDrone candidate load).

One process per GPU (`torch.distributed.run`), sequences are independent -> weak scaling, no data-path collective;
RCCL is used once, for the result gather (+ id re-basing so ids equal the reference's single-process global counter).
Prints ONE JSON line (rank 0).
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_MFMA_F16 = 2.5e15      # dense fp16/bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM = 8.0e12           # HBM3E, same guide (6.3 TB/s achievable)
GFLOP_PER_FRAME_W6 = 354.9   # 177.45 GMAC x 2, yolov7-w6 deploy graph, nc=10, 1280x1280


# Frames per step.  Every kernel of the list that runs several workgroups per CU pays for its last, partly filled round of workgroups; how much depends on the batch:
# at 32 frames the 80 x 80 layers have 25 x 32 pixel tiles x 2 channel tiles = 1600 workgroups on 512 slots (3.125 rounds -> 4), the 40 x 40 strips 663 on 512 (1.3 -> 2).
# Measured in one session (profiles/r05_batch_and_latency.txt): 24 frames 0.3051 of the MFMA peak, 32 frames 0.3194 / 0.3200, 40 frames 0.3250 (2207 vs 2169 fps).
# Round 6: 40 was the ceiling while a batch had to keep every tensor below the 2 GiB a buffer descriptor's 32-bit byte offsets reach (the 640 x 640 x 64-channel tensor of 41
# frames passes it); now a conv whose tensors are larger goes out as several launches over runs of frames (csrc/y7t_detector.hip::forward_impl) and one session measured
# 40 frames 0.3197 / 0.3194, 48 0.3274, 56 0.3300, 64 0.3343 / 0.3331, 80 0.3390, 96 0.3408, 128 0.3429 (profiles/r06_batch_80.txt): 80 is where the curve bends
# (the 20 x 20 layers are then 250 / 500 tiles on 256 CUs x 1 / 2 slots, the 40 x 40 strips 6.5 rounds).
DEFAULT_BATCH = 80


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="GPUs (= ranks) of this node; default: WORLD_SIZE under a launcher, else 1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="frames per step (consecutive frames of the sequence); default %d: see DEFAULT_BATCH" % DEFAULT_BATCH)
    ap.add_argument("--n_obj", type=int, default=None, help="objects in the synthetic scene (default: 80 for cfg2, 500 for cfg3)")
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg3", "cfg4"],
                    help="cfg2 (default, BASELINE's metric): w6@1280 + ByteTrack, ~80 objects.  cfg3: BASELINE configs[2], w6@1280 + BoT-SORT "
                         "(xywh Kalman, per-frame camera-motion warp), 500 objects -- stresses the IoU matrices / linear assignment")
    ap.add_argument("--img", type=int, default=1280)
    ap.add_argument("--arch", default="yolov7-w6")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--no_latency_mode", action="store_true")
    ap.add_argument("--seqs", type=int, default=1, help="sequences per GPU: the frames of a step are split over S independent sequences, each with its own "
                    "tracker and stream (their frame-step chains run side by side); default 1 = one sequence per GPU (the metric's configuration)")
    ap.add_argument("--tracker_threads", type=int, default=0, help="threads of the tracker step workgroup (64 / 256 / 1024; 0 = the library's rule)")
    ap.add_argument("--prio", type=int, default=0, help="1: the detector forward runs on a high-priority HIP stream (measured: no gain); 2: the tracker chain's stream does")
    ap.add_argument("--rotate_batches", type=int, default=4, help="distinct resident input batches consumed round-robin by the timed steps (1 = the same batch every step)")
    ap.add_argument("--hipgraph", type=int, default=0, help="1: replay detector+NMS as one captured hipGraph (no NMS overlap); "
                    "2: the forward as two captured hipGraphs (before / after the gate event), same pipeline as eager")
    ap.add_argument("--cpu_frames", type=int, default=20, help="frames of the detector oracle in the CPU baseline (about 10 s of CPU work on a GPU box at 32 threads)")
    ap.add_argument("--chained_frames", type=int, default=8, help="frames of the chained detect -> NMS -> ByteTrack parity run in `parity.chained` (0: off)")
    ap.add_argument("--nms_gate_div", type=int, default=NMS_GATE_DIV, help="the previous batch's rank sort + NMS is released when the forward reaches its first op on a map of "
                    "img / this (8: behind the 640^2 / 320^2 layers; 16: behind the 160^2 ones too)")
    ap.add_argument("--no_coupled", action="store_true", help="skip the third timed pass (`coupled`: the tracker steps consume the same step's NMS output on the device)")
    ap.add_argument("--no_other_workloads", action="store_true", help="skip the short cfg3 / cfg4 runs behind the headline line (`other_workloads`)")
    ap.add_argument("--weights", default="conditioned", choices=["conditioned", "chaotic"],
                    help="seeded random weights of the timed detector.  conditioned (default): BatchNorm shifts ~ +2, statistics calibrated on frame 0, damped "
                         "width / height logits -- a random network that does not amplify rounding noise, so that `parity` (heads, pre-NMS candidates, boxes "
                         "against the fp32 oracle) describes the TIMED weights; chaotic: iid zero-mean weights (rounds 1-2)")
    ap.add_argument("--tracker_launch", default="frames", choices=["per_frame", "frames"],
                    help="frames: the tracker frame steps of a step's frames as ONE launch per sequence (y7t_tracker_step_frames) instead of one launch per frame")
    ap.add_argument("--cu_reserve", type=int, default=0, help="N > 0: the tracker chain's stream owns N compute units (hipExtStreamCreateWithCUMask), the "
                    "detector's stream the rest -- the single-workgroup frame steps no longer share CUs with 256-thread convolution workgroups")
    ap.add_argument("--cu_reserve_nms", type=int, default=0, help="1: rank sort + NMS run on the reserved compute units too")
    ap.add_argument("--halves", type=int, default=1, choices=[1, 2], help="2: experiment -- each step as two interleaved half-batch forwards")
    ap.add_argument("--mode", default="sequences", choices=["sequences", "frames"],
                    help="sequences (default): one sequence per GPU, weak scaling, no data-path exchange.  frames: ONE sequence, batches of "
                         "frames detected round-robin over the GPUs, detections sent to the tracker on rank 0 (strong scaling, SURVEY 8e)")
    ap.add_argument("--full", action="store_true", help="also run what the headline figure does not need: the pinned-host and coupled timed passes, the launch-list "
                    "probe and PMC traffic, the cfg4 ReID figures, latency mode, the tracker roofline, the CPU baseline with parity, the cfg3 / cfg4 child runs")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64): "
                    "detections, detection_counts, tracks, track_counts (rank 0's sequence)")
    args = ap.parse_args()
    # under a launcher (torchrun / the driver's torch.distributed.run / SLURM: WORLD_SIZE with RANK or LOCAL_RANK) the world size comes from the environment and
    # --gpus, if given, must agree; WORLD_SIZE=1 without a rank variable is a container default, not a launcher
    args.launched = "WORLD_SIZE" in os.environ and ("RANK" in os.environ or "LOCAL_RANK" in os.environ or int(os.environ["WORLD_SIZE"]) > 1)
    if args.gpus is None:
        args.gpus = int(os.environ["WORLD_SIZE"]) if args.launched else 1
    return args


TRACKER_THREADS = 0      # --tracker_threads: 0 = the library's rule (four waves up to 384 detections, eight beyond: csrc/y7t_tracker.hip::step_threads)


def make_opts():
    return types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="default", img_size=1280, iou_thresh=0.5,
                                 max_tracks=512, max_dets=512, tracker_threads=TRACKER_THREADS)


NMS_GATE_DIV = 8
LEVEL_QUOTA = (0.55, 0.2, 0.15, 0.1)      # share of the candidates each Detect level (stride 8 / 16 / 32 / 64) supplies: all four live, weighted towards the fine ones


def plant_objectness_bias(det, frames, target=2000):
    """~`target` anchors per frame above conf_thres = 0.01 (state dict and device blob both updated), every Detect level supplying its quota of them"""
    return det.plant_objectness_bias(frames, target, level_quota=LEVEL_QUOTA if len(det.plan.heads) == len(LEVEL_QUOTA) else None)


def dump_outputs(path, dets, ndets, rows, cap_t):
    """--dump-outputs: what a caller of the timed path receives for the frames of its last step -- the detector's NMS output (B, 300, 6)
    [x1, y1, x2, y2, conf, cls] and the tracker's returned tracks (B, cap_t, 7) [id, x, y, w, h, cls, score], each with its per-frame count
    and with the rows past that count zeroed (buffer contents a caller never reads)"""
    nd = ndets.cpu().numpy().astype(np.int64)
    d = dets.cpu().numpy().astype(np.float32)
    d[np.arange(d.shape[1])[None, :] >= nd[:, None]] = 0
    r = rows.cpu().numpy()
    nt = np.ascontiguousarray(r[:, cap_t]).view(np.int32)[:, 0].astype(np.int64)      # row cap_t of a frame starts with its track count
    t = r[:, :cap_t, :7].astype(np.float64)
    t[np.arange(cap_t)[None, :] >= nt[:, None]] = 0
    os.makedirs(path, exist_ok=True)
    for name, a in (("detections", d), ("detection_counts", nd.astype(np.float64)), ("tracks", t), ("track_counts", nt.astype(np.float64))):
        np.save(os.path.join(path, name + ".npy"), a)


def cpu_baseline(args, det, frames_host, dets_seq, gpu_heads0=None, gpu_dets0=None, gpu_cands0=None, gpu_kept_rows0=None):
    """the oracle (CPU restatement of the reference path, kind='port') timed on this host's cores on a bounded sample:
    `cpu_frames` frames through the torch-fp32 detector + NMS oracle, 100 frames through the numpy ByteTrack oracle.
    The oracle's output for frame 0 is also the checker of the timed GPU run: -> (cpu_baseline dict, parity dict)."""
    from oracle import detector_torch as dt, tracker_np
    f = frames_host[:1]
    img = (torch.from_numpy(f[..., ::-1].copy()).permute(0, 3, 1, 2).float() / 255.0).contiguous()
    sd = {k: v for k, v in det._sd.items()}
    # "the box's own host cores" -- why 32 threads and not os.cpu_count(): measured on the GPU box in round 6 (session r6g, 256 logical cores): the
    # detector oracle takes 82.3 s per frame with 256 threads against 0.395 s with 32 (torch's CPU convolutions oversubscribe and thrash), and timing that inside
    # every bench run would cost five minutes.  The baseline is the port at the thread count where it is FASTEST on such hosts; hosts with fewer cores use them all.
    ncores = min(os.cpu_count(), 32)
    torch.set_num_threads(ncores)
    dt.forward(det.nodes, sd, img, det.spec["anchors"])      # (untimed: thread pool, allocator)
    t0 = time.perf_counter()
    for _ in range(args.cpu_frames):
        dec, raw_ref = dt.forward(det.nodes, sd, img, det.spec["anchors"])
    t_det = (time.perf_counter() - t0) / args.cpu_frames
    by_threads = {ncores: t_det}
    torch.set_num_threads(ncores)
    parity = None
    if gpu_heads0 is not None:      # the heads the timed launch list left for frame 0 vs the fp32 oracle's (same weights, same frame)
        rel = [float((a - b).abs().mean() / b.std()) for a, b in zip(gpu_heads0, raw_ref)]
        parity = {"checker": "oracle/detector_torch.py fp32 forward of frame 0 (same seeded weights)",
                  "heads_mean_abs_err_over_logit_std": [round(r, 5) for r in rel]}
        if gpu_cands0 is not None:      # SURVEY 8a's bar BEFORE the NMS (no greedy order to amplify a rounding difference): every candidate, not a percentage
            want = dt.candidates(dec[0], 0.01)
            st = dt.compare_candidate_sets(gpu_cands0, want, 0.01, px=1.0, dconf=5e-3, iou=0.99)      # 8a: same class, IoU >= 0.99 OR |dcoord| <= 1 px, |dconf| <= 5e-3
            st.pop("worst_rows", None)
            st["n_out_of_coord_bar"] = len(st.pop("out_of_coord_bar", []))
            ny = [args.img // s_ for s_ in (8, 16, 32, 64)][:len(raw_ref)]
            rows0 = np.cumsum([0] + [int(r_.shape[1] * r_.shape[2] * r_.shape[3]) for r_ in raw_ref])
            st["candidates_per_detect_level"] = np.bincount(np.searchsorted(rows0, np.array(sorted(gpu_cands0)), side="right") - 1, minlength=len(ny))[:len(ny)].tolist()
            parity["candidates_before_nms"] = st
            if gpu_kept_rows0 is not None:      # final boxes by anchor row: rows kept by both at the bar; rows kept by one side only traced to the tied greedy decision
                kw = dt.nms_rows(want, 0.45)
                both = sorted(set(int(r_) for r_ in kw) & set(int(r_) for r_ in gpu_kept_rows0))
                common = set(gpu_cands0) & set(want)
                noise = max([1e-4] + [abs(gpu_cands0[r_][1] - want[r_][1]) for r_ in common])
                ex = dt.explain_kept_set_difference(gpu_cands0, gpu_kept_rows0, want, kw, score_noise=noise)
                reasons = {}
                for v in ex.values():
                    reasons[v or "UNEXPLAINED"] = reasons.get(v or "UNEXPLAINED", 0) + 1
                parity["boxes_by_anchor_row"] = {"oracle_keeps": int(len(kw)), "device_keeps": int(len(gpu_kept_rows0)), "kept_by_both": len(both),
                                                 "kept_by_one_side_only": len(ex), "reasons": reasons, "score_noise": round(float(noise), 6)}
        if gpu_dets0 is not None:
            ref = dt.non_max_suppression(dec, 0.01, 0.45)[0]
            rb = dt.scale_coords_round((args.img, args.img), ref[:, :4], (args.img, args.img))
            d = gpu_dets0
            used, m = torch.zeros(len(d), dtype=torch.bool), 0
            for row, box in zip(ref, rb):
                near = (d[:, :4] - box).abs().max(1).values <= 1.0
                if not bool(((~used) & near).any()):      # 8a's other coordinate bar: IoU >= 0.99 (the several-hundred-pixel boxes of the coarse levels)
                    near = torch.tensor([dt.box_iou_1(x_, box) >= 0.99 for x_ in d[:, :4].numpy()])
                ok = (~used) & (d[:, 5] == row[5]) & near & ((d[:, 4] - row[4]).abs() <= 5e-3)
                if ok.any():
                    used[int(torch.nonzero(ok)[0])] = True
                    m += 1
            parity.update({"boxes_oracle": int(len(ref)), "boxes_device": int(len(d)), "boxes_matched_same_class_1px_or_iou99_conf5e-3": m})
        parity["third_party"] = ("unpinned: lap.lapjv, cython_bbox.bbox_overlaps, torchvision.ops.nms and cv2 are not vendored by the reference and not "
                                 "installed here -- restated from their published algorithms in oracle/y7t_oracle.c / oracle/letterbox_np.py and cross-checked "
                                 "against scipy.optimize.linear_sum_assignment / brute force; everything the reference itself implements is pinned to its own "
                                 "classes (tests/golden, oracle/ref_harness.py)")
    # NMS load comparable to the GPU run: plant ~2000 candidates
    dec = dec.clone()
    dec[..., 4] = 0.0
    idx = torch.randperm(dec.shape[1], generator=torch.Generator().manual_seed(0))[:2000]
    dec[0, idx, 4] = torch.rand(2000) * 0.9 + 0.05
    dec[..., 5:] = torch.rand_like(dec[..., 5:])
    t0 = time.perf_counter()
    dt.non_max_suppression(dec, 0.01, 0.45)
    t_nms = time.perf_counter() - t0
    n = min(100, len(dets_seq))
    t0 = time.perf_counter()
    tracker_np.run("botsort" if args.workload == "cfg3" else "bytetrack", dets_seq[:n], **({"kalman_format": "botsort"} if args.workload == "cfg3" else {}))
    t_trk = (time.perf_counter() - t0) / n
    fps = 1.0 / (t_det + t_nms + t_trk)
    return {"value": round(fps, 3), "unit": "frames/s", "cores": ncores, "host_cpu_count": os.cpu_count(), "kind": "port",
            "detector_s_per_frame_by_threads": {str(k_): round(v_, 3) for k_, v_ in by_threads.items()},
            "why_not_every_core": "measured on a 256-core GPU box (round 6, profiles/r06_small_experiments.txt): 82.3 s per frame with 256 threads against 0.395 s with 32 -- "
                                  "torch's CPU convolutions thrash when oversubscribed; 32 threads is where the port is fastest on such hosts",
            "reference_over_port": {"as_its_cli_runs_it_no_no_grad": 0.27, "with_no_grad": 0.56,
                                    "note": "fps of the reference's OWN Model + non_max_suppression + ByteTrack divided by this port's, same job, the 8-core build container "
                                            "(the reference does not exist on the GPU box): 0.45 and 0.93 fps vs 1.65 fps, outputs equal -- profiles/r03_cpu_reference_vs_port.txt. "
                                            "`value` is the PORT's speed: the reference itself is 1.8-3.7x slower"},
            "sample": "%d frames 1280x1280 through the torch-fp32 detector oracle (%.2f s/frame, %d threads) + 1 NMS call on 2000 "
                      "candidates (%.1f ms) + %d frames through the numpy tracker oracle (%.2f ms/frame, 1 thread)"
                      % (args.cpu_frames, t_det, ncores, t_nms * 1e3, n, t_trk * 1e3)}, parity


def roofline_tracker(det, frames, nc, img):
    """SURVEY 8d / VERDICT r3 missing 5: the tracker-side pieces against THEIR roof (HBM), each launched alone on an idle GPU, device time by HIP events over `reps`
    back-to-back launches, algorithmic bytes as SURVEY 8d counts them: multi_predict 1152 B per track (mean + covariance read and written, tracker/kalman_filter.py:289-329),
    IoU cost 32 (N + M) B in + 8 N M B out (tracker/matching.py:44-82), decode + NMS 102 000 x (5 + nc) x 4 B of head tensors read per 1280^2 frame
    (utils/general.py:607-695; the unfused y7t_det_postprocess path -- in the timed pipeline the decode sits in the Detect convs' epilogue and those tensors are never written).
    These are KB-to-MB working sets: launch latency bounds them, the GB/s figure says how far from the 8 TB/s roof that leaves them."""
    from yolov7_tracker_amd import _lib
    L = _lib.load()
    out = {"peak": PEAK_HBM / 1e9, "unit": "GB/s", "bound": "hbm (latency-bound at these sizes)", "pieces": {}}

    def timed(fn, reps=200):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps       # us per launch

    g = torch.Generator(device="cuda").manual_seed(0)
    for n_trk, n_det in ((100, 80), (500, 500)):
        mean = torch.rand((n_trk, 8), dtype=torch.float64, device="cuda", generator=g) * 100 + 50
        a = torch.rand((n_trk, 8, 8), dtype=torch.float64, device="cuda", generator=g)
        cov = a @ a.transpose(1, 2) + torch.eye(8, dtype=torch.float64, device="cuda")
        us = timed(lambda: _lib.check(L.y7t_kf_multi_predict_f64(0, _lib.ptr(mean), _lib.ptr(cov), None, n_trk, _lib.stream_ptr())))
        by = 1152 * n_trk
        out["pieces"]["kf_multi_predict_%d_tracks" % n_trk] = {"us_per_frame": round(us, 2), "algorithmic_bytes": by, "achieved": round(by / us / 1e3, 3)}
        xy = torch.rand((n_trk + n_det, 2), dtype=torch.float64, device="cuda", generator=g) * 1000
        wh = torch.rand((n_trk + n_det, 2), dtype=torch.float64, device="cuda", generator=g) * 80 + 10
        bx = torch.cat([xy, xy + wh], 1).contiguous()
        ta, tb = bx[:n_trk].contiguous(), bx[n_trk:].contiguous()
        cost = torch.empty((n_trk, n_det), dtype=torch.float64, device="cuda")
        us = timed(lambda: _lib.check(L.y7t_iou_cost_f64(_lib.ptr(ta), n_trk, _lib.ptr(tb), n_det, _lib.ptr(cost), _lib.stream_ptr())))
        by = 32 * (n_trk + n_det) + 8 * n_trk * n_det
        out["pieces"]["iou_cost_%dx%d" % (n_trk, n_det)] = {"us_per_frame": round(us, 2), "algorithmic_bytes": by, "achieved": round(by / us / 1e3, 3)}
    B = frames.shape[0]
    o = det.forward(frames)                  # plain forward: the four head tensors are written
    torch.cuda.synchronize()
    us = timed(lambda: det.postprocess(o, 0.01, 0.45, None), reps=10) / B
    by = sum(3 * (img // s_) ** 2 for s_ in (8, 16, 32, 64)) * (5 + nc) * 4
    out["pieces"]["decode_nms_unfused"] = {"us_per_frame": round(us, 2), "algorithmic_bytes": by, "achieved": round(by / us / 1e3, 3), "frames_per_launch": int(B),
                                            "candidates_per_frame": int(det.plan.cand[:B].float().mean().item())}
    return out


def conditioned_state_dict(args, nc, frames_host):
    """seeded weights that do not amplify rounding noise (tests/test_detector_pinned_gpu.py::smooth_det): BatchNorm shifts ~ +2 with the statistics
    calibrated on frame 0 (SiLUs in their near-linear region: the relative growth of a perturbation per layer drops from ~1.1 to ~1.0), and a
    VisDrone-like head (width / height logits damped -> boxes of roughly anchor size)"""
    from yolov7_tracker_amd.detector import arch, graph, weights
    spec = arch.ARCHS[args.arch](nc)
    img = (torch.from_numpy(frames_host[:1][..., ::-1].copy()).permute(0, 3, 1, 2).float() / 255.0).contiguous()
    nodes, _ = graph.parse(spec)
    plan = graph.lower(graph.parse(spec)[0], args.img, args.img, 1)
    torch.set_num_threads(min(os.cpu_count(), 32))
    sd = weights.calibrate_bn(nodes, weights.random_state_dict(plan.wlayout, 0, bn_bias_mean=2.0), seed=0, image=img)
    na, no = 3, nc + 5
    for k in list(sd):
        if ".m." in k and k.endswith(".weight"):                 # Detect 1x1 convs: rows (anchor, [x, y, w, h, obj, cls...])
            w = sd[k].clone().view(na, no, -1)
            w[:, 2:4] *= 0.25
            sd[k] = w.view(na * no, -1, 1, 1)
    return sd


def parity_well_conditioned(args, nc, frames_host):
    """image -> heads -> boxes of frame 0 on seeded weights that do not amplify rounding noise (BatchNorm shifts ~ +2, statistics calibrated on
    the frame; weights.random_state_dict) against the fp32 oracle: the end-to-end check tests/test_detector_pinned_gpu.py makes at 32 frames"""
    from oracle import detector_torch as dt
    from yolov7_tracker_amd.detector import arch, graph, model, weights
    H = W = args.img
    spec = arch.ARCHS[args.arch](nc)
    img = (torch.from_numpy(frames_host[:1][..., ::-1].copy()).permute(0, 3, 1, 2).float() / 255.0).contiguous()
    nodes, _ = graph.parse(spec)
    plan = graph.lower(graph.parse(spec)[0], H, W, 1)
    sd = weights.calibrate_bn(nodes, weights.random_state_dict(plan.wlayout, 0, bn_bias_mean=2.0), seed=0, image=img)
    na, no = 3, nc + 5
    for k in list(sd):
        if ".m." in k and k.endswith(".weight"):                 # VisDrone-like head: damped width / height logits
            w = sd[k].clone().view(na, no, -1)
            w[:, 2:4] *= 0.25
            sd[k] = w.view(na * no, -1, 1, 1)
    d2 = model.Detector(spec, sd, img_size=(H, W), max_batch=2)
    fr = torch.from_numpy(frames_host[:2]).cuda()
    plant_objectness_bias(d2, fr)
    out = d2.forward(fr, fuse_decode=0.01)
    dets, nd = d2.postprocess(out, 0.01, 0.45, None)
    torch.cuda.synchronize()
    raw = [r[:1].cpu() for r in out.raw()]
    dec, ref = dt.forward(d2.nodes, d2._sd, img, spec["anchors"])
    rel = [float((a - b).abs().mean() / b.std()) for a, b in zip(raw, ref)]
    r = dt.non_max_suppression(dec, 0.01, 0.45)[0]
    rb = dt.scale_coords_round((H, W), r[:, :4], (H, W))
    d = dets[0, :int(nd[0])].cpu()
    used, m = torch.zeros(len(d), dtype=torch.bool), 0
    for row, box in zip(r, rb):
        ok = (~used) & (d[:, 5] == row[5]) & ((d[:, :4] - box).abs().max(1).values <= 1.0) & ((d[:, 4] - row[4]).abs() <= 5e-3)
        if ok.any():
            used[int(torch.nonzero(ok)[0])] = True
            m += 1
    return {"heads_mean_abs_err_over_logit_std": [round(v, 5) for v in rel], "boxes_oracle": int(len(r)), "boxes_device": int(len(d)),
            "boxes_matched_same_class_1px_conf5e-3": m}


def chained_parity(args, nc, frames_host, n_frames):
    """VERDICT r4 next 1, the bench-line form of tests/test_chained_gpu.py: the reference's per-frame loop as ONE chain (tracker/track.py:138-174,234-244) on the first
    `n_frames` frames of the scene -- DEVICE forward -> decode + NMS -> scale_coords / round -> ByteTrack.update (the detector's own output feeds the tracker: no synthetic
    detections) against the ORACLE chain (fp32 network, NMS restatement, numpy ByteTrack).  Conditioned weights with the objectness rows x 2.75 (a head that is confident
    about ~100 of its ~2000 candidates per frame; otherwise no row ever exceeds the tracker's 0.2 / 0.3 thresholds), candidates from the two fine Detect levels (the
    small-object regime).  Reports: the seam (oracle tracker on the device's hand-over == device tracker: ids / classes exact, tlwh 1e-6), how the two hand-overs differ,
    and HOTA / IDF1 / MOTA of the device chain's tracks scored against the oracle chain's through the TrackEval-style harness."""
    import tempfile
    import types as _types
    from oracle import chained
    from yolov7_tracker_amd.detector import arch, model
    from yolov7_tracker_amd.tracker import track as cli
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.bytetrack import ByteTrack
    gain, quota = 2.75, (0.9, 0.1, 0.0, 0.0)
    H = W = args.img
    fh = frames_host[:n_frames]
    sd = conditioned_state_dict(args, nc, frames_host)
    na, no = 3, nc + 5
    for k in list(sd):
        if ".m." in k and k.endswith(".weight"):
            w = sd[k].clone().view(na, no, -1)
            w[:, 4] *= gain
            sd[k] = w.view(na * no, -1, 1, 1)
    det = model.Detector(arch.ARCHS[args.arch](nc), sd, img_size=(H, W), max_batch=n_frames)
    fr = torch.from_numpy(fh).cuda()
    det.plant_objectness_bias(fr, 2000, level_quota=quota)
    count0 = BaseTrack._count
    BaseTrack._count = 0
    trk = ByteTrack(_types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="default", img_size=args.img, iou_thresh=0.5, max_tracks=1024, max_dets=1024))
    head = det.forward(fr, fuse_decode=0.01)            # conf_thres of post_process_v7 (tracker/track.py:239)
    outs = cli.post_process_v7(head, img_size=(H, W), ori_img_size=(H, W, 3), all_images=True)
    handed, dev = [], []
    for k in range(n_frames):
        handed.append(outs[k].detach().cpu().numpy().copy())
        dev.append([(t.track_id, np.asarray(t.tlwh, np.float64), float(t.cls), float(t.score)) for t in trk.update(outs[k], None)])
    BaseTrack._count = count0
    seam = chained.track("bytetrack", handed)
    seam_ok = len(seam) == len(dev) and all(
        [a[0] for a in fa] == [b[0] for b in fb] and all(a[2] == b[2] and np.allclose(a[1], b[1], rtol=1e-6, atol=1e-5) for a, b in zip(fa, fb)) for fa, fb in zip(dev, seam))
    ora = chained.oracle_detections(det.nodes, det._sd, det.spec["anchors"], fh, chunk=4)
    diff = [chained.detection_set_difference(a, b) for a, b in zip(ora, handed)]
    ora_tracks = chained.track("bytetrack", ora)
    with tempfile.TemporaryDirectory() as tmp:
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):      # (the harness prints its tables; the bench prints ONE line)
            g = chained.grade(tmp, ora_tracks, dev)
    return {"frames": n_frames, "checker": "oracle/chained.py: fp32 oracle network -> NMS -> scale_coords/round -> numpy ByteTrack; graded by yolov7-tracker_amd/tracker/trackeval",
            "seam_device_tracker_equals_oracle_tracker_on_the_devices_handover": bool(seam_ok),
            "handover_rows_per_frame_mean": round(float(np.mean([len(h) for h in handed])), 1),
            "handover_rows_without_partner_at_8a_bar": {"oracle_only": int(sum(len(a) for a, _ in diff)), "device_only": int(sum(len(b) for _, b in diff))},
            "frames_with_identical_handover": int(sum(chained.same_detections(a, b) for a, b in zip(ora, handed))),
            "track_rows": {"device": int(sum(len(f) for f in dev)), "oracle": int(sum(len(f) for f in ora_tracks))},
            "device_chain_graded_against_oracle_chain": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in g.items()},
            "objectness_gain": gain, "level_quota": list(quota)}


def other_workloads(args):
    """configs[2] (BoT-SORT, 500 objects) and configs[3] (DeepSORT + OSNet ReID) in the driver's default run -- two short runs of this script
    (--steps 16, no CPU baseline, no latency mode) as child processes AFTER the headline's timed region, their lines reduced to the figures that matter.
    (Round 6: 16 steps instead of 5 -- the timed region ends when the LAST batch's tracker chain has drained, one chain of ~35-54 ms behind the last forward; over five steps
    of 35 ms that tail was a fifth of the quoted time per step: cfg3 41-43 ms per step with a 35 ms list AND a 35 ms chain, kernel trace in profiles/r06_batch_80.txt.)"""
    import subprocess
    out = {}
    for wl in ("cfg3", "cfg4"):
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--workload", wl, "--steps", "16", "--warmup", "3", "--no_cpu_baseline", "--no_latency_mode",
               "--no_other_workloads", "--full", "--batch", str(args.batch), "--img", str(args.img), "--arch", args.arch]
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
            l = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            ph = l.get("phases_ms_per_step", {})
            o = {"workload": l["config"]["workload"].split(",")[0], "fps": l["value"], "ms_per_step": l["ms_per_step"], "steps": l["steps"],
                 "launch_list_ms": l["roofline"].get("launch_list_ms"), "tracker_chain_ms": ph.get("tracker_chain"),
                 "tracks_alive_last_frame": l["config"].get("tracks_alive_last_frame"), "dets_per_frame": l["config"].get("dets_per_frame_timed_mean")}
            if wl == "cfg4":
                o["reid_ms"] = ph.get("reid")
                o["reid_crops_per_step"] = l["config"].get("reid_crops_per_step_mean")
                o["roofline_reid"] = {k: l.get("roofline_reid", {}).get(k) for k in ("achieved", "peak", "unit", "frac", "bound")}
            out[wl] = o
        except Exception as e:      # a failed child must not take the headline line with it
            out[wl] = {"error": repr(e)[:300]}
    out["note"] = "short child runs of this script (--workload cfg3 / cfg4 --steps 5) behind the headline's timed region; never part of `value`"
    return out


def latency_mode(args, nc, frames_host, dets_seq, n_timed=60, n_warm=10, sd=None):
    """Reference `Timer` semantics (tracker/track.py:140-181, tracker/timer.py): batch 1, wall time from "frame tensor on the HOST" (the
    loader's float32 RGB CHW tensor, tracker_dataloader.py:83-88) to "track list produced" (tracker.update returned, rows copied back,
    device idle), one frame at a time, H2D copy inside the timer.  Also with the raw uint8 frame as the host input (device pre-processing).
    -> dict for the JSON line."""
    from yolov7_tracker_amd.detector import arch, model
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.bytetrack import ByteTrack
    H = W = args.img
    det1 = model.Detector(arch.ARCHS[args.arch](nc), sd, img_size=(H, W), max_batch=1, seed=0)      # the timed run's weights (before its objectness shift)
    nf = min(8, len(frames_host))
    u8 = [torch.from_numpy(frames_host[i]).pin_memory() for i in range(nf)]
    f32 = [(torch.from_numpy(np.ascontiguousarray(frames_host[i][:, :, ::-1].transpose(2, 0, 1))).float() / 255.0).pin_memory() for i in range(nf)]
    plant_objectness_bias(det1, u8[0][None].cuda())
    res = {}
    count0 = BaseTrack._count
    for mode, src in (("f32_chw_host", f32), ("u8_hwc_host", u8)):
        # the frame's detector + decode/NMS chain is ONE hipGraph replay on a fixed device input buffer (189 launches per frame at batch 1: host launch cost
        # is a tenth of the frame; measured 259 -> 280 fps, profiles/r03_conv_variants.txt); the H2D copy and the tracker step are enqueued around it
        dev_in = torch.empty((1,) + tuple(src[0].shape), dtype=src[0].dtype, device="cuda")
        dev_in.copy_(src[0][None])
        graph, _, _ = det1.capture(dev_in, 0.01, 0.45, None)
        trk = ByteTrack(make_opts(), frame_rate=30)
        tot = 0.0
        for i in range(n_warm + n_timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()                                   # timer.tic()
            dev_in.copy_(src[i % nf][None], non_blocking=True)          # model(img.to(device)): H2D inside the timer
            graph.replay()                                              # forward + non_max_suppression + scale_coords + round
            cur = trk.update(dets_seq[i], None)                         # tracker.update: rows come back to the host (syncs)
            _ = [c.tlwh for c in cur]
            torch.cuda.synchronize()
            if i >= n_warm:
                tot += time.perf_counter() - t0                         # timer.toc()
        res[mode] = {"fps": round(n_timed / tot, 1), "ms_per_frame": round(tot / n_timed * 1e3, 3)}
    BaseTrack._count = count0
    res["note"] = ("batch 1, reference Timer semantics: host frame in -> track list out, H2D inside the timer, device sync every frame, detector + NMS as a hipGraph replay; "
                   "%d timed frames after %d warm-up" % (n_timed, n_warm))
    return res


def frames_mode(args, dist, world, rank, backend, det, frames, dets_dev, trk, results):
    """single-stream mode: batch s of the ONE sequence is detected (forward + decode/NMS) by rank s % world; its detections go to
    rank 0 with one point-to-point message (sharding.DetectionRelay); rank 0 runs every tracker frame step, in order.
    Returns (seconds for the K timed batches, forward ms list of this rank's timed batches)."""
    from yolov7_tracker_amd import sharding
    from yolov7_tracker_amd.detector.model import MAX_DET
    B, K, Wm = args.batch, args.steps, args.warmup
    on_gpu = backend == "nccl"
    relay = sharding.DetectionRelay(B, MAX_DET, device="cuda" if on_gpu else "cpu")
    sA, sB, sC, sD = (torch.cuda.Stream() for _ in range(4))
    ev = {}
    fwd_ms_ev = []

    own = []              # steps this rank detected (candidate set k % 2 is reused every second own batch)

    def detect(s, timed):
        k = len(own)
        with torch.cuda.stream(sA):
            e0, e1, est = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
            if k >= 2:
                sA.wait_event(ev[own[k - 2]])            # the NMS that last read candidate set k % 2 is through
            e0.record(sA)
            out = det.forward(frames, fuse_decode=0.01, pset=k % 2)     # Detect epilogues decode + filter into candidate set k % 2
            e1.record(sA)
            if timed:
                fwd_ms_ev.append((e0, e1))
            est.record(sA)
        with torch.cuda.stream(sC):
            sC.wait_event(est)
            dets, nd = det.postprocess(out, 0.01, 0.45, None)
            if rank != 0:
                if on_gpu:
                    relay.send(dets, nd)                  # RCCL send, ordered behind the NMS on this stream
                else:
                    relay.send(dets.cpu(), nd.cpu())      # gloo smoke path
            ev[s] = torch.cuda.Event()
            ev[s].record(sC)
        own.append(s)

    def run(lo, hi, timed):
        for s in range(lo, hi):
            owner = sharding.batch_owner(s, world)
            if owner == rank:
                detect(s, timed)
            if rank == 0:
                if owner != 0:
                    with torch.cuda.stream(sD):
                        relay.recv(owner)                 # (B, 300, 6) + counts; the tracker below consumes the scene's detections
                        ev[s] = torch.cuda.Event()
                        ev[s].record(sD)
                with torch.cuda.stream(sB):
                    sB.wait_event(ev[s])
                    for i in range(B):
                        trk._launch(dets_dev[s * B + i], out=results[s * B + i])

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    run(0, Wm, False)
    barrier()
    t0 = time.perf_counter()
    run(Wm, Wm + K, True)
    barrier()
    dt_s = time.perf_counter() - t0
    return dt_s, [a.elapsed_time(b) for a, b in fwd_ms_ev]


def halves_mode(args, det_factory, frames, dets_dev, trk, results, plant):
    """experiment (--halves 2): every step's B frames as two B/2-frame forwards on two streams with two detectors; a forward enters
    its memory-bound high-resolution ops only when the other one has left them, so byte-bound and MFMA-bound layers of the two
    halves overlap.  Same decode/NMS gating and tracker ordering as the default pipeline.  -> (seconds, forward spans in ms)"""
    B, K, Wm = args.batch, args.steps, args.warmup
    Bh = B // 2
    dets = [det_factory(Bh), det_factory(Bh)]
    for d in dets:
        plant(d, frames[:Bh])
    sAs = [torch.cuda.Stream(), torch.cuda.Stream()]
    sB, sC = (torch.cuda.Stream(priority=-1) if args.prio == 2 else torch.cuda.Stream()), torch.cuda.Stream()
    n = (K + Wm) * 2
    ev_mid = [torch.cuda.Event() for _ in range(n)]
    ev_staged = [torch.cuda.Event() for _ in range(n)]
    ev_nms = [torch.cuda.Event() for _ in range(n)]
    ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    k_mid = next((i for i, op in enumerate(dets[0].plan.ops) if int(op["H"]) <= args.img // 8), 0)
    pending = []

    def finish(prev, gate):
        m, staged = prev
        with torch.cuda.stream(sC):
            sC.wait_event(ev_staged[m])
            if gate is not None:
                sC.wait_event(gate)
            dets[m % 2].postprocess(staged, 0.01, 0.45, None)
            ev_nms[m].record(sC)
        with torch.cuda.stream(sB):
            sB.wait_event(ev_nms[m])
            for i in range(Bh):
                trk._launch(dets_dev[m * Bh + i], out=results[m * Bh + i])

    def mini(m):
        d, sA = dets[m % 2], sAs[m % 2]
        fr = frames[(m % 2) * Bh:(m % 2 + 1) * Bh]
        with torch.cuda.stream(sA):
            if m > 0:
                sA.wait_event(ev_mid[m - 1])           # the other half has left its high-resolution layers
            ev0[m].record(sA)
            out = d.forward(fr, mid_hook=(k_mid, lambda: ev_mid[m].record(sA)))
            ev1[m].record(sA)
        if pending:
            finish(pending.pop(0), ev_mid[m])
        with torch.cuda.stream(sA):
            if m > 1:
                sA.wait_event(ev_nms[m - 2])           # this detector's staging set is free again
            staged = d.stage_heads(out)
            ev_staged[m].record(sA)
        pending.append((m, staged))

    def run(lo, hi):
        for m in range(lo, hi):
            mini(m)
        while pending:
            finish(pending.pop(0), None)
        torch.cuda.synchronize()

    run(0, Wm * 2)
    t0 = time.perf_counter()
    run(Wm * 2, n)
    dt_s = time.perf_counter() - t0
    for d in dets:
        d.check_overflow()
    span = ev0[Wm * 2].elapsed_time(ev1[n - 1])        # first timed forward start -> last forward end (they overlap)
    return dt_s, span / K, dets[0]


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launcher_command(argv, n):
    """the command `python bench.py --gpus N ...` re-executes itself as when it was started WITHOUT a launcher (no WORLD_SIZE in the environment):
    one rank per GPU under torch.distributed.run, exactly the driver's own command line (rendezvous on 127.0.0.1: the hostname may not resolve)"""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
            "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)


def self_launch(args):
    """--gpus N > 1 without a launcher: start the N ranks ourselves and pass their output through (rank 0 prints the ONE JSON line).
    Fewer than N devices is an error, never a silent n_gpus = 1 line."""
    import subprocess
    share = os.environ.get("Y7T_BENCH_SHARE_GPU") == "1"
    if os.environ.get("Y7T_BENCH_DRYRUN_LAUNCH") == "1":      # (tests/test_bench_contract.py: the command, without starting it)
        print(json.dumps({"launch": launcher_command(sys.argv[1:], args.gpus)}))
        return 0
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have == 0:
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    if have < args.gpus and not share:
        raise SystemExit("bench.py --gpus %d: only %d device%s visible on this node (one rank per GPU; Y7T_BENCH_SHARE_GPU=1 with "
                         "Y7T_BENCH_BACKEND=gloo is the 1-GPU plumbing test, not a measurement)" % (args.gpus, have, "" if have == 1 else "s"))
    cmd = launcher_command(sys.argv[1:], args.gpus)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def main():
    global TRACKER_THREADS
    args = parse()
    TRACKER_THREADS = args.tracker_threads
    launched = args.launched
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if not launched:
        os.environ.pop("WORLD_SIZE", None)
        if args.gpus > 1:
            sys.exit(self_launch(args))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit("bench.py --gpus %d was started under a launcher with WORLD_SIZE=%s: the two must agree (one rank per GPU)"
                         % (args.gpus, os.environ.get("WORLD_SIZE")))
    cfg3, cfg4 = args.workload == "cfg3", args.workload == "cfg4"
    if args.n_obj is None:
        args.n_obj = 500 if cfg3 else 80
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    share = os.environ.get("Y7T_BENCH_SHARE_GPU") == "1"     # smoke-test the N>1 code path on a 1-GPU box (with the gloo backend)
    backend = os.environ.get("Y7T_BENCH_BACKEND", "nccl")    # 'nccl' == RCCL on ROCm
    if not share and local >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d (LOCAL_RANK %d) has no device of its own: %d visible, one rank per GPU" % (rank, local, torch.cuda.device_count()))
    torch.cuda.set_device(0 if share else local)
    dist = None
    cdev = "cuda" if backend == "nccl" else "cpu"            # where the (tiny) collective payloads live
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.detector import arch, model
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.bytetrack import ByteTrack

    B, K, Wm = args.batch, args.steps, args.warmup
    H = W = args.img
    nc = 10
    n_frames = (K + Wm) * B
    seq = 0 if args.mode == "frames" else rank                                # single-stream mode: every rank sees the same sequence
    frames_host = synth.make_frames(B, args.n_obj, H, seq_idx=seq)           # B distinct frames, reused every step
    conditioned = args.weights == "conditioned"
    sd0 = conditioned_state_dict(args, nc, frames_host) if conditioned else None
    det = model.Detector(arch.ARCHS[args.arch](nc), sd0, img_size=(H, W), max_batch=B, seed=0)
    frames = torch.from_numpy(frames_host).cuda()
    extra_passes = args.full and world == 1 and args.mode == "sequences" and args.halves == 1
    coupled_pass = extra_passes and not cfg3 and not cfg4 and max(1, args.seqs) == 1 and args.tracker_launch == "frames" and args.hipgraph == 0 and not args.no_coupled
    n_frames *= 2 if extra_passes else 1   # second pass: the same pipeline fed from host memory (a third, `coupled`, has its own tracker and result rows)
    S = max(1, args.seqs)
    if B % S:
        raise SystemExit("--seqs must divide --batch")
    Bq = B // S                                                               # frames of one sequence per step
    per_seq = [synth.make_detections(n_frames // S, args.n_obj, H, seq_idx=seq * S + q, bounce=True) for q in range(S)]   # each scene's detections, frame by frame
    # frame slot i of step s belongs to sequence i // Bq, at its local time s * Bq + i % Bq; everything below is indexed by t = s * B + i
    dets_seq = [per_seq[(t % B) // Bq][(t // B) * Bq + (t % B) % Bq] for t in range(n_frames)]
    dets_dev = [torch.from_numpy(d).cuda() for d in dets_seq]
    plant_objectness_bias(det, frames)       # ~2000 candidates per frame, every Detect level supplying its quota: all four are live

    BaseTrack._count = 0
    if cfg3:
        from yolov7_tracker_amd.tracker.botsort import BoTSORT
        o3 = make_opts()
        o3.kalman_format, o3.max_tracks, o3.max_dets = "botsort", 2048, 1024
        trks = [BoTSORT(o3, frame_rate=30) for _ in range(S)]
        wq = [synth.make_warps(n_frames // S, seq_idx=seq * S + q).reshape(-1, 6) for q in range(S)]            # what GMC.apply would estimate (botsort.py:13-248)
        warps_dev = torch.from_numpy(np.stack([wq[(t % B) // Bq][(t // B) * Bq + (t % B) % Bq] for t in range(n_frames)])).cuda()
    elif cfg4:
        # BASELINE configs[3]: DeepSORT, appearance features from OSNet x0_25 over 128 x 64 crops of every detection, taken from the frames in HBM
        from yolov7_tracker_amd.tracker.deepsort import DeepSORT
        from yolov7_tracker_amd.tracker.reid import ReIDExtractor
        reid = ReIDExtractor(None, max_crops=B * 2 * args.n_obj + 64, seed=0)
        trks = [DeepSORT(make_opts(), frame_rate=30, reid_model=reid) for _ in range(S)]
        step_boxes, step_idx, step_off = [], [], []       # per step: the boxes of its B frames' detections, their frame index, row ranges
        for s0 in range(0, n_frames, B):
            ns = [len(dets_seq[t]) for t in range(s0, s0 + B)]
            step_boxes.append(torch.cat([dets_dev[t][:, :4] for t in range(s0, s0 + B)]).contiguous())
            step_idx.append(torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), ns)).cuda())
            step_off.append(np.concatenate([[0], np.cumsum(ns)]).astype(np.int64))
    else:
        trks = [ByteTrack(make_opts(), frame_rate=30) for _ in range(S)]
    trk = trks[0]
    results = torch.zeros((n_frames, trk.cap_t + 1, 8), dtype=torch.float64, device="cuda")
    ev_reid = {}
    seq_streams = [torch.cuda.Stream() for _ in range(S - 1)]      # sequence 0 steps on the caller's stream, the others beside it
    def launch_step(s):
        """the tracker frame steps of batch s: every sequence's frames in order on that sequence's stream (BoT-SORT: with each frame's
        camera-motion warp; DeepSORT: after ONE ReID pass over all detections of the batch's frames)"""
        cur = torch.cuda.current_stream()
        if cfg4:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            feats = reid.features_for_frames(frames, step_boxes[s], step_idx[s])
            e1.record()
            ev_reid[s] = (e0, e1)
            off = step_off[s]
        fork = torch.cuda.Event()
        fork.record(cur)
        for q in range(S):
            st = cur if q == 0 else seq_streams[q - 1]
            with torch.cuda.stream(st):
                if q:
                    st.wait_event(fork)
                if s in coupled_tables:                                # coupled passes: the rows and the row counts y7t_det_postprocess left for this step's frames
                    cv = coupled_tables[s]
                    if cv["gain"] != 1.0:
                        det.plan.post[s % 2].dets[:B, :, 4].mul_(cv["gain"])      # (the score gain of the second coupled pass, see below)
                    cv["trk"]._launch_frames(cv["tables"][s])
                    continue_frames = False
                elif args.tracker_launch == "frames" and not cfg4:      # one launch for the sequence's frames of this step (pointer tables built before the timed region)
                    trks[q]._launch_frames(frame_tables[(s, q)])
                    continue_frames = False
                else:
                    continue_frames = True
                for i in (range(q * Bq, (q + 1) * Bq) if continue_frames else ()):
                    t = s * B + i
                    if cfg3:
                        trks[q]._launch(dets_dev[t], out=results[t], warp=warps_dev[t])
                    elif cfg4:
                        trks[q]._launch(dets_dev[t], feats[int(off[i]):int(off[i + 1])], out=results[t])
                    else:
                        trks[q]._launch(dets_dev[t], out=results[t])
                if q:
                    j = torch.cuda.Event()
                    j.record(st)
                    cur.wait_event(j)          # join: the step's chain is complete on the caller's stream
    frame_tables = {}
    coupled_tables, coupled_variants = {}, []      # step -> variant; filled below, once the post-processing sets exist
    if args.tracker_launch == "frames" and not cfg4:
        for s_ in range(n_frames // B):
            for q in range(S):
                ts = [s_ * B + i for i in range(q * Bq, (q + 1) * Bq)]
                frame_tables[(s_, q)] = trks[q].frames_table([dets_dev[t] for t in ts], [results[t] for t in ts], [warps_dev[t] for t in ts] if cfg3 else None)
    tracker_name = "botsort" if cfg3 else "deepsort" if cfg4 else "bytetrack"
    metric_name = "end-to-end fps (detect+track) YOLOv7-w6@1280 " + ("BoT-SORT, 500-object stress" if cfg3 else
                                                                     "DeepSORT + OSNet x0_25 ReID (128x64 crops)" if cfg4 else "ByteTrack")
    if args.dump_outputs and (args.mode == "frames" or (args.halves == 2 and world == 1)):
        raise SystemExit("--dump-outputs: the default pipeline only (--mode sequences --halves 1)")
    if args.halves == 2 and world == 1:
        dt_s, fwd_ms_step, d0 = halves_mode(args, lambda b: model.Detector(arch.ARCHS[args.arch](nc), None, img_size=(H, W), max_batch=b, seed=0),
                                           frames, dets_dev, trk, results, plant_objectness_bias)
        tf = d0.gflop_per_frame * B / (fwd_ms_step * 1e-3) / 1e3
        print(json.dumps({"metric": "end-to-end fps (detect+track) YOLOv7-w6@1280 ByteTrack", "value": round(K * B / dt_s, 2), "unit": "frames/s",
                          "n_gpus": 1, "steps": K, "warmup": Wm, "ms_per_step": round(dt_s / K * 1e3, 3), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "f16", "data": "synthetic",
                          "config": {"workload": "configs[1], two interleaved half-batch forwards per step (experiment)", "frames_per_step": B},
                          "roofline": {"bound": "mfma", "achieved": round(tf, 2), "peak": PEAK_MFMA_F16 / 1e12, "unit": "TFLOP/s",
                                       "frac": round(tf * 1e12 / PEAK_MFMA_F16, 4), "traffic": None,
                                       "note": "forward span of a step (two overlapping launch lists) = %.3f ms" % fwd_ms_step}, "cpu_baseline": None}))
        return
    if args.mode == "frames":
        dt_s, fwd_ms = frames_mode(args, dist, world, rank, backend, det, frames, dets_dev, trk, results)
        if dist is not None:
            tmax = torch.tensor([dt_s], dtype=torch.float64, device=cdev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt_s = float(tmax.item())
        torch.cuda.synchronize()
        det.check_overflow()
        if rank == 0:
            last = results[(Wm + K) * B - 1].cpu().numpy()
            conv_tflops = det.gflop_per_frame * B / (np.mean(fwd_ms) * 1e-3) / 1e3 if fwd_ms else None
            print(json.dumps({
                "metric": "end-to-end fps (detect+track) YOLOv7-w6@1280 ByteTrack", "value": round(K * B / dt_s, 2), "unit": "frames/s",
                "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": round(dt_s / K * 1e3, 3), "higher_is_better": True,
                "scaling": "strong", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
                "config": {"workload": "configs[1], single-stream mode: ONE synthetic VisDrone-shape sequence, YOLOv7-w6 1280x1280 + ByteTrack",
                           "frames_per_step": B, "arch": args.arch, "nc": nc, "tracker": "bytetrack",
                           "tracks_alive_last_frame": int(last[trk.cap_t].view(np.int32)[0]),
                           "parallelism": "detector frame-sharded x%d (batch s on rank s %% N), detections sent to the tracker on rank 0" % world,
                           "collective_backend": backend if world > 1 else None},
                "roofline": {"bound": "mfma", "achieved": None if conv_tflops is None else round(conv_tflops, 2), "peak": PEAK_MFMA_F16 / 1e12,
                             "unit": "TFLOP/s", "frac": None if conv_tflops is None else round(conv_tflops * 1e12 / PEAK_MFMA_F16, 4), "traffic": None},
                "cpu_baseline": None}))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    # the forward's stream gets the high hardware priority: its workgroups are dispatched ahead of the NMS / tracker kernels that run beside it
    sA = torch.cuda.Stream(priority=-1) if args.prio == 1 else torch.cuda.Stream()
    sB, sC, sH = (torch.cuda.Stream(priority=-1) if args.prio == 2 else torch.cuda.Stream()), torch.cuda.Stream(), torch.cuda.Stream()
    if args.cu_reserve > 0:    # the tracker chain on compute units of its own (include/y7t.h: y7t_stream_create_cu_mask)
        from yolov7_tracker_amd import _lib as _y7t_lib
        sA, sB = _y7t_lib.cu_masked_streams(args.cu_reserve)
        sC = sB if args.cu_reserve_nms else sA      # NMS on the reserved CUs beside the tracker chain, or on the detector's share (an unmasked stream would be free to use the reserved CUs)
    NS = 4 * (K + Wm)                  # pass 0: frames resident in HBM (`value`); pass 1 (N=1 only): the same pipeline fed from pinned host memory; passes 2, 3 (N=1, configs[1]): coupled
    ev_staged = [torch.cuda.Event() for _ in range(NS)]
    ev_fwd0 = [torch.cuda.Event(enable_timing=True) for _ in range(NS)]
    ev_fwd1 = [torch.cuda.Event(enable_timing=True) for _ in range(NS)]
    ev_nms = [torch.cuda.Event(enable_timing=True) for _ in range(NS)]
    ev_h2d = [torch.cuda.Event() for _ in range(NS)]
    ev_trk0 = [torch.cuda.Event(enable_timing=True) for _ in range(NS)]
    ev_trk1 = [torch.cuda.Event(enable_timing=True) for _ in range(NS)]

    CONF = 0.01                 # tracker/track.py:239
    graph = None
    if args.hipgraph == 1:
        with torch.cuda.stream(sA):
            graph, g_dets, g_nd = det.capture(frames, CONF, 0.45, None)

    # ops of the launch list that run on the 640^2 / 320^2 maps: memory-bound; the previous batch's decode+NMS (memory-bound too)
    # is held back until the forward is past them (an event recorded between two pieces of the list)
    k_mid = next((i for i, op in enumerate(det.plan.ops) if int(op["H"]) <= H // args.nms_gate_div), 0)
    ev_mid = [torch.cuda.Event() for _ in range(NS)]
    pending = []          # (step, staged heads) whose decode+NMS and tracker steps are not enqueued yet
    post_of = {}          # step -> (dets, ndets) its decode + NMS wrote
    fwd_graphs = fwd_out = None
    if args.hipgraph == 2:    # the same launch list, captured in two pieces around the gate event, once per candidate set
        fwd_graphs, fwd_out = [], []
        with torch.cuda.stream(sA):
            for ps_i in range(2):
                fwd_out.append(det.forward(frames, fuse_decode=CONF, pset=ps_i))   # warm-up: plan selection, kernel attributes
                torch.cuda.synchronize()
                g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(g1, stream=sA):
                    det.forward_part(frames, 0, k_mid, fuse_decode=CONF, pset=ps_i)
                with torch.cuda.graph(g2, stream=sA):
                    det.forward_part(None, k_mid, -1, fuse_decode=CONF, pset=ps_i)
                fwd_graphs.append((g1, g2))
    host_feed = None      # pass 1: (pinned host batch, two device batches)
    # the timed steps do not re-read ONE resident batch (157 MB of uint8 < the 256 MB Infinity Cache: the stem's reads could be cache hits).
    # N_ROT distinct batches (the scene's frames shifted in time and space: other bytes at other addresses, 4 x 157 MB = 629 MB) are consumed round-robin.
    N_ROT = max(1, args.rotate_batches) if (graph is None and fwd_graphs is None) else 1
    frames_rot = [frames] + [torch.roll(frames, shifts=(5 * k, 96 * k, 160 * k), dims=(0, 1, 2)).contiguous() for k in range(1, N_ROT)]
    # the reference's timer stops when tracker.update has returned HOST objects (tracker/track.py:151-174): every step's result rows are copied
    # to pinned host memory inside the timed region (own stream, behind the step's tracker chain, two buffers)
    sD = torch.cuda.Stream()
    host_rows = [torch.empty((B,) + tuple(results.shape[1:]), dtype=results.dtype).pin_memory() for _ in range(2)]
    ev_d2h = [torch.cuda.Event() for _ in range(NS)]

    if coupled_pass:      # the device NMS output feeding the device tracker inside the timed pipeline: a fresh ByteTrack, one launch per step
        # Two passes.  `coupled`: the step's (300, 6) NMS rows and row counts as they are -- with random weights 0.4 of a frame's 300 rows reach ByteTrack's 0.2 and none
        # its birth gate of 0.3, so the tracker reads, gathers and thresholds 300 rows per frame and tracks nothing: the cost of the DATA PATH.  `coupled_confident_rows`:
        # the hand-over multiplies the rows' score column by one constant (a strided in-place multiply on the tracker's stream, in front of the launch) chosen so that
        # every frame's n_obj-th best row sits at det_thresh: as many rows per frame above the threshold as the headline's scene has detections, and the rows behind
        # them in the low-score association.  The detector, the candidates and the NMS are the headline's in both; the boxes are a random head's (up to 1000+ px, heavily
        # overlapping), so the second pass is an ill-posed association, not a scene.
        with torch.cuda.stream(sA):
            d_, n_ = det.postprocess(det.forward(frames, fuse_decode=CONF), CONF, 0.45, None)
        torch.cuda.synchronize()
        sc_ = d_[:B, :, 4].clone()
        sc_[torch.arange(sc_.shape[1], device=sc_.device)[None, :] >= n_[:B, None]] = -1.0
        kth = torch.sort(sc_, dim=1, descending=True).values[:, min(args.n_obj, sc_.shape[1]) - 1]
        gain2 = (make_opts().conf_thresh + 1e-4) / float(torch.median(kth[kth > 0]).item()) if bool((kth > 0).any()) else 1.0
        for vi, (vname, vgain) in enumerate((("coupled", 1.0), ("coupled_confident_rows", gain2))):
            oc = make_opts()
            oc.max_tracks = 2048      # (a random head's boxes: more births and lost tracks than a scene's)
            tc = ByteTrack(oc, frame_rate=30)
            # (its own result rows: the pool is twice as large as the headline tracker's, and a tracker writes `cap_t` rows + the count per frame)
            rc_ = torch.zeros(((K + Wm) * B, tc.cap_t + 1, 8), dtype=torch.float64, device="cuda")
            cv = {"name": vname, "gain": vgain, "trk": tc, "results": rc_, "first": (2 + vi) * (K + Wm), "tables": {},
                  "host_rows": [torch.empty((B,) + tuple(rc_.shape[1:]), dtype=rc_.dtype).pin_memory() for _ in range(2)]}
            for s_ in range(cv["first"], cv["first"] + K + Wm):
                pp = det.plan.post[s_ % 2]
                f0 = (s_ - cv["first"]) * B
                cv["tables"][s_] = tc.frames_table([pp.dets[i] for i in range(B)], [rc_[f0 + i] for i in range(B)], None, counts_dev=pp.ndets)
                coupled_tables[s_] = cv
            coupled_variants.append(cv)

    def finish(prev, gate):
        """rank sort + NMS of batch `prev` on stream C (after `gate`, if any), then its tracker frame steps on stream B"""
        ps, out = prev
        with torch.cuda.stream(sC):
            sC.wait_event(ev_staged[ps])
            if ps in coupled_tables and (ps - 2) in coupled_tables:
                sC.wait_event(ev_trk1[ps - 2])     # coupled pass: this NMS rewrites the rows the tracker steps of batch ps - 2 read
            if gate is not None:
                sC.wait_event(gate)
            post_of[ps] = det.postprocess(out, CONF, 0.45, None)
            ev_nms[ps].record(sC)
        with torch.cuda.stream(sB):
            sB.wait_event(ev_nms[ps])      # a frame's detections exist before its tracker step runs
            ev_trk0[ps].record(sB)
            launch_step(ps)
            ev_trk1[ps].record(sB)
        with torch.cuda.stream(sD):            # the step's track rows -> host
            sD.wait_event(ev_trk1[ps])
            if ps >= 2:
                sD.wait_event(ev_d2h[ps - 2])
            if ps in coupled_tables:
                cv = coupled_tables[ps]
                f0 = (ps - cv["first"]) * B
                cv["host_rows"][ps % 2].copy_(cv["results"][f0:f0 + B], non_blocking=True)
            else:
                host_rows[ps % 2].copy_(results[ps * B:(ps + 1) * B], non_blocking=True)
            ev_d2h[ps].record(sD)

    def step(s):
        if graph is not None:
            with torch.cuda.stream(sA):
                ev_fwd0[s].record(sA)
                graph.replay()                 # input layout + conv launches + pools + decode/NMS as one hipGraph
                post_of[s] = (g_dets, g_nd)
                ev_fwd1[s].record(sA)
                ev_nms[s].record(sA)
            with torch.cuda.stream(sB):
                sB.wait_event(ev_nms[s])
                ev_trk0[s].record(sB)
                launch_step(s)
                ev_trk1[s].record(sB)
            return
        src = frames_rot[s % N_ROT]
        if host_feed is not None:              # this batch comes over PCIe: copy on its own stream into the buffer the forward two steps back used
            src = host_feed[1][s % 2]
            with torch.cuda.stream(sH):
                if s >= 2:
                    sH.wait_event(ev_fwd1[s - 2])
                src.copy_(host_feed[0], non_blocking=True)
                ev_h2d[s].record(sH)
        with torch.cuda.stream(sA):
            if host_feed is not None:
                sA.wait_event(ev_h2d[s])
            if s >= 2:
                sA.wait_event(ev_nms[s - 2])   # the Detect epilogues of this forward refill candidate set s % 2: its last NMS must be through
            ev_fwd0[s].record(sA)
            if fwd_graphs is not None and host_feed is None:
                fwd_graphs[s % 2][0].replay()
                ev_mid[s].record(sA)
                fwd_graphs[s % 2][1].replay()
                out = fwd_out[s % 2]
            else:
                out = det.forward(src, mid_hook=(k_mid, lambda: ev_mid[s].record(sA)), fuse_decode=CONF, pset=s % 2)
            ev_fwd1[s].record(sA)
            ev_staged[s].record(sA)            # the candidates of batch s are in set s % 2
        if pending:                            # the previous batch: NMS starts once this forward has left the big maps
            finish(pending.pop(), ev_mid[s])
        pending.append((s, out))

    def flush():
        while pending:
            finish(pending.pop(), None)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_pass(first):
        for s in range(first, first + Wm):
            step(s)
        flush()
        barrier()
        t0 = time.perf_counter()
        for s in range(first + Wm, first + Wm + K):
            step(s)
        flush()
        barrier()
        return time.perf_counter() - t0

    dt_s = timed_pass(0)
    if args.dump_outputs and rank == 0:
        s_last = Wm + K - 1
        dump_outputs(args.dump_outputs, *post_of[s_last], results[s_last * B:(s_last + 1) * B], trk.cap_t)
    dt_h2d = None
    second_pass = extra_passes and graph is None
    dt_coupled = {}
    if second_pass:       # PCIe-inclusive rate: never `value`, reported beside it
        host_feed = (torch.from_numpy(frames_host).pin_memory(), [torch.empty_like(frames), torch.empty_like(frames)])
        dt_h2d = timed_pass(K + Wm)
        for cv in coupled_variants:  # ... and with it the coupled chain: host-fed frames -> forward -> NMS -> the tracker steps on that NMS's rows -> track rows on the host
            dt_coupled[cv["name"]] = timed_pass(cv["first"])
        host_feed = None
    if dist is not None:
        tmax = torch.tensor([dt_s], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt_s = float(tmax.item())
        # result gather (the only collective, after the timed steps): sharding.rebase_and_gather -- the code the world-size-2 gloo test proves -- does the id
        # re-basing (per-rank id counts -> exclusive prefix: the ids of a single-process run with the reference's global BaseTrack._count) and ONE
        # gather of compact 28-byte rows (frame, id, x, y, w, h, cls) to rank 0.  Each rank's sequences travel as one block keyed by its rank.
        from yolov7_tracker_amd import sharding as _sh
        live = results[:, :trk.cap_t, 0] > 0                  # row cap_t of every frame holds the row count, not a track
        fi, ri = torch.nonzero(live, as_tuple=True)
        rr = results[fi, ri]                                  # (n, 8) [id, x, y, w, h, cls, score, slot]
        rows = torch.cat([(fi + 1).to(torch.float64)[:, None], rr[:, :6]], 1)      # [frame (1-based, in this rank's frame order), id (local), x, y, w, h, cls]
        rows = rows if cdev == "cuda" else rows.cpu()
        gathered = _sh.rebase_and_gather({rank: rows}, {rank: int(BaseTrack._count)}, world, device=cdev)
        if rank == 0:
            st = dict(_sh.last_gather_stats)
            # what a >= 2-GPU lease has to show without a code change: the backend torch.distributed reports, the ranks it saw, and a digest of
            # the GLOBAL ids per rank block (sum of frame x id over the gathered rows) that tests/test_multirank_gpu.py recomputes from a single-process run
            gathered_info = {"backend_reported": dist.get_backend(), "ranks_seen": dist.get_world_size(),
                             "rows_per_rank": st["rows_per_rank"], "bytes_per_row": st["bytes_per_row"], "payload_bytes_per_rank": st["payload_bytes_per_rank"],
                             "id_base_per_rank": st["id_offset_per_seq"],
                             "frame_x_id_digest_per_rank": [int((g_[:, 0] * g_[:, 1]).sum().item()) for g_ in gathered],
                             "distinct_ids_per_rank": [int(torch.unique(g_[:, 1]).numel()) for g_ in gathered],
                             "via": "yolov7_tracker_amd.sharding.rebase_and_gather (2 all_reduce of 2 x world int64 + 1 gather)"}
    torch.cuda.synchronize()
    det.check_overflow()

    fwd_ms = [ev_fwd0[s].elapsed_time(ev_fwd1[s]) for s in range(Wm, Wm + K)]
    nms_ms = [ev_fwd1[s].elapsed_time(ev_nms[s]) for s in range(Wm, Wm + K)]
    gflop_frame = det.gflop_per_frame
    conv_tflops = gflop_frame * B / (np.mean(fwd_ms) * 1e-3) / 1e3
    traffic, traffic_meta = None, {}
    tpath = next((q for q in (os.path.join(ROOT, "profiles", n) for n in ("r06_conv_hbm_traffic.json", "r05_conv_hbm_traffic.json", "r04_conv_hbm_traffic.json", "r03_conv_hbm_traffic.json", "r02_conv_hbm_traffic.json")) if os.path.exists(q)), "")
    if tpath:      # PMC counters cannot be collected inside the timed run: separate rocprofv3 --pmc passes, committed WITH the launch list they were taken on
        traffic_meta = json.load(open(tpath))
    if rank == 0:
        # sanity: the tracker produced tracks
        last = results[(Wm + K) * B - 1].cpu().numpy()
        n_tracks_last = int(last[trk.cap_t].view(np.int32)[0])
        fps = world * K * B / dt_s
        line = {
            "metric": metric_name, "value": round(fps, 2), "unit": "frames/s",
            "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": round(dt_s / K * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": ("configs[2]: YOLOv7-w6 1280x1280 + BoT-SORT (xywh Kalman, multi_gmc with a synthetic 2x3 warp per frame)" if cfg3 else
                                    "configs[3]: YOLOv7-w6 1280x1280 + DeepSORT, OSNet x0_25 embeddings of 128x64 crops of every detection (one fused "
                                    "MFMA kernel, one workgroup per crop), cascade + gated cosine/Mahalanobis cost on the device" if cfg4 else
                                    "configs[1]: YOLOv7-w6 1280x1280 + ByteTrack") + ", %d synthetic VisDrone-shape sequence%s per GPU, %d objects per frame "
                                   "(10 %% missed, 5 %% false positives, reflected at the border)" % (S, "" if S == 1 else "s (their tracker chains side by side)", args.n_obj), "frames_per_step": B, "arch": args.arch, "nc": nc,
                       "tracker": tracker_name, "sequences_per_gpu": S,
                       "input_batches_rotated": N_ROT, "track_rows_copied_to_host_inside_the_timed_region": graph is None,
                       "tracks_alive_last_frame": n_tracks_last, "nms_candidates_last": int(det.plan.cand.max().item()),
                       "parallelism": "sequence-sharded x%d" % world, "collective_backend": backend if world > 1 else None,
                       "result_gather": gathered_info if world > 1 else None},
            "roofline": {"bound": "mfma", "achieved": round(conv_tflops, 2), "peak": PEAK_MFMA_F16 / 1e12, "unit": "TFLOP/s",
                         "frac": round(conv_tflops * 1e12 / PEAK_MFMA_F16, 4), "traffic": None,
                         "sustained_peak": 1627.0,
                         "sustained_peak_note": "register-only v_mfma_f32_32x32x16_f16 loop with random operands (power-limited clock; "
                                                "2278-2389 with zero / constant operands): scripts/ubench/mfma_power.hip, re-measured in round 6 "
                                                "(1624 / 1631 TFLOP/s, profiles/r06_small_experiments.txt; round 1: 1550-1565)",
                         "frac_of_sustained_peak": round(conv_tflops / 1627.0, 4),
                         "traffic_note": None,
                         "kernel": "the conv launch list of one forward (107 convs in 96 launches + 1 pool launch: k_stem_u8, k_conv3x3s2_c64_ws, k_conv3x3_c64_ws, k_conv3x3_c128_ws, k_conv3x3_patch*, "
                                   "k_conv3x3s2_patch, k_conv1x1_p8, k_conv_igemm, k_spp3_lds; nearest-x2 upsamples folded into their consumers' loaders, Detect decode + "
                                   "candidate filter in the Detect convs' epilogues)",
                         "algorithmic_gflop_per_launch_list": round(gflop_frame * B, 1),
                         "launch_list_ms": round(float(np.mean(fwd_ms)), 3)},
            "phases_ms_per_step": {"detector_forward": round(float(np.mean(fwd_ms)), 3), "decode_nms": round(float(np.mean(nms_ms)), 3),
                                   "tracker_chain": round(float(np.mean([ev_trk0[s].elapsed_time(ev_trk1[s]) for s in range(Wm, Wm + K)])), 3),
                                   "note": "decode_nms = end of this batch's forward (its Detect epilogues have already decoded + filtered) -> end of its rank sort + "
                                           "NMS on stream C: held back until the NEXT forward has left the memory-bound 640^2/320^2 layers, then overlaps the "
                                           "rest of that forward (latency, not cost)"},
        }
        timed = range(Wm * B, (Wm + K) * B)
        line["config"]["dets_per_frame_timed_mean"] = round(float(np.mean([len(dets_seq[t]) for t in timed])), 2)
        line["config"]["tracks_per_frame_timed_mean"] = round(float(np.mean([int(results[t, trk.cap_t].cpu().numpy().view(np.int32)[0]) for t in list(timed)[::8]])), 2)
        if dt_h2d is not None:
            line["fps_incl_h2d"] = {"value": round(K * B / dt_h2d, 2), "ms_per_step": round(dt_h2d / K * 1e3, 3),
                                    "note": "same pipeline, every batch copied from pinned host memory (uint8 BGR, %.1f MB per frame) on a copy "
                                            "stream, double-buffered; never `value`" % (H * W * 3 / 1e6)}
        line["value_note"] = ("frames resident in HBM when the timed region starts (the measurement contract of this build: a PCIe-inclusive rate is never `value`); "
                              "the reference's own timer starts with the frame on the host (tracker/track.py:140): that rate is `fps_incl_h2d` (--full), and `coupled` is the same "
                              "host-fed pipeline with the tracker consuming the step's own NMS output")
        for cv in coupled_variants:
            s0c, tc, rc_, dtc = cv["first"] + Wm, cv["trk"], cv["results"], dt_coupled[cv["name"]]
            cnts = torch.stack([rc_[t, tc.cap_t].view(torch.int32)[0] for t in range(Wm * B, (Wm + K) * B, 4)]).cpu().numpy()
            line[cv["name"]] = {"fps": round(K * B / dtc, 2), "ms_per_step": round(dtc / K * 1e3, 3),
                                "tracker_chain_ms": round(float(np.mean([ev_trk0[s_].elapsed_time(ev_trk1[s_]) for s_ in range(s0c, s0c + K)])), 3),
                                "launch_list_ms": round(float(np.mean([ev_fwd0[s_].elapsed_time(ev_fwd1[s_]) for s_ in range(s0c, s0c + K)])), 3),
                                "score_gain_in_the_handover": round(cv["gain"], 3),
                                "tracks_per_frame_mean": round(float(cnts.mean()), 1), "tracker_status": int(tc._status())}
        if coupled_variants:
            pl_ = det.plan.post[(coupled_variants[-1]["first"] + K + Wm - 1) % 2]      # the rows of the very last step (the second pass's gain already in them)
            nd_last, dl = pl_.ndets[:B].cpu().numpy(), pl_.dets[:B].cpu().numpy()
            g2 = coupled_variants[-1]["gain"]
            line["coupled"]["nms_rows_per_frame_mean"] = round(float(nd_last.mean()), 1)
            for nm_, div_ in (("coupled", g2), ("coupled_confident_rows", 1.0)):
                line[nm_]["rows_at_or_above_0.3_0.2_0.15_mean"] = [round(float(np.mean([(dl[b, :nd_last[b], 4] / div_ >= th_).sum() for b in range(B)])), 1) for th_ in (0.3, 0.2, 0.15)]
            line["coupled"]["note"] = ("third timed pass: frames from pinned host memory, forward, rank sort + NMS, and the SAME step's (300, 6) rows and row counts read by "
                                       "y7t_tracker_step_frames on the device (no synthetic detections, no host round trip), track rows to the host; a fresh ByteTrack with the "
                                       "CLI's thresholds. Random weights: hardly a row of a frame's 300 reaches 0.2, none the birth gate -- this pass times the data path")
            line["coupled_confident_rows"]["note"] = ("fourth timed pass: the same, with the rows' score column multiplied by one constant in the hand-over (every frame's n_obj-th best row -> "
                                                      "det_thresh), so that the tracker associates as many confident rows per frame as the headline's scene has detections. The boxes "
                                                      "are a random head's (up to 1000+ px, heavily overlapping): an ill-posed association, the tracker's worst case rather than a scene")
        exps = {k: v for k, v in os.environ.items() if k.startswith("Y7T_") and k != "Y7T_TEST_EXPERIMENTS"}
        if exps:      # a run with experiment switches in the environment says so in its own line (none in the driver's run)
            line["config"]["environment_switches"] = exps
        if world == 1 and args.full:
            hist, ll_names = {}, det.launch_list(B)
            for nme in ll_names:
                hist[nme] = hist.get(nme, 0) + 1
            line["config"]["launch_list"] = hist
            import hashlib
            ll_sha = hashlib.sha1(json.dumps(ll_names).encode()).hexdigest()[:16]
            line["config"]["launch_list_sha"] = ll_sha
            # roofline.traffic is a PMC measurement of a particular launch list: printed only when THIS run's list is the one it was taken on
            r = line["roofline"]
            if traffic_meta.get("launch_list_sha") == ll_sha and traffic_meta.get("frames_per_launch_list") == B:
                r["traffic"] = traffic_meta["hbm_bytes_per_frame"] * B
                r["traffic_note"] = ("HBM bytes per launch list from profiles/%s (FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes; measured at commit %s on "
                                     "launch list %s = this run's); algorithmic = 1.217 GB/frame"
                                     % (os.path.basename(tpath), traffic_meta.get("commit", "?"), ll_sha))
            else:
                r["traffic_note"] = ("not reported: the committed PMC passes (profiles/%s, launch list %s) were taken on another launch list than this run's (%s); "
                                     "scripts/gpu_round.sh profile re-measures" % (os.path.basename(tpath) or "-", traffic_meta.get("launch_list_sha", "unstamped"), ll_sha))
            with torch.cuda.stream(sA):
                out0 = det.forward(frames, fuse_decode=CONF)       # the launch_list probe re-ran ops out of context: redo frame 0..B-1 cleanly
                d0, n0 = det.postprocess(out0, CONF, 0.45, None)
            torch.cuda.synchronize()
            cb, cs, cc, ci_, cn = det.candidate_arrays(out0.pset)
            n_c0 = int(cn[0])
            cands0 = {int(r_): (bx, float(sc), int(cl)) for r_, bx, sc, cl in zip(ci_[0, :n_c0].cpu().numpy(), cb[0, :n_c0].cpu().numpy(),
                                                                                cs[0, :n_c0].cpu().numpy(), cc[0, :n_c0].cpu().numpy())}
            heads0 = [r[:1].cpu() for r in out0.raw()]
            dets0 = d0[0, :int(n0[0])].cpu()
            kept_rows0 = ci_[0].cpu().numpy()[det.plan.post[out0.pset].keep[0, :int(n0[0])].cpu().numpy()]      # anchor row of every kept detection of frame 0
            if cfg4:
                pr = trk._state[trk._layout["hdr_prof"]:trk._layout["hdr_prof"] + 256].view(torch.int64).cpu().numpy()
                line["config"]["cascade"] = {"frames_with_several_ages": int(pr[27]), "of_them_with_a_contested_detection": int(pr[28]),
                                             "solved_as_one_assignment": int(pr[29])}
                rs = [ev_reid[s][0].elapsed_time(ev_reid[s][1]) for s in range(Wm, Wm + K)]
                line["phases_ms_per_step"]["reid"] = round(float(np.mean(rs)), 3)
                n_crops = float(np.mean([len(step_boxes[s]) for s in range(Wm, Wm + K)]))
                line["config"]["reid_crops_per_step_mean"] = round(n_crops, 1)
                # configs[3]'s own kernel ("ReID conv as MFMA kernel") against ITS roof: algorithmic MACs of OSNet x0_25 per 128 x 64 crop, counted from the op
                # list (tracker/reid.py::macs_per_crop), x 2 x crops / the HIP-event time of the one k_osnet_x025 launch of a step
                from yolov7_tracker_amd.tracker import reid as _reid
                dense, other = _reid.macs_per_crop(reid.ops)
                tfl = 2.0 * (dense + other) * n_crops / (np.mean(rs) * 1e-3) / 1e12
                line["roofline_reid"] = {"kernel": "k_osnet_x025 (csrc/y7t_reid_fused.hip): crop + resize + Normalize + OSNet x0_25 in one workgroup per crop, "
                                                   "1x1 convs / 7x7 stem / fc on v_mfma_f32_16x16x16_f16, depthwise 3x3 and gates on the VALU",
                                         "bound": "latency (about 140 barrier-separated phases per crop, activations resident in LDS)",
                                         "algorithmic_mmac_per_crop": {"mfma": round(dense / 1e6, 2), "valu": round(other / 1e6, 2)},
                                         "achieved": round(tfl, 2), "peak": PEAK_MFMA_F16 / 1e12, "unit": "TFLOP/s", "frac": round(tfl * 1e12 / PEAK_MFMA_F16, 4),
                                         "hbm_bytes_per_crop": "source pixels of the crop (uint8, read once) + 2 KB of embedding out; parameters 461 KB, L2-resident",
                                         "lds_bank_conflict_rate": "0.27 (profiles/r02_reid_pmc.json: the depthwise reads of the 32-channel stages)"}
                nd_ = float(np.mean([len(dets_seq[t_]) for t_ in range(Wm * B, (Wm + K) * B)]))
                live = float(line["config"].get("tracks_alive_last_frame", 0))
                line["roofline_embed_dist"] = {"kernel": "k_embed_dist: nearest cosine distance of every live slot's <= 100 stored vectors to every detection (fp32 FMA chains)",
                                               "bound": "hbm", "algorithmic_bytes_per_frame": int(live * 100 * 512 * 4 + nd_ * 512 * 4 + live * nd_ * 4),
                                               "note": "~%.1f MB per frame (%.0f live slots x 100 rows x 512 floats): 2-3 us at HBM rate, measured 0.13 ms inside the pipeline "
                                                       "(profiles/r02_deepsort_phases.txt) -- latency / occupancy bound at this size, not bandwidth" % (live * 100 * 512 * 4 / 1e6, live)}
            if not args.no_latency_mode and not cfg3 and not cfg4:
                line["latency_mode"] = latency_mode(args, nc, frames_host, dets_seq, sd=sd0)
            if not args.no_latency_mode and not cfg4:            # (same switch: the extras of the driver's default line)
                line["roofline_tracker"] = roofline_tracker(det, frames, nc, args.img)
            if not args.no_cpu_baseline and not cfg4:            # the CPU baseline is timed on rank 0 at N=1 only (configs[1] / [2])
                line["cpu_baseline"], line["parity"] = cpu_baseline(args, det, frames_host, dets_seq, heads0, dets0, cands0, kept_rows0)
                line["parity"]["weights"] = args.weights
                if conditioned:
                    line["parity"]["note"] = ("frame 0 of the TIMED run (same weights, same launch list, %d frames per forward) against the fp32 oracle: raw heads, the "
                                              "pre-NMS candidate set at SURVEY 8a's full bar (same class, IoU >= 0.99 or |dcoord| <= 1 px, |dconf| <= 5e-3: every candidate, all four "
                                              "Detect levels live), and the final boxes by anchor row (every row only one side keeps is traced to the greedy NMS decision that "
                                              "flipped and shown to be a tie within the frame's measured score noise: `reasons`)" % B)
                else:
                    line["parity"]["note"] = ("the benchmarked weights are iid random (chaotic: rounding noise x ~300 over the depth); the same kernels "
                                              "on well-conditioned seeded weights:")
                    line["parity"]["well_conditioned"] = parity_well_conditioned(args, nc, frames_host)
                if args.chained_frames > 0 and not cfg3 and len(frames_host) >= args.chained_frames:
                    line["parity"]["chained"] = chained_parity(args, nc, frames_host, args.chained_frames)
            if not args.no_other_workloads and not cfg3 and not cfg4:
                line["other_workloads"] = other_workloads(args)
        print(json.dumps(line))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
