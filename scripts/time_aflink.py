"""AFLink on the device: the device time of y7t_aflink_score_pairs_f32 at 1 000 and 10 000 pairs, the time of the whole y7t_aflink_candidates call (gate, compaction,
transform, network) on a scene of about 1 000 tracklets, and -- in the same run -- the same network as a torch module on the host CPU, one pair per forward (as the
StrongSORT release evaluates it) and batched.  (The torch module below is this project's statement of PostLinker, checked here against the device scores; the
reference's own file is timed nowhere, it is not on the measuring machine.)

    python scripts/time_aflink.py [--out profiles/aflink_timing.txt]

Device times are HIP events around `reps` back-to-back calls after a warm-up of every shape; the rates follow from 32.8 MFLOP (16.4 M multiply-adds) a pair and the
157.3 TFLOP/s fp32 matrix peak.  A whole-call rate over peak is an end-to-end figure, not a kernel's share of peak."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOP_PER_PAIR = 32.8e6
PEAK = 157.3e12


def torch_module(weights):
    import torch
    import torch.nn.functional as F
    w = {k: torch.from_numpy(v) for k, v in weights.items()}

    def bn(x, p):      # x [..., C] channel last
        return (x - w[p + ".running_mean"]) / torch.sqrt(w[p + ".running_var"] + 1e-5) * w[p + ".weight"] + w[p + ".bias"]

    @torch.no_grad()
    def forward(x1, x2):
        feats = []
        for b, x in ((1, x1), (2, x2)):
            h = x[:, None]      # [P][1][30][3]
            for k in range(4):
                p = "TemporalModule_%d.%d" % (b, k)
                y = F.conv2d(h, w[p + ".conv.weight"])
                y = torch.stack([bn(y[:, :, :, c].transpose(1, 2), "%s.%s" % (p, n)).transpose(1, 2) for c, n in enumerate(("bnf", "bnx", "bny"))], 3)
                h = torch.relu(y)
            y = F.conv2d(h, w["FusionBlock_%d.conv.weight" % b])[:, :, :, 0]
            y = torch.relu(bn(y.transpose(1, 2), "FusionBlock_%d.bn" % b))
            feats.append(y.mean(1))
        v = torch.cat(feats, 1)
        lg = F.linear(torch.relu(F.linear(v, w["classifier.fc1.weight"], w["classifier.fc1.bias"])), w["classifier.fc2.weight"], w["classifier.fc2.bias"])
        return torch.softmax(lg, 1)[:, 1]

    return forward


def scene(n_tracklets, seed=0):
    rng = np.random.RandomState(seed)
    trk = []
    for _ in range(n_tracklets):
        n, f0 = int(rng.randint(5, 61)), int(rng.randint(1, 600))
        f = np.arange(f0, f0 + n, dtype=np.float64)
        pos, vel = rng.uniform(0, 1280, 2), rng.uniform(-4, 4, 2)
        trk.append(np.column_stack([f, pos[0] + (f - f0) * vel[0], pos[1] + (f - f0) * vel[1]]))
    off = np.zeros(n_tracklets + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in trk])
    return np.concatenate(trk, 0), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aflink_timing.txt"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from yolov7_tracker_amd import _lib, synth
    from yolov7_tracker_amd.tracker.aflink import DeviceAFLink
    _lib.require_gpu()      # a measurement without a device fails, it does not fall back
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    weights = synth.make_aflink_weights(3, 1.5)
    model = DeviceAFLink(weights, max_tracklets=2048, max_rows=1 << 17, max_pairs=1 << 16)
    say("# AFLink timing on %s, torch %s; %d repetitions after a warm-up" % (torch.cuda.get_device_name(0), torch.__version__, args.reps))
    say("# y7t_aflink_score_pairs_f32: HIP events around the repetitions; end-to-end rate of the call (six launches a chunk of 2048 pairs), not a kernel's share of peak")
    x1, x2 = synth.make_aflink_pairs(256, 99)
    for P in (1000, 10000):
        idx = np.arange(P) % 256
        a, b = torch.from_numpy(x1[idx]).cuda(), torch.from_numpy(x2[idx]).cuda()
        first = model.score_pairs(a, b)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            out = model.score_pairs(a, b)
        e1.record()
        torch.cuda.synchronize()
        assert torch.equal(first, out)
        ms = e0.elapsed_time(e1) / args.reps
        say("P = %5d  %8.3f ms  %10.0f pairs/s  %6.2f TFLOP/s  %5.1f %% of the 157.3 TFLOP/s fp32 matrix peak" % (
            P, ms, P / (ms * 1e-3), FLOP_PER_PAIR * P / (ms * 1e-3) / 1e12, 100 * FLOP_PER_PAIR * P / (ms * 1e-3) / PEAK))
    dev_scores = model.score_pairs(x1, x2).cpu().numpy()
    say("# y7t_aflink_candidates through DeviceAFLink.candidates: host clock around the call (table upload, the launches, the read-back of count, pairs and scores)")
    table, off = scene(1000)
    res = model.candidates(table, off)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = model.candidates(table, off)
        ts.append(time.perf_counter() - t0)
    say("N = 1000 tracklets, %d rows, %d candidates (status %d): %8.3f ms median, %8.3f ms min" % (len(table), res["count"], res["status"], 1e3 * np.median(ts), 1e3 * np.min(ts)))
    say("# the same network as a torch module on the host CPU (%d threads), float32" % torch.get_num_threads())
    fwd = torch_module(weights)
    a, b = torch.from_numpy(x1), torch.from_numpy(x2)
    cpu = fwd(a, b).numpy()
    say("(device vs this module over 256 pairs: max |difference| %.3g)" % np.abs(cpu - dev_scores).max())
    fwd(a[:1], b[:1])
    t0 = time.perf_counter()
    for k in range(100):
        fwd(a[k:k + 1], b[k:k + 1])
    one = (time.perf_counter() - t0) / 100
    big_a, big_b = a[np.arange(1000) % 256], b[np.arange(1000) % 256]
    fwd(big_a, big_b)
    t0 = time.perf_counter()
    fwd(big_a, big_b)
    batched = time.perf_counter() - t0
    say("one pair per forward: %8.3f ms a pair  %8.0f pairs/s" % (1e3 * one, 1 / one))
    say("batched, 1000 pairs : %8.3f ms a pair  %8.0f pairs/s" % (1e3 * batched / 1000, 1000 / batched))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
