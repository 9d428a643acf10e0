"""tests/golden/make_golden_aflink.py -- regenerates the committed AFLink golden vectors (aflink_pairs.npz, aflink_link_*.npz).

Runs ONLY in the build container (needs the reference sources): it imports the reference's own tracker/reid_models/AFLink.py through oracle/ref_harness.py (cv2 and
torchvision are stubbed there), loads the seeded weights of synth.make_aflink_weights into its PostLinker (weights are never stored, only seed and gain) and
evaluates it in eval mode.  The maker asserts that the float tensors of the reference's own state dict are, by name, order and shape, synth.aflink_tensor_shapes().

aflink_pairs.npz: 256 transformed pairs of seeded synthetic tracklets (lengths 1, 2, 29, 30, 31, 60, gaps 0..29, a constant column, a single-row pair), the
reference module's float32 scores, the same module's scores in .double(), e_ref = max|s32 - s64| and E, the largest e_ref of the set: a device score must lie
within 4 E of the float64 score (tests/test_aflink_gpu.py).
aflink_link_<name>.npz: scenes of at most 40 tracklets over 120 frames, synth.make_ground_truth tracks cut into fragments with fresh ids: the rows in, the candidate
pair list, the reference module's float32 and float64 scores of the candidates, the accepted links and the rows out (tests/aflink_np.py with the float32 scores).
A scene is kept only if no candidate's cost lies within 4 E of thrP and neither the links nor the rows out change with the float64 scores or under +-4 E with
random signs.  The set must hold a chain a -> b -> c, an accepted pair whose latter begins in the former's last frame (a duplicate row), a scene without a
candidate, a compressed-away row or column, an accepted and a rejected pair: the maker fails loudly otherwise.

    python tests/golden/make_golden_aflink.py
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from tests import aflink_np  # noqa: E402
from yolov7_tracker_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, GAIN = 3, 1.5
PAIR_SEED, N_PAIRS = 99, 256
THR_T, THR_S, THR_P = (0, 30), 75, 0.05


def load_reference():
    with ref_harness._patched_modules([os.path.join(ref_harness.REF_ROOT, "tracker", "reid_models")]):
        sys.modules.pop("AFLink", None)
        mod = importlib.import_module("AFLink")
        sys.modules.pop("AFLink", None)
    return mod


def reference_nets(mod):
    net = mod.PostLinker()
    sd = net.state_dict()
    floats = [(k, tuple(v.shape)) for k, v in sd.items() if not k.endswith("num_batches_tracked")]
    assert floats == [(k, tuple(s)) for k, s in synth.aflink_tensor_shapes()], "the reference's state dict is not synth.aflink_tensor_shapes()"
    assert sum(int(np.prod(s)) for _, s in floats) == aflink_np.N_WEIGHTS == 1075266
    w = synth.make_aflink_weights(SEED, GAIN)
    net.load_state_dict({k: torch.from_numpy(w[k]) if k in w else v for k, v in sd.items()})
    net.eval()
    return net, copy.deepcopy(net).double(), w


def ref_scores(net, x1, x2, dtype):
    if len(x1) == 0:
        return np.zeros(0, np.float32 if dtype == torch.float32 else np.float64)
    with torch.no_grad():
        y = net(torch.as_tensor(np.asarray(x1), dtype=dtype)[:, None], torch.as_tensor(np.asarray(x2), dtype=dtype)[:, None])
    return y[:, 1].numpy()


def make_scene(seed, n_obj, dup_rate=0.25):
    """make_ground_truth tracks cut into fragments with fresh ids -> rows (R, 6) float64 [frame, id, x, y, w, h]"""
    rng = np.random.RandomState(5000 + seed)
    gt = synth.make_ground_truth(120, n_obj, 1280, seq_idx=300 + seed)
    per = {}
    for t, rows in enumerate(gt):
        for r in rows:
            per.setdefault(int(r[0]), []).append([t + 1, 0, r[1], r[2], r[3], r[4]])
    out, next_id = [], 1
    for oid in sorted(per):
        tr = np.array(per[oid], np.float64)
        k = int(rng.randint(1, 4))
        cuts = sorted(rng.choice(np.arange(10, len(tr) - 10), k - 1, replace=False).tolist()) if k > 1 and len(tr) > 30 else []
        start = 0
        for c in cuts + [len(tr)]:
            frag = tr[start:c].copy()
            if len(frag):
                frag[:, 1] = next_id
                next_id += 1
                out.append(frag)
            if c < len(tr):
                start = c - 1 if rng.rand() < dup_rate else c + int(rng.randint(0, 20))      # the next fragment repeats the last frame, or a gap of 0..19 frames
    rows = np.concatenate(out, 0)
    rows = rows[rng.permutation(len(rows))]                   # the file order is not the frame order
    return np.round(rows, 2)                                  # values as a results file holds them


def evaluate(rows, net, net64, E, rng):
    """-> (record, flags) or None when the scene is not stable"""
    trace = {}
    s64_of = {}

    def f32(pairs, x1, x2):
        s = ref_scores(net, x1, x2, torch.float32)
        s64_of["s"] = ref_scores(net64, x1, x2, torch.float64)
        return s

    out = aflink_np.link(rows, f32, THR_T, THR_S, THR_P, trace=trace)
    s32, s64 = trace["scores"], s64_of.get("s", np.zeros(0))
    cost = (np.float32(1) - s32).astype(np.float64)
    if len(cost) and np.abs(cost - THR_P).min() <= 4 * E:
        return None
    links = trace["links"]
    for alt in (s64.astype(np.float32), (s32.astype(np.float64) + np.where(rng.rand(len(s32)) < 0.5, -4 * E, 4 * E)).astype(np.float32)):
        t2 = {}
        out2 = aflink_np.link(rows, lambda p, a, b: alt, THR_T, THR_S, THR_P, trace=t2)
        if not (np.array_equal(out, out2) and np.array_equal(links, t2["links"])):
            return None
    n = len(trace["ids"])
    lk = [tuple(x) for x in links.tolist()]
    off, table = trace["offsets"], trace["table"]
    flags = dict(
        chain=any((j, k) in lk for i, j in lk for k in range(n)),
        dup=any(table[off[j], 0] == table[off[i + 1] - 1, 0] for i, j in lk),
        nocand=len(s32) == 0,
        compressed=len(lk) > 0 and (len({i for i, _ in lk}) < n or len({j for _, j in lk}) < n),
        accepted=len(lk) > 0,
        rejected=bool((cost >= THR_P).any()),
        dropped_rows=len(out) < len(rows))
    rec = dict(rows_in=rows, pairs=trace["pairs"], scores32=s32, scores64=s64, links=links, rows_out=out, n_tracklets=np.array(n), thrT=np.array(THR_T, np.float64),
               thrS=np.array(float(THR_S)), thrP=np.array(THR_P), seed=np.array(SEED), gain=np.array(GAIN), E=np.array(E), numpy_version=np.array(np.__version__),
               torch_version=np.array(torch.__version__))
    return rec, flags


def main():
    mod = load_reference()
    net, net64, w = reference_nets(mod)
    x1, x2 = synth.make_aflink_pairs(N_PAIRS, PAIR_SEED)
    s32, s64 = ref_scores(net, x1, x2, torch.float32), ref_scores(net64, x1, x2, torch.float64)
    assert s32.dtype == np.float32 and s64.dtype == np.float64
    e_ref = float(np.abs(s32.astype(np.float64) - s64).max())
    E = e_ref
    mine = aflink_np.forward_packed(np.concatenate([w[k].reshape(-1) for k, _ in synth.aflink_tensor_shapes()]), x1, x2)
    print("pairs: scores %.3g .. %.3g, %d >= 0.95, e_ref = E = %.3g, restatement vs float64 %.3g, nearest to 0.95: %.3g" % (
        s64.min(), s64.max(), int((s64 >= 0.95).sum()), E, np.abs(mine - s64).max(), np.abs(s64 - 0.95).min()))
    path = os.path.join(HERE, "aflink_pairs.npz")
    np.savez_compressed(path, x1=x1, x2=x2, scores32=s32, scores64=s64, e_ref=np.array(e_ref), E=np.array(E), seed=np.array(SEED), gain=np.array(GAIN),
                        pair_seed=np.array(PAIR_SEED), torch_version=np.array(torch.__version__))
    print("aflink_pairs.npz", os.path.getsize(path), "bytes")

    rng = np.random.RandomState(777)
    want = ["chain", "dup", "compressed", "accepted", "rejected", "dropped_rows"]
    have, kept = set(), []
    # the scene without a candidate: whole tracks, every one begins before every other ends
    gt = synth.make_ground_truth(120, 3, 1280, seq_idx=299)
    rows = np.round(np.array([[t + 1, int(r[0]) + 1, r[1], r[2], r[3], r[4]] for t, g in enumerate(gt) for r in g], np.float64), 2)
    rec, flags = evaluate(rows, net, net64, E, rng)
    assert flags["nocand"] and np.array_equal(rec["rows_out"], rows[np.lexsort((rows[:, 1], rows[:, 0]))])
    kept.append(("nocand", rec, flags))
    for seed in range(400):
        if all(k in have for k in want) or len(kept) >= 6:
            break
        r = evaluate(make_scene(seed, 8 + seed % 8), net, net64, E, rng)
        if r is None:
            continue
        rec, flags = r
        new = {k for k in want if flags[k]} - have
        if not new or rec["n_tracklets"] > 40:
            continue
        have |= new
        kept.append(("s%d" % seed, rec, flags))
    missing = [k for k in want if k not in have]
    assert not missing, "the set has no %s" % missing
    for name, rec, flags in kept:
        path = os.path.join(HERE, "aflink_link_%s.npz" % name)
        np.savez_compressed(path, **rec, **{"flag_" + k: np.array(v) for k, v in flags.items()})
        print(name, "tracklets", int(rec["n_tracklets"]), "rows", len(rec["rows_in"]), "->", len(rec["rows_out"]), "candidates", len(rec["pairs"]), "links", len(rec["links"]),
              {k: v for k, v in flags.items() if v}, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    assert ref_harness.available(), "needs the reference sources"
    main()
