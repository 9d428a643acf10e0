"""tests/golden/make_golden_deepmot.py -- regenerates the committed DeepMOT golden vectors (dhn_*.npz, tracker_deepmot_*.npz).

Runs ONLY in the build container (needs the reference sources): it imports the reference's own tracker/deepmot.py through oracle/ref_harness.py (torchvision and
reid_models are stubbed there), neutralises `Tensor.cuda` while the reference constructs and runs its network on the CPU, replaces `torch.load` by the seeded
state dict (synth.make_dhn_weights; weights are never stored) and calls `.eval()` on the reference's module -- the reference never does, so its dropout is live and
its own output random (DeepMOT).

dhn_*.npz: D, the reference module's float32 output, the same module evaluated in float64 (.double(), float64 hidden state), e_ref = max|out32 - out64|, and
E = the largest e_ref of the set: the device output must lie within 4 E of the float64 output (tests/test_deepmot_gpu.py).
tracker_deepmot_*.npz: what DeepMOT.update returns on seeded scenes of at most 24 objects x 30 frames: the rows, the ids of the tracked / lost lists after every
frame, the detections, the weight seed and scale, and the counts of the events the set must contain.  A scene is kept only if the reference's ids and lists do not
change when its network output is replaced by the float64 evaluation, nor when it is perturbed by +-4 E with random signs: the maker fails loudly otherwise.

    python tests/golden/make_golden_deepmot.py [name,...]
"""
import contextlib
import copy
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from yolov7_tracker_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DHN_SEED, DHN_SCALE = 7, 3.0
DHN_SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (12, 9), (33, 20), (64, 48)]      # non-square: the row / column re-order; T = 660 and 3072 cross a position chunk
IMG_SHAPE = (720, 1280)

CASES = [
    # name, n_frames, n_obj, seq_idx, make_detections arguments, conf_thresh, empty_every, none_every, kalman_format, weight seed, weight scale
    ("default", 30, 20, 50, {}, 0.2, 0, 0, "default", 7, 3.0),
    ("miss", 30, 20, 51, {"miss": 0.2}, 0.2, 0, 0, "default", 7, 3.0),
    ("conf04", 30, 20, 52, {"conf_jitter": 0.2}, 0.4, 0, 0, "botsort", 7, 3.0),
    ("empty", 30, 16, 53, {}, 0.2, 7, 0, "default", 7, 3.0),
    ("gaps", 30, 16, 54, {"miss": 0.2}, 0.2, 0, 5, "strongsort", 7, 3.0),
    ("reject", 25, 20, 55, {}, 0.2, 0, 0, "default", 7, 4.0),               # weights that reject some first-association pairs
    ("crowd", 30, 24, 56, {"miss": 0.3, "conf_jitter": 0.25}, 0.5, 0, 0, "default", 7, 4.0),      # non-square: up to 23 pool tracks x 14 high detections; second-association matches
]


def make_scene(nf, nobj, seq, extra, empty_every=0, none_every=0):
    dets = synth.make_detections(nf, nobj, 1280, seq_idx=seq, **extra)
    if empty_every:
        dets = [np.zeros((0, 6), np.float32) if i % empty_every == empty_every - 1 else d for i, d in enumerate(dets)]
    if none_every:
        dets = [None if i % none_every == none_every - 1 else d for i, d in enumerate(dets)]
    return dets


def frames_from_golden(g):
    """the per-frame detections of a tracker golden (None: update_without_detection)"""
    out, o = [], 0
    for c in g["det_counts"].tolist():
        if c < 0:
            out.append(None)
        else:
            out.append(g["dets"][o:o + c])
            o += c
    return out


@contextlib.contextmanager
def _cpu_only():
    """Munkrs(is_cuda=True) calls .cuda() on its hidden state: the identity while the reference runs here"""
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = saved


class _Matching:
    """the harness's matching module with linear_assignment logged: (thresh, cost, matches, unmatched rows, unmatched columns) per call"""

    def __init__(self, inner):
        self._inner, self.log = inner, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def linear_assignment(self, cost, thresh):
        r = self._inner.linear_assignment(cost, thresh=thresh)
        self.log.append((thresh, np.array(cost), r[0], r[1], r[2]))
        return r


def load_deepmot():
    """-> the reference's deepmot module; its matching is the harness's (the np.float shim, lap and cython_bbox restated in oracle/cnative.py), logged"""
    with ref_harness._patched_modules([os.path.join(ref_harness.REF_ROOT, "tracker")]):
        for name in ("basetrack", "matching", "deepmot"):
            sys.modules.pop(name, None)
        mod = importlib.import_module("deepmot")
        sys.modules.pop("deepmot", None)
    mod.matching = _Matching(ref_harness.load_tracker().matching)
    mod.STrack.__init__.__globals__["matching"] = mod.matching._inner
    return mod


def reference_dhn(mod, seed, scale):
    """-> (the reference's Munkrs in eval mode with the seeded weights, its float64 copy)"""
    with _cpu_only():
        net = mod.Munkrs(element_dim=1, hidden_dim=256, target_size=1, bidirectional=True, minibatch=1, is_cuda=True, is_train=False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_dhn_weights(seed, scale).items()})
    net.eval()
    net64 = copy.deepcopy(net).double()
    net64.init_hidden = lambda batch: torch.zeros(4, batch, 256, dtype=torch.float64)
    return net, net64


def eval_dhn(net, D, dtype):
    with _cpu_only(), torch.no_grad():
        return net(torch.as_tensor(D, dtype=dtype).unsqueeze(0)).squeeze(0).numpy()


def run_reference(dets, mod, conf_thresh, kalman_format, seed, scale, net_mode="f32", tol=0.0, timing=None, counts=None, net_timing=None):
    """-> per frame (rows, tracked ids, lost ids).  net_mode: f32 (the reference's own float32 forward), f64 (replaced by the float64 evaluation), perturb (float32 +- tol,
    random signs)"""
    next(c for c in mod.STrack.__mro__ if c.__name__ == "BaseTrack")._count = 0
    saved_load = torch.load
    torch.load = lambda *a, **k: {k_: torch.from_numpy(v) for k_, v in synth.make_dhn_weights(seed, scale).items()}
    try:
        with _cpu_only():
            trk = mod.DeepMOT(ref_harness.make_opts(conf_thresh=conf_thresh, kalman_format=kalman_format, dhn_path="seeded"), frame_rate=30)
    finally:
        torch.load = saved_load
    net = trk.DHN.eval()
    net64 = copy.deepcopy(net).double()
    net64.init_hidden = lambda batch: torch.zeros(4, batch, 256, dtype=torch.float64)
    rng = np.random.RandomState(12345)

    def forward(D):
        t0 = time.perf_counter()
        with torch.no_grad():
            if net_mode == "f64":
                out = net64(D.double())
            else:
                out = net(D)
                if net_mode == "perturb":
                    out = out + torch.from_numpy(np.where(rng.rand(*out.shape) < 0.5, -tol, tol).astype(np.float32))
        if net_timing is not None:
            net_timing.append((tuple(D.shape[1:]), time.perf_counter() - t0))
        return out

    trk.DHN = forward
    img = np.zeros(IMG_SHAPE + (3,), np.uint8)
    n_react = [0]
    orig_react = mod.STrack.re_activate

    def react(self, *a, **k):
        n_react[0] += 1
        return orig_react(self, *a, **k)

    mod.STrack.re_activate = react
    out = []
    try:
        for d in dets:
            mod.matching.log.clear()
            t0 = time.perf_counter()
            with _cpu_only():
                cur = trk.update_without_detection(None, img) if d is None else trk.update(np.asarray(d, dtype=np.float32), img)
            if timing is not None:
                timing.append(time.perf_counter() - t0)
            rows = [(int(t.track_id), np.asarray(t.tlwh, dtype=np.float64).copy(), float(t.cls), float(t.score)) for t in cur]
            out.append((rows, [int(t.track_id) for t in trk.tracked_stracks], [int(t.track_id) for t in trk.lost_stracks]))
            if counts is not None and d is not None:
                log = [c for c in mod.matching.log if c[0] in (0.9, 0.5, 0.7)][:3]
                if len(log) == 3:
                    (_, c0, m0, _, _), (_, _, m1, _, _), (_, _, _, ua2, _) = log
                    counts["first_matches"] += len(m0)
                    if c0.size and c0.dtype == np.float32:      # (the network ran: its costs are float32)
                        counts["first_pairs"] += c0.size
                        counts["first_rejected"] += int((c0 > 0.9).sum())
                    counts["second_matches"] += len(m1)
                    counts["unconfirmed_removed"] += len(ua2)
                # the index quirk's trace: an entry of the tracked list this frame's update did not touch but left Tracked (the unmatched track itself was not marked)
                counts["quirk_frames"] += int(any(t.state == mod.TrackState.Tracked and t.frame_id != trk.frame_id for t in trk.tracked_stracks))
    finally:
        mod.STrack.re_activate = orig_react
    if counts is not None:
        counts["reactivated"] += n_react[0]
    return out


def flat_lists(lists):
    return np.array([len(x) for x in lists], np.int32), np.array([i for x in lists for i in x], np.int32)


def same_ids(a, b):
    return all([r[0] for r in x[0]] == [r[0] for r in y[0]] and x[1] == y[1] and x[2] == y[2] for x, y in zip(a, b))


def make_dhn(mod):
    net, net64 = reference_dhn(mod, DHN_SEED, DHN_SCALE)
    recs = []
    for k, (h, w) in enumerate(DHN_SHAPES):
        D = np.random.RandomState(100 + k).uniform(0.0, 1.0, (h, w)).astype(np.float32)
        t0 = time.perf_counter()
        o32 = eval_dhn(net, D, torch.float32)
        sec = time.perf_counter() - t0
        o64 = eval_dhn(net64, D, torch.float64)
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and o32.shape == (h, w)
        recs.append((h, w, D, o32, o64, float(np.abs(o32.astype(np.float64) - o64).max()), sec))
    E = max(r[5] for r in recs)
    for h, w, D, o32, o64, e, sec in recs:
        path = os.path.join(HERE, "dhn_%dx%d.npz" % (h, w))
        np.savez_compressed(path, D=D, out32=o32, out64=o64, e_ref=np.array(e), E=np.array(E), seed=np.array(DHN_SEED), scale=np.array(DHN_SCALE), ref_seconds=np.array(sec),
                            torch_version=np.array(torch.__version__))
        print("dhn %dx%d  e_ref %.3g  output std %.3g  reference %.3f s  bytes %d" % (h, w, e, o64.std(), sec, os.path.getsize(path)), flush=True)
    print("E = %.3g -> device tolerance 4 E = %.3g" % (E, 4 * E))
    return E


def main(only=None):
    mod = load_deepmot()
    E = make_dhn(mod)
    total = {k: 0 for k in ("first_matches", "first_pairs", "first_rejected", "second_matches", "unconfirmed_removed", "reactivated", "quirk_frames")}
    for name, nf, nobj, seq, extra, conf, empty, none, kform, wseed, wscale in CASES:
        if only and name not in only:
            continue
        dets = make_scene(nf, nobj, seq, extra, empty, none)
        times, counts, net_times = [], {k: 0 for k in total}, []
        ref = run_reference(dets, mod, conf, kform, wseed, wscale, timing=times, counts=counts, net_timing=net_times)
        # the stability condition
        assert same_ids(ref, run_reference(dets, mod, conf, kform, wseed, wscale, net_mode="f64")), "%s: the ids change with the float64 network" % name
        assert same_ids(ref, run_reference(dets, mod, conf, kform, wseed, wscale, net_mode="perturb", tol=4 * E)), "%s: the ids change under +-4 E" % name
        fr, ids, tlwh, cls, score = [], [], [], [], []
        for f, (rows, _, _) in enumerate(ref):
            for r in rows:
                fr.append(f); ids.append(r[0]); tlwh.append(r[1]); cls.append(r[2]); score.append(r[3])
        tc, tl = flat_lists([x[1] for x in ref])
        lc, ll = flat_lists([x[2] for x in ref])
        for k in total:
            total[k] += counts[k]
        big = max(net_times, key=lambda x: x[0][0] * x[0][1]) if net_times else ((0, 0), 0.0)
        path = os.path.join(HERE, "tracker_deepmot_%s.npz" % name)
        np.savez_compressed(path, tracker=np.array("deepmot"), det_counts=np.array([-1 if d is None else len(d) for d in dets], np.int32),
                            dets=np.concatenate([d for d in dets if d is not None], 0).astype(np.float32), frame=np.array(fr, np.int32),
                            track_id=np.array(ids, np.int32), tlwh=np.array(tlwh, np.float64).reshape(-1, 4), cls=np.array(cls, np.float32),
                            score=np.array(score, np.float32), tracked_counts=tc, tracked_ids=tl, lost_counts=lc, lost_ids=ll, conf_thresh=np.array(conf),
                            kalman_format=np.array(kform), img_shape=np.array(IMG_SHAPE), weight_seed=np.array(wseed), weight_scale=np.array(wscale),
                            E=np.array(E), numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__),
                            ref_ms_per_frame=np.array(1e3 * float(np.median(times))), largest_net=np.array(big[0]), largest_net_seconds=np.array(big[1]),
                            **{"count_" + k: np.array(v) for k, v in counts.items()})
        print(name, "rows", len(ids), "max id", max(ids) if ids else 0, "tracked / lost at the end", tc[-1], lc[-1], "reference ms per frame (median) %.1f" % (1e3 * np.median(times)),
              "largest network %s in %.3f s" % (big[0], big[1]), counts, "bytes", os.path.getsize(path), flush=True)
    if not only:
        for k, v in total.items():
            assert v > 0, "the set has no %s" % k
        print("over the set:", total)


if __name__ == "__main__":
    assert ref_harness.available(), "needs the reference sources"
    main(sys.argv[1].split(",") if len(sys.argv) > 1 else None)
