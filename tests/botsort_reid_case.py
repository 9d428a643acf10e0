"""What tests/test_botsort_reid_cpu.py and tests/test_botsort_reid_gpu.py share: the reference's golden vectors of BoT-SORT with its appearance branch
(tests/golden/tracker_botsort_reid_*.npz, scenes regenerated from their seeds), the host pool of the same program, numpy restatements of its pinned arithmetic,
and raw device pools of the new tracker kind.  Built on tests/tracker_case.py's generic functions."""
import os

import numpy as np

from tests import tracker_case as tc
from tests._hostsim import botsort_reid as hbr

KIND = 8      # include/y7t.h: Y7T_TRACKER_BOTSORT_REID
KALMAN_BOTSORT = 2
_maker = None


def maker():
    global _maker
    if _maker is None:
        _maker = tc.maker("botsort_reid")
    return _maker


def names():
    return maker().NAMES


_GOLDEN = {}


def load_golden(name):
    """tests/golden/tracker_botsort_reid_<name>.npz in tracker_case.load_golden's form, + the scene (dets, feature_fn, warps) and the file's own records.
    Loaded once and shared: nothing in it is written to."""
    if name not in _GOLDEN:
        g = np.load(os.path.join(tc.GOLDEN, "tracker_botsort_reid_%s.npz" % name))
        dets, fn, warps = maker().scene_from_golden(g)

        def split(counts, flat):
            o = np.concatenate([[0], np.cumsum(counts)])
            return [flat[o[i]:o[i + 1]].tolist() for i in range(len(counts))]
        frames = []
        for f in range(len(dets)):
            sel = g["frame"] == f
            frames.append((g["track_id"][sel], g["tlwh"][sel], g["cls"][sel], g["score"][sel]))
        _GOLDEN[name] = dict(dets=dets, feature_fn=fn, warps=warps, dim=int(g["feat_dim"]), conf=float(g["conf_thresh"]), frames=frames,
                             tracked=split(g["tracked_counts"], g["tracked_ids"]), lost=split(g["lost_counts"], g["lost_ids"]),
                             final_ids=g["final_slots_ids"].tolist(), final_features=g["final_features"], gate_counts=g["gate_counts"],
                             evaluated=g["evaluated_pairs"].tolist(), margin_iou=float(g["margin_iou"]), margin_emb=float(g["margin_emb"]),
                             differs=int(g["frames_differing_from_state_path"]), ref_ms=float(g["ref_ms_per_frame"]))
    return _GOLDEN[name]


def host_tracker(g, **kw):
    return hbr.HostBoTSORTReID(g["feature_fn"], g["dim"], conf_thresh=g["conf"], **kw)


def np_norm(x):
    """np.linalg.norm(axis=1) of float32 rows cast to float64, as matching.cal_cosine_distance takes it"""
    return np.linalg.norm(np.asarray(x, np.float32).astype(np.float64), axis=1, keepdims=True)


def np_cosine(u, v):
    """cal_cosine_distance(u, v) of float32 rows: numpy's own (np.dot = the BLAS's dgemm)"""
    u, v = np.asarray(u, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    u, v = u / np.linalg.norm(u, axis=1, keepdims=True), v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.dot(u, v.T)


def np_chain_cosine(u, v):
    """the same with np.dot replaced by ONE sequential FMA chain per pair, emulated exactly: a product of two doubles splits into its rounded value and an exact
    remainder (Dekker / Veltkamp), and s + p + e is rounded once through two-sum -- slow, for small inputs"""
    import math
    u, v = np.asarray(u, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    u, v = u / np.linalg.norm(u, axis=1, keepdims=True), v / np.linalg.norm(v, axis=1, keepdims=True)
    from fractions import Fraction
    out = np.zeros((len(u), len(v)))
    for i in range(len(u)):
        for j in range(len(v)):
            s = 0.0
            for a, b in zip(u[i].tolist(), v[j].tolist()):
                s = float(Fraction(a) * Fraction(b) + Fraction(s))      # (exact rational arithmetic, one rounding: what fma does)
            out[i, j] = s
    return out


def np_gate(iou_d, half, theta_iou=0.5, theta_emb=0.25):
    """botsort.py:387-392 on arrays"""
    app = np.array(half, np.float64, copy=True)
    iou_d = np.asarray(iou_d, np.float64)
    app[iou_d > theta_iou] = 1
    app[app > theta_emb] = 1
    return np.minimum(iou_d, app)


def raw_pool(cap=256):
    """a pool of the new kind initialised through the C ABI -> (library, state blob, id counter, out rows)"""
    import torch
    from yolov7_tracker_amd import _lib
    L = _lib.load()
    nbytes = int(L.y7t_tracker_state_bytes(cap, cap))
    st = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.y7t_tracker_init(_lib.ptr(st), nbytes, KIND, KALMAN_BOTSORT, cap, cap, 0.2, 0.5, 30, 1, _lib.ptr(ids), _lib.stream_ptr()))
    out = torch.zeros((cap + 1, 8), dtype=torch.float64, device="cuda")
    return L, st, ids, out


def raw_feature_state(L, cap=256, dim=128):
    import torch
    from yolov7_tracker_amd import _lib
    nb = int(L.y7t_botsort_reid_feature_bytes(cap, cap, dim))
    feat = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_botsort_reid_init(_lib.ptr(feat), nb, cap, cap, dim, 0.5, 0.25, _lib.stream_ptr()))
    return feat
