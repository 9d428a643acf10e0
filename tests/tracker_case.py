"""What the per-tracker test files (test_c_biou_*, test_uavmot_*, test_strongsort_*, test_deepmot_*) share: the reference's golden vectors of a tracker kind, the
frame-by-frame comparison of a host pool (tests/_hostsim) or a device tracker with them, and the construction of device trackers and raw device pools."""
import ctypes
import importlib.util
import os
import types

import numpy as np

from tests import _hostsim as hs
from tests import util

GOLDEN = util.GOLDEN
LIB = os.path.join(os.path.dirname(GOLDEN), "..", "yolov7-tracker_amd", "lib", "liby7t.so")
NAMES = {"c_biou": ["default", "bounce", "misses", "crowd", "empty", "conf04"],
         "uavmot": ["default", "misses", "sparse1", "sparse3", "crowd", "empty", "conf04", "botsort"],
         "strongsort": ["identity128", "identity512", "dim100", "boxfeat", "crowd300", "crowd500", "gamma05", "conf04", "empty", "gaps"],
         "deepmot": ["default", "miss", "conf04", "empty", "gaps", "reject", "crowd"]}
DHN_NAMES = ["1x1", "1x7", "7x1", "3x5", "12x9", "33x20", "64x48"]      # tests/golden/dhn_<name>.npz: the Deep Hungarian Net alone
DEEPMOT_COUNTS = ["first_matches", "first_rejected", "second_matches", "unconfirmed_removed", "reactivated", "quirk_frames"]


def maker(kind):
    """tests/golden/make_golden_<kind>.py as a module: the scenes' generators (and, where the reference exists, its runner)"""
    spec = importlib.util.spec_from_file_location("make_golden_" + kind, os.path.join(GOLDEN, "make_golden_%s.py" % kind))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


# ---- the golden vectors ----
def _plain_dets(g):
    off = np.concatenate([[0], np.cumsum(g["det_counts"])])
    return [g["dets"][off[i]:off[i + 1]] for i in range(len(g["det_counts"]))]


def _strongsort_keys(g):
    dets, fn, warps = maker("strongsort").scene_from_golden(g)
    return dict(dets=dets, feature_fn=fn, warps=warps, dim=int(g["feat_dim"]), gamma=float(g["gamma"]), final_ids=g["final_slots_ids"].tolist(),
                final_features=g["final_features"], stale=g["stale_counts"], both=g["both_counts"], ref_ms=float(g["ref_ms_per_frame"]),
                kalman_format=str(g["kalman_format"]))


def _deepmot_keys(g):
    return dict(dets=maker("deepmot").frames_from_golden(g), kalman_format=str(g["kalman_format"]), img_shape=tuple(int(v) for v in g["img_shape"]),
                seed=int(g["weight_seed"]), scale=float(g["weight_scale"]), counts={k: int(g["count_" + k]) for k in DEEPMOT_COUNTS}, E=float(g["E"]))


_KIND_KEYS = {"c_biou": lambda g: dict(dets=_plain_dets(g)),
              "uavmot": lambda g: dict(dets=_plain_dets(g), kalman_format=str(g["kalman_format"])),
              "strongsort": _strongsort_keys, "deepmot": _deepmot_keys}


def load_golden(kind, name):
    """tests/golden/tracker_<kind>_<name>.npz -> dets, per frame (ids, tlwh, cls, score) and the tracked / lost id lists, conf, + the kind's own keys"""
    g = np.load(os.path.join(GOLDEN, "tracker_%s_%s.npz" % (kind, name)))
    want = _KIND_KEYS[kind](g)

    def split(counts, flat):
        o = np.concatenate([[0], np.cumsum(counts)])
        return [flat[o[i]:o[i + 1]].tolist() for i in range(len(counts))]
    frames = []
    for f in range(len(want["dets"])):
        sel = g["frame"] == f
        frames.append((g["track_id"][sel], g["tlwh"][sel], g["cls"][sel], g["score"][sel]))
    want.update(frames=frames, tracked=split(g["tracked_counts"], g["tracked_ids"]), lost=split(g["lost_counts"], g["lost_ids"]), conf=float(g["conf_thresh"]))
    return want


def want_from_reference(ref, **keys):
    """the frames of a live reference run [(rows, tracked ids, lost ids), ...] in load_golden's form"""
    return dict(keys, tracked=[t for _, t, _ in ref], lost=[lo for _, _, lo in ref],
                frames=[(np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float64).reshape(-1, 4),
                         np.array([r[2] for r in rows], np.float32), np.array([r[3] for r in rows], np.float32)) for rows, _, _ in ref])


# ---- the pool blob ----
_LAYOUT = {}


def layout(cap_t, cap_d):
    """byte offsets of the pool blob's fields (the product library's y7t_tracker_layout: host code, no device needed)"""
    if (cap_t, cap_d) not in _LAYOUT:
        L = ctypes.CDLL(LIB)
        L.y7t_tracker_layout.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.y7t_tracker_field_name.restype = ctypes.c_char_p
        n = L.y7t_tracker_layout(cap_t, cap_d, None, 0)
        offs = (ctypes.c_int64 * n)()
        L.y7t_tracker_layout(cap_t, cap_d, offs, n)
        _LAYOUT[(cap_t, cap_d)] = {L.y7t_tracker_field_name(i).decode(): int(offs[i]) for i in range(n)}
    return _LAYOUT[(cap_t, cap_d)]


def id_lists(t):
    """-> (ids of the tracked list, ids of the lost list) in list order, of a host pool (tests/_hostsim: `blob`) or of a device tracker (its snapshot)"""
    if not hasattr(t, "blob"):
        s = t._snapshot()
        return s["tid"][s["tracked"][:s["hdr_n_tracked"]]].tolist(), s["tid"][s["lost"][:s["hdr_n_lost"]]].tolist()
    lo, b = layout(t.cap_t, t.cap_d), t.blob
    i32 = lambda off, n: b[off:off + 4 * n].view(np.int32)      # noqa: E731
    tid = i32(lo["tid"], t.cap_t)
    nt, nl = int(i32(lo["hdr_n_tracked"], 1)[0]), int(i32(lo["hdr_n_lost"], 1)[0])
    return tid[i32(lo["tracked"], nt)].tolist(), tid[i32(lo["lost"], nl)].tolist()


def slot_of(trk, track_id):
    """the slot of a host pool's tracked list that holds `track_id`"""
    lo = layout(trk.cap_t, trk.cap_d)
    tid = trk.blob[lo["tid"]:lo["tid"] + 4 * trk.cap_t].view(np.int32)
    nt = int(trk.blob[lo["hdr_n_tracked"]:lo["hdr_n_tracked"] + 4].view(np.int32)[0])
    tracked = trk.blob[lo["tracked"]:lo["tracked"] + 4 * nt].view(np.int32)
    hit = [int(s) for s in tracked if tid[s] == track_id]
    assert len(hit) == 1, track_id
    return hit[0]


# ---- a frame against the golden / the reference ----
def check_rows(rows, want, f, exact):
    """rows [(id, tlwh, cls, score), ...] of frame f: ids, classes and scores exactly; tlwh exactly (C-BIoU: no Kalman filter) or at util's tolerance (the Kalman
    arithmetic matches the reference to it, as for ByteTrack: tests/test_hostsim.py)"""
    ids, tlwh, cls, score = want["frames"][f]
    assert [r[0] for r in rows] == ids.tolist(), "frame %d: ids" % f
    got = np.array([r[1] for r in rows], np.float64).reshape(-1, 4)
    if exact:
        assert np.array_equal(got, tlwh), "frame %d: tlwh" % f
    else:
        np.testing.assert_allclose(got, tlwh, rtol=util.TLWH_RTOL, atol=util.TLWH_ATOL, err_msg="frame %d: tlwh" % f)
    assert np.array_equal(np.array([r[2] for r in rows], np.float32), cls) and np.array_equal(np.array([r[3] for r in rows], np.float32), score), "frame %d" % f


def check_tracks(cur, want, f, exact, lists=None):
    """the track views a device tracker's update() returned for frame f; lists: its (tracked ids, lost ids), compared too"""
    check_rows([(t.track_id, t.tlwh, t.cls, t.score) for t in cur], want, f, exact)
    if lists is not None:
        assert lists == (want["tracked"][f], want["lost"][f]), "frame %d: tracked / lost lists" % f


def replay_host(trk, want, arena_frames=0, n_frames=None, exact=False):
    """step the host pool `trk` over want["dets"] (with want["warps"], if any) and compare every frame's rows and lists with `want` -> the frames' rows.
    arena_frames > 0: groups of that many frames run with the index lists in the launch-long arena, like the frames of one k_tracker_step_frames launch"""
    dets, warps, got = want["dets"][:n_frames], want.get("warps"), []
    for f, d in enumerate(dets):
        if arena_frames and f % arena_frames == 0:
            assert hs.lib().hs_arena_begin(trk.blob.ctypes.data)
        rows = trk.update(d) if warps is None else trk.update(d, warps[f])
        group_end = not arena_frames or f % arena_frames == arena_frames - 1 or f == len(dets) - 1
        if arena_frames and group_end:
            hs.lib().hs_arena_end(trk.blob.ctypes.data)
        got.append(rows)
        check_rows(rows, want, f, exact)
        if group_end:      # (inside an arena group the lists live in the arena)
            assert id_lists(trk) == (want["tracked"][f], want["lost"][f]), "frame %d: tracked / lost lists" % f
    return got


# ---- device trackers and raw device pools ----
def opts(conf=0.2, threads=0, kalman_format="default", **kw):
    o = types.SimpleNamespace(conf_thresh=conf, track_buffer=30, kalman_format=kalman_format, img_size=1280, iou_thresh=0.5, tracker_threads=threads)
    o.__dict__.update(kw)
    return o


def new_tracker(cls, conf=0.2, threads=0, kalman_format="default", feature_fn=None, ctor=None, **kw):
    """a device tracker of class `cls` on opts(conf, threads, kalman_format, **kw), the track ids starting at 1.  ctor: further constructor arguments;
    feature_fn(tlbrs) -> (n, D): injected at the get_feature seam"""
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    t = cls(opts(conf, threads, kalman_format, **kw), frame_rate=30, **(ctor or {}))
    if feature_fn is not None:
        t.get_feature = lambda tlbrs, ori_img, _fn=feature_fn: _fn(tlbrs)
    return t


def raw_pool(kind, cap=256, kalman=0):
    """a pool of tracker `kind` (a name of hs.HostSimTracker.TRACKERS) initialised through the C ABI -> (library, state blob, id counter, out rows)"""
    import torch
    from yolov7_tracker_amd import _lib
    L = _lib.load()
    nbytes = int(L.y7t_tracker_state_bytes(cap, cap))
    st = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.y7t_tracker_init(_lib.ptr(st), nbytes, hs.HostSimTracker.TRACKERS[kind], kalman, cap, cap, 0.2, 0.5, 30, 1, _lib.ptr(ids), _lib.stream_ptr()))
    out = torch.zeros((cap + 1, 8), dtype=torch.float64, device="cuda")
    return L, st, ids, out


def pool_status(L, st, cap=256):
    """the status word of a raw device pool"""
    import torch
    off = layout(cap, cap)["hdr_status"]
    return int(st[off:off + 4].view(torch.int32).item())
