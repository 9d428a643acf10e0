"""tests/_hostsim/botsort_reid.py -- TEST INFRASTRUCTURE ONLY: the BoT-SORT-with-appearance program (csrc/y7t_track_botsort_reid.h) of the host build
(liby7t_hostsim_botsort_reid.so, y7t_hostsim_botsort_reid.cpp): the plain forms of the frame's three launches at nt = 1, and its pinned arithmetic on its own."""
import ctypes
import os

import numpy as np

from tests import _hostsim as hs

_SO = os.path.join(hs._HERE, "liby7t_hostsim_botsort_reid.so")
_lib = None


def build(force=False):
    return hs._build(_SO, "y7t_hostsim_botsort_reid.cpp", force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, ci, cd, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
        L.hs_br_tracker_bytes.restype = sz
        L.hs_br_tracker_bytes.argtypes = [ci, ci]
        L.hs_br_tracker_init.argtypes = [vp, ci, ci, ci, ci, cd, cd, vp]
        L.hs_br_feat_bytes.restype = sz
        L.hs_br_feat_bytes.argtypes = [ci, ci, ci]
        L.hs_br_feat_init.argtypes = [vp, ci, ci, ci, cd, cd]
        L.hs_br_step.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp]
        L.hs_br_predict.argtypes = [vp, vp, ci]
        for name in ("hs_br_tracker_status", "hs_br_feat_status", "hs_br_n_dots", "hs_br_n_emb"):
            getattr(L, name).argtypes = [vp]
        L.hs_br_layout.argtypes = [ci, ci, ci, vp]
        L.hs_br_norm.restype = cd
        L.hs_br_norm.argtypes = [vp, ci]
        L.hs_br_cosine.argtypes = [vp, ci, vp, ci, ci, vp]
        L.hs_br_half.restype = cd
        L.hs_br_half.argtypes = [cd]
        L.hs_br_gate.restype = cd
        L.hs_br_gate.argtypes = [cd] * 4
        L.hs_br_set_fast_bytes.argtypes = [ci]
        L.hs_br_set_fast_bytes(int(os.environ.get("Y7T_HOSTSIM_FAST_BYTES", str(hs.FAST_BYTES))))
        _lib = L
    return _lib


def norm(x):
    """np.linalg.norm of a float32 row cast to float64, as the program pins it (numpy's pairwise sum of squares)"""
    x = np.ascontiguousarray(x, np.float32)
    return lib().hs_br_norm(x.ctypes.data, len(x))


def cosine(u, v):
    """the program's cosine (each row / its norm, then ONE sequential FMA chain) of float32 rows u (n, dim) and v (m, dim) -> (n, m) float64"""
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    out = np.zeros((len(u), len(v)), np.float64)
    lib().hs_br_cosine(u.ctypes.data, len(u), v.ctypes.data, len(v), u.shape[1], out.ctypes.data)
    return out


def half(dot):
    """0.5 * (1. - dot)"""
    return lib().hs_br_half(float(dot))


def gate(iou_d, app_half, theta_iou=0.5, theta_emb=0.25):
    """equations 12-13 on one pair: np.minimum(IoU_dist, App) after App[IoU_dist > theta_iou] = 1, App[App > theta_emb] = 1"""
    return lib().hs_br_gate(float(iou_d), float(app_half), float(theta_iou), float(theta_emb))


def feature_layout(cap_t, cap_d, dim):
    """byte offsets of the feature state's arrays + the pair table's entry count"""
    out = np.zeros(8, np.int64)
    hcap = lib().hs_br_layout(cap_t, cap_d, dim, out.ctypes.data)
    return dict(zip(("vec", "pend", "tn", "dn", "hkey", "hlist", "hval", "total"), (int(v) for v in out)), hcap=hcap)


def pair_table(fblob, cap_t, cap_d, dim):
    """the pairs of the last association that took cosines, out of a feature state's bytes -> {(row, column): 0.5 * (1 - cos)}"""
    lo = feature_layout(cap_t, cap_d, dim)
    nb = int(fblob[56:60].view(np.int32)[0])
    key = fblob[lo["hkey"]:lo["hkey"] + 4 * lo["hcap"]].view(np.int32)
    val = fblob[lo["hval"]:lo["hval"] + 8 * lo["hcap"]].view(np.float64)
    return {(int(k) // nb, int(k) % nb): float(v) for k, v in zip(key, val) if k >= 0}


class HostBoTSORTReID:
    """the pool + feature state on the host.  feature_fn(boxes (k, 4)) -> (k, dim) float32: the get_feature seam (rows with score >= conf_thresh)"""

    def __init__(self, feature_fn, feat_dim, conf_thresh=0.2, track_buffer=30, frame_rate=30, cap_t=1024, cap_d=1024, ids=None, f32_quirk=1, theta_iou=0.5,
                 theta_emb=0.25, feat_cap_t=None, feat_cap_d=None):
        L = lib()
        self.ids = ids if ids is not None else np.zeros(1, np.int32)
        self.cap_t, self.cap_d, self.dim, self.feature_fn, self.conf = cap_t, cap_d, feat_dim, feature_fn, conf_thresh
        self.blob = np.zeros(L.hs_br_tracker_bytes(cap_t, cap_d), np.uint8)
        L.hs_br_tracker_init(self.blob.ctypes.data, cap_t, cap_d, int(frame_rate / 30.0 * track_buffer), f32_quirk, conf_thresh, max(0.15, conf_thresh - 0.3), self.ids.ctypes.data)
        self.fcap_t, self.fcap_d = feat_cap_t or cap_t, feat_cap_d or cap_d
        self.fblob = np.zeros(L.hs_br_feat_bytes(self.fcap_t, self.fcap_d, feat_dim), np.uint8)
        L.hs_br_feat_init(self.fblob.ctypes.data, self.fcap_t, self.fcap_d, feat_dim, theta_iou, theta_emb)
        self.out = np.zeros((cap_t, 8), np.float64)

    def _rows(self, cnt):
        st, fs = lib().hs_br_tracker_status(self.blob.ctypes.data), self.feature_status
        if st or fs:
            raise RuntimeError("tracker refused the frame or a capacity was exceeded (status %d, feature status %d)" % (st, fs))
        return [(int(r[0]), r[1:5].copy(), float(r[5]), float(r[6])) for r in self.out[:cnt]]

    def update(self, det, warp=None):
        L = lib()
        if det is None:      # update_without_detection: the plain program's predict-only form
            return self._rows(L.hs_br_predict(self.blob.ctypes.data, self.out.ctypes.data, self.cap_t))
        det = np.ascontiguousarray(det, dtype=np.float32).reshape(-1, 6)
        feats = np.full((max(len(det), 1), self.dim), np.nan, np.float32)      # (rows below det_thresh are never read: NaN would show)
        keep = det[:, 4] >= np.float32(self.conf)
        if keep.any():
            feats[keep] = self.feature_fn(det[keep, :4])
        wp = None
        if warp is not None:
            self._warp = np.ascontiguousarray(warp, dtype=np.float64).reshape(6)
            wp = self._warp.ctypes.data
        return self._rows(L.hs_br_step(self.blob.ctypes.data, self.fblob.ctypes.data, det.ctypes.data, det.shape[0], feats.ctypes.data, self.out.ctypes.data, self.cap_t, wp))

    feature_status = property(lambda self: lib().hs_br_feat_status(self.fblob.ctypes.data))
    n_dots = property(lambda self: lib().hs_br_n_dots(self.fblob.ctypes.data))
    n_emb = property(lambda self: lib().hs_br_n_emb(self.fblob.ctypes.data))

    def vector(self, slot):
        off = feature_layout(self.fcap_t, self.fcap_d, self.dim)["vec"] + 4 * self.dim * int(slot)
        return self.fblob[off:off + 4 * self.dim].view(np.float32).copy()

    def pairs(self):
        return pair_table(self.fblob, self.fcap_t, self.fcap_d, self.dim)
