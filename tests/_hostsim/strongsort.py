"""tests/_hostsim/strongsort.py -- TEST INFRASTRUCTURE ONLY: the StrongSORT program (csrc/y7t_track_strongsort.h) of the host build: the plain forms of the frame's
three launches at nt = 1, and its pinned arithmetic on its own."""
import numpy as np

from tests._hostsim import HostSimTracker, lib


def cdist(u, v):
    """the program's embedding distance (float64 chain per pair) of float32 rows u (n, dim) and v (m, dim)"""
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    out = np.zeros((len(u), len(v)), np.float64)
    lib().hs_ss_cdist(u.ctypes.data, len(u), v.ctypes.data, len(v), u.shape[1], out.ctypes.data)
    return out


def ema(prev, raw):
    """STrack.update's moving average as the store kernel's plain form computes it -> the new float32 vector"""
    vec, raw = np.array(prev, np.float32), np.ascontiguousarray(raw, np.float32)
    lib().hs_ss_ema(vec.ctypes.data, raw.ctypes.data, len(vec))
    return vec


class HostStrongSORT:
    """the StrongSORT pool + feature state on the host.  feature_fn(boxes (k, 4)) -> (k, dim) float32: the get_feature seam"""

    def __init__(self, feature_fn, feat_dim, conf_thresh=0.2, track_buffer=30, kalman_format="default", gamma=0.1, frame_rate=30, cap_t=1024, cap_d=1024,
                 ids=None, f32_quirk=1, feat_cap_t=None, feat_cap_d=None):
        L = lib()
        self.ids = ids if ids is not None else np.zeros(1, np.int32)
        self.cap_t, self.cap_d, self.dim, self.feature_fn, self.conf = cap_t, cap_d, feat_dim, feature_fn, conf_thresh
        self.blob = np.zeros(L.hs_tracker_bytes(cap_t, cap_d), np.uint8)
        L.hs_tracker_init(self.blob.ctypes.data, HostSimTracker.TRACKERS["strongsort"], HostSimTracker.KINDS[kalman_format], cap_t, cap_d, int(frame_rate / 30.0 * track_buffer), f32_quirk,
                          conf_thresh, max(0.15, conf_thresh - 0.3), 0.5, self.ids.ctypes.data)
        self.fcap_t, self.fcap_d = feat_cap_t or cap_t, feat_cap_d or cap_d
        self.fblob = np.zeros(L.hs_ss_feat_bytes(self.fcap_t, self.fcap_d, feat_dim), np.uint8)
        L.hs_ss_feat_init(self.fblob.ctypes.data, self.fcap_t, self.fcap_d, feat_dim, gamma)
        self.out = np.zeros((cap_t, 8), np.float64)

    def _rows(self, cnt):
        st, fs = lib().hs_tracker_status(self.blob.ctypes.data), lib().hs_ss_feat_status(self.fblob.ctypes.data)
        if st or fs:
            raise RuntimeError("tracker capacity exceeded (status %d, feature status %d)" % (st, fs))
        return [(int(r[0]), r[1:5].copy(), float(r[5]), float(r[6])) for r in self.out[:cnt]]

    def update(self, det, warp=None):
        L = lib()
        if det is None:      # update_without_detection: the program's predict-only form (what y7t_tracker_step(state, NULL, -1, ...) launches for this kind)
            return self._rows(L.hs_strongsort_predict(self.blob.ctypes.data, self.out.ctypes.data, self.cap_t))
        det = np.ascontiguousarray(det, dtype=np.float32).reshape(-1, 6)
        feats = np.full((max(len(det), 1), self.dim), np.nan, np.float32)      # (rows at or below det_thresh are never read: NaN would show)
        keep = det[:, 4] > np.float32(self.conf)
        if keep.any():
            feats[keep] = self.feature_fn(det[keep, :4])
        wp = None
        if warp is not None:
            self._warp = np.ascontiguousarray(warp, dtype=np.float64).reshape(6)
            wp = self._warp.ctypes.data
        return self._rows(L.hs_strongsort_step(self.blob.ctypes.data, self.fblob.ctypes.data, det.ctypes.data, det.shape[0], feats.ctypes.data,
                                               self.out.ctypes.data, self.cap_t, wp))

    def vector(self, slot):
        off = lib().hs_ss_vec_offset(self.fcap_t, self.fcap_d, self.dim) + 4 * self.dim * int(slot)
        return self.fblob[off:off + 4 * self.dim].view(np.float32).copy()
