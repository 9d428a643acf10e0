"""tests/_hostsim/orb.py -- TEST INFRASTRUCTURE ONLY: the feature-estimator bodies of csrc/y7t_orb.h of the host build (y7t_hostsim_orb.cpp), one item at a time into
the device's workspace and state layout, so that the camera-motion estimate and every intermediate array can be tested without a GPU."""
import ctypes
import os

import numpy as np

from tests._hostsim import _HERE, _build

_SO_ORB = os.path.join(_HERE, "liby7t_hostsim_orb.so")
_lib = None


def build_orb(force=False):
    return _build(_SO_ORB, "y7t_hostsim_orb.cpp", force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_orb())
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.hs_orb_layout.argtypes = [ci, ci, ci, vp]
        L.hs_orb_state_bytes.restype = ctypes.c_size_t
        L.hs_orb_state_bytes.argtypes = [ci]
        L.hs_orb_extract.argtypes = [vp, ci, ci, ci, vp, ci, ci, vp, vp]
        L.hs_orb_estimate.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp]
        L.hs_orb_ransac.argtypes = [vp, ci, ci, vp, vp, vp]
        L.hs_orb_pick.argtypes = [ci, ci, ci]
        _lib = L
    return _lib


def layout(h, w, cap):
    off = np.zeros(12, np.uint64)
    lib().hs_orb_layout(h, w, cap, off.ctypes.data)
    return [int(v) for v in off]


def dets6(dets):
    """(n, >= 4) -> (n, 6) float32 rows as the tracker step takes them"""
    if dets is None or len(dets) == 0:
        return np.zeros((0, 6), np.float32)
    d = np.asarray(dets, np.float32)
    out = np.zeros((len(d), 6), np.float32)
    out[:, :min(6, d.shape[1])] = d[:, :6]
    return out


def read_taps(ws, state, h, w, cap):
    """the arrays of a workspace and a state (uint8 NumPy buffers) by name, shaped as tests/orb_np.py has them"""
    off = layout(h, w, cap)
    hdr = state[:32].view(np.int32)
    n = int(hdr[0])

    def img(k):
        return ws[off[k]:off[k] + h * w].reshape(h, w)
    est = ws[off[9]:off[9] + 32].view(np.int32)
    return dict(plane=img(0), scores=img(1), keep=img(2).astype(bool), smooth=img(3), rowcnt=ws[off[4]:off[4] + 4 * h].view(np.int32),
                moments=ws[off[6]:off[6] + 8 * n].view(np.int32).reshape(n, 2).astype(np.int64),
                n=n, total=int(hdr[1]), truncated=int(hdr[2]), h=int(hdr[3]), w=int(hdr[4]),
                desc=state[32:32 + 32 * n].view(np.uint32).reshape(n, 8),
                kp=state[32 + 32 * cap:32 + 32 * cap + 8 * n].view(np.int32).reshape(n, 2).astype(np.int64),
                matches=ws[off[7]:off[7] + 16 * cap].view(np.int32).reshape(cap, 4).astype(np.int64),
                good=ws[off[8]:off[8] + 16 * cap].view(np.int32).reshape(cap, 4).astype(np.int64),
                est=dict(zip(("n_good", "flag", "n_first", "winner", "n_inliers"), (int(v) for v in est[:5]))),
                counts=ws[off[10]:off[10] + 4 * 2000].view(np.int32).astype(np.int64))


class HostFeatures:
    """the estimator's backend on the host: what tracker/gmc.py's _DeviceFeatures does through liby7t.so (the `backend=` seam of GMC)"""

    def __init__(self):
        lib()
        self._ws = {}

    def workspace(self, h, w, cap):
        if (h, w, cap) not in self._ws:
            self._ws[(h, w, cap)] = np.zeros(layout(h, w, cap)[11] + 16, np.uint8)
        return self._ws[(h, w, cap)]

    def extract(self, frame, downscale, dets, cap, state=None):
        if hasattr(frame, "cpu"):
            frame = frame.cpu().numpy()
        if hasattr(dets, "cpu"):
            dets = dets.cpu().numpy()
        frame = np.ascontiguousarray(frame, np.uint8)
        H, W = frame.shape[:2]
        d = dets6(dets)
        if state is None:
            state = np.zeros(lib().hs_orb_state_bytes(cap), np.uint8)
        ws = self.workspace(H // downscale, W // downscale, cap)
        lib().hs_orb_extract(frame.ctypes.data, H, W, int(downscale), d.ctypes.data if len(d) else None, len(d), cap, ws.ctypes.data, state.ctypes.data)
        return state

    def estimate(self, prev, cur, h, w, downscale, cap):
        out = np.zeros(12, np.float64)
        ws = self.workspace(h, w, cap)
        lib().hs_orb_estimate(prev.ctypes.data, cur.ctypes.data, h, w, int(downscale), cap, ws.ctypes.data, out.ctypes.data, out.ctypes.data + 48)
        return out[:6], out[6:]


def ransac(good, ds=2):
    """the hypotheses and the refinement over (n, 4) matches -> (counts (2000,), est dict, warp (6,))"""
    lib()
    g = np.ascontiguousarray(good, np.int32)
    counts, est, warp = np.zeros(2000, np.int32), np.zeros(5, np.int32), np.zeros(6, np.float64)
    lib().hs_orb_ransac(g.ctypes.data, len(g), ds, counts.ctypes.data, est.ctypes.data, warp.ctypes.data)
    return counts.astype(np.int64), dict(zip(("n_good", "flag", "n_first", "winner", "n_inliers"), (int(v) for v in est))), warp
