"""tests/_hostsim_deepmot -- TEST INFRASTRUCTURE ONLY: tests/_hostsim's CPU build (nt = 1) of the tracker workgroup programs plus DeepMOT's two programs
(csrc/y7t_track_deepmot.h), so that their control flow and pinned arithmetic can be tested without a GPU.  The Deep Hungarian Net between the two programs is a
callable the test supplies (the package's fp32 torch module).  Never imported by the product package."""
import ctypes
import os
import subprocess

import numpy as np

from tests import _hostsim as hs

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "liby7t_hostsim_deepmot.so")
_SRC = os.path.join(_HERE, "y7t_hostsim_deepmot.cpp")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "yolov7-tracker_amd", "csrc")
FAST_BYTES = 131072      # the device's LDS budget for the step's fast scratch (csrc/y7t_tracker.hip: kFastBytes)


def build(force=False):
    deps = [_SRC, os.path.join(os.path.dirname(_HERE), "_hostsim", "y7t_hostsim.cpp")] + \
           [os.path.join(_CSRC, h) for h in ("y7t_track_core.h", "y7t_track_step.h", "y7t_track_cbiou.h", "y7t_track_deepmot.h")]
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _SO, _SRC])      # (tests/_hostsim's flags)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.hs_tracker_bytes.restype = ctypes.c_size_t
        L.hs_tracker_bytes.argtypes = [ci, ci]
        L.hs_tracker_init.argtypes = [vp] + [ci] * 6 + [cd] * 3 + [vp]
        L.hs_tracker_step.argtypes = [vp, vp, ci, vp, ci, vp]
        L.hs_tracker_status.argtypes = [vp]
        L.hs_deepmot_front.argtypes = [vp, vp, ci, ci, ci, vp, ctypes.c_longlong]
        L.hs_deepmot_back.argtypes = [vp, vp, vp, ctypes.c_uint, vp, ci]
        L.hs_dm_ecu_iou.restype = cd
        L.hs_dm_ecu_iou.argtypes = [vp, vp, cd, ci, ci]
        L.hs_set_fast_bytes(int(os.environ.get("Y7T_HOSTSIM_FAST_BYTES", str(FAST_BYTES))))
        _lib = L
    return _lib


def ecu_iou(t_tlwh, d_tlwh, iou_d, img_shape):
    t, d = np.ascontiguousarray(t_tlwh, np.float64), np.ascontiguousarray(d_tlwh, np.float32)
    return lib().hs_dm_ecu_iou(t.ctypes.data, d.ctypes.data, float(iou_d), int(img_shape[0]), int(img_shape[1]))


class HostDeepMOT:
    """the DeepMOT pool on the host.  net(D (h, w) float32 numpy) -> (h, w) float32 numpy: the Deep Hungarian Net seam"""

    def __init__(self, net, img_shape, conf_thresh=0.2, track_buffer=30, kalman_format="default", frame_rate=30, cap_t=256, cap_d=256, ids=None, f32_quirk=1,
                 net_cap=None, kind=7):
        L = lib()
        self.ids = ids if ids is not None else np.zeros(1, np.int32)
        self.cap_t, self.cap_d, self.net, self.img_shape = cap_t, cap_d, net, img_shape
        self.blob = np.zeros(L.hs_tracker_bytes(cap_t, cap_d), np.uint8)
        L.hs_tracker_init(self.blob.ctypes.data, kind, hs.HostSimTracker.KINDS[kalman_format], cap_t, cap_d, int(frame_rate / 30.0 * track_buffer), f32_quirk,
                          conf_thresh, max(0.15, conf_thresh - 0.3), 0.5, self.ids.ctypes.data)
        self.net_cap = cap_t * cap_d if net_cap is None else net_cap
        self.D = np.zeros(max(self.net_cap, 1), np.float32)
        self.out = np.zeros((cap_t, 8), np.float64)
        self.net_shapes, self.net_status = [], 0      # the matrices the network ran on; a status to hand the back program (tests of the give-up path)
        self.last_D = None

    def status(self):
        return lib().hs_tracker_status(self.blob.ctypes.data)

    def _rows(self, cnt):
        st = self.status()
        if st:
            raise RuntimeError("tracker status %d" % st)
        return [(int(r[0]), r[1:5].copy(), float(r[5]), float(r[6])) for r in self.out[:cnt]]

    def update(self, det):
        L = lib()
        if det is None:      # update_without_detection: the plain program's predict-only form (what y7t_tracker_step(state, NULL, -1, ...) launches for this kind)
            return self._rows(L.hs_tracker_step(self.blob.ctypes.data, None, -1, self.out.ctypes.data, self.cap_t, None))
        det = np.ascontiguousarray(det, dtype=np.float32).reshape(-1, 6)
        hw = L.hs_deepmot_front(self.blob.ctypes.data, det.ctypes.data, det.shape[0], int(self.img_shape[0]), int(self.img_shape[1]), self.D.ctypes.data, self.net_cap)
        h, w = hw >> 16, hw & 0xffff
        out = np.zeros(1, np.float32)
        if h and w:
            self.last_D = self.D[:h * w].reshape(h, w).copy()
            self.net_shapes.append((h, w))
            out = np.ascontiguousarray(self.net(self.last_D), np.float32)
            assert out.shape == (h, w)
        return self._rows(L.hs_deepmot_back(self.blob.ctypes.data, det.ctypes.data, out.ctypes.data, self.net_status, self.out.ctypes.data, self.cap_t))
