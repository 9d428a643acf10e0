"""tests/_hostsim/deepmot.py -- TEST INFRASTRUCTURE ONLY: DeepMOT's two programs (csrc/y7t_track_deepmot.h) of the host build.  The Deep Hungarian Net between
the two programs is a callable the test supplies (the package's fp32 torch module)."""
import numpy as np

from tests._hostsim import HostSimTracker, lib


_NETS = {}


def torch_net(seed, scale):
    """the package's torch module with the seeded weights as a numpy -> numpy callable (built once per weight set, never modified)"""
    import torch
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker.deepmot import TorchDHN
    key = (int(seed), float(scale))
    if key not in _NETS:
        net = TorchDHN(synth.make_dhn_weights(*key))
        _NETS[key] = lambda D, _n=net: _n(torch.from_numpy(np.ascontiguousarray(D, np.float32))).numpy()
    return _NETS[key]


def ecu_iou(t_tlwh, d_tlwh, iou_d, img_shape):
    t, d = np.ascontiguousarray(t_tlwh, np.float64), np.ascontiguousarray(d_tlwh, np.float32)
    return lib().hs_dm_ecu_iou(t.ctypes.data, d.ctypes.data, float(iou_d), int(img_shape[0]), int(img_shape[1]))


class HostDeepMOT:
    """the DeepMOT pool on the host.  net(D (h, w) float32 numpy) -> (h, w) float32 numpy: the Deep Hungarian Net seam"""

    def __init__(self, net, img_shape, conf_thresh=0.2, track_buffer=30, kalman_format="default", frame_rate=30, cap_t=256, cap_d=256, ids=None, f32_quirk=1,
                 net_cap=None, kind="deepmot"):
        L = lib()
        self.ids = ids if ids is not None else np.zeros(1, np.int32)
        self.cap_t, self.cap_d, self.net, self.img_shape = cap_t, cap_d, net, img_shape
        self.blob = np.zeros(L.hs_tracker_bytes(cap_t, cap_d), np.uint8)
        L.hs_tracker_init(self.blob.ctypes.data, HostSimTracker.TRACKERS[kind], HostSimTracker.KINDS[kalman_format], cap_t, cap_d, int(frame_rate / 30.0 * track_buffer), f32_quirk,
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
