"""tests/_hostsim/map.py -- TEST INFRASTRUCTURE ONLY: the host build of csrc/y7t_map.h (y7t_hostsim_map.cpp, -DY7T_HOSTSIM): the per-image matching and the
per-(class, threshold) curve program the device's workgroups run, so that both can be tested without a GPU.  HostMAP takes the arrays y7t_map_update takes."""
import ctypes
import os

import numpy as np

from tests._hostsim import _HERE, _build

_SO = os.path.join(_HERE, "liby7t_hostsim_map.so")
_lib = None
NIOU = 10


def build_map(force=False):
    return _build(_SO, "y7t_hostsim_map.cpp", defs=["-DY7T_HOSTSIM"], force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_map())
        vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
        L.hs_map_bytes.restype = sz
        L.hs_map_bytes.argtypes = [ci, ci]
        L.hs_map_layout.argtypes = [ci, ci, vp]
        L.hs_map_linspace01.restype = ctypes.c_double
        L.hs_map_linspace01.argtypes = [ci, ci]
        L.hs_map_iou.restype = cf
        L.hs_map_iou.argtypes = [vp, vp]
        L.hs_map_target_box.argtypes = [vp, cf, cf, vp, vp]
        L.hs_map_scale_coords.argtypes = [vp, vp]
        L.hs_map_init.argtypes = [vp, ci, ci]
        L.hs_map_update.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp]
        L.hs_map_compute.argtypes = [vp] * 9
        _lib = L
    return _lib


def iou(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.float32(lib().hs_map_iou(a.ctypes.data, b.ctypes.data))


def target_box(row, W, H, lb):
    row, lb, out = np.ascontiguousarray(row, np.float32), np.ascontiguousarray(lb, np.float32), np.zeros(4, np.float32)
    lib().hs_map_target_box(row.ctypes.data, float(W), float(H), lb.ctypes.data, out.ctypes.data)
    return out


def scale_coords(box, lb):
    box, lb = np.array(box, np.float32), np.ascontiguousarray(lb, np.float32)
    lib().hs_map_scale_coords(box.ctypes.data, lb.ctypes.data)
    return box


def linspace01(n):
    return np.array([lib().hs_map_linspace01(q, n) for q in range(n)])


class HostMAP:
    def __init__(self, nc, cap_rows):
        self.nc, self.cap = int(nc), int(cap_rows)
        self.state = np.zeros(int(lib().hs_map_bytes(self.cap, self.nc)) + 256, np.uint8)
        off = (ctypes.c_size_t * 4)()
        lib().hs_map_layout(self.cap, self.nc, off)
        self._off = dict(zip(("nt", "conf", "cls", "correct"), (int(v) for v in off)))
        self.reset()

    def reset(self):
        lib().hs_map_init(self.state.ctypes.data, self.cap, self.nc)

    def header(self):
        return self.state[:256].view(np.int32)

    def update_raw(self, dets, ndets, keep, cbox, targets, toff, hw, lb, iouv):
        """the arguments of y7t_map_update as NumPy arrays: dets (B, max_det, 6), ndets (B,), keep (B, max_det), cbox (B, cap, 4), targets (L, 6), toff (B + 1,)"""
        f32, i32 = (lambda a: np.ascontiguousarray(a, np.float32)), (lambda a: np.ascontiguousarray(a, np.int32))
        dets, ndets, keep, cbox, toff, lb, iouv = f32(dets), i32(ndets), i32(keep), f32(cbox), i32(toff), f32(lb), f32(iouv)
        targets = f32(targets).reshape(-1, 6)
        tg = targets if len(targets) else np.zeros((1, 6), np.float32)
        lib().hs_map_update(self.state.ctypes.data, dets.ctypes.data, ndets.ctypes.data, keep.ctypes.data, cbox.ctypes.data, cbox.shape[1], cbox.shape[1], len(ndets),
                            dets.shape[1], tg.ctypes.data, toff.ctypes.data, int(hw[0]), int(hw[1]), lb.ctypes.data, iouv.ctypes.data)

    def rows(self):
        n = int(self.header()[0])
        v = lambda k, dt: self.state[self._off[k]:self._off[k] + 4 * self.cap].view(dt)[:n].copy()
        mask = v("correct", np.int32)
        nt = self.state[self._off["nt"]:self._off["nt"] + 8 * self.nc].view(np.int64).copy()
        return v("conf", np.float32), v("cls", np.int32), ((mask[:, None] >> np.arange(NIOU)) & 1).astype(bool), nt

    def compute_raw(self):
        n = int(self.header()[0])
        ap, p, r = np.zeros((self.nc, NIOU)), np.zeros((self.nc, 1000)), np.zeros((self.nc, 1000))
        nt, cl, info = np.zeros(self.nc, np.int64), np.zeros(self.nc, np.int32), np.zeros(4, np.int32)
        order, tpc = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), NIOU), np.int32)
        lib().hs_map_compute(self.state.ctypes.data, ap.ctypes.data, p.ctypes.data, r.ctypes.data, nt.ctypes.data, cl.ctypes.data, info.ctypes.data, order.ctypes.data,
                             tpc.ctypes.data)
        return dict(ap=ap, p=p, r=r, nt=nt, classes=cl[:int(info[3])], rows=int(info[0]), seen=int(info[1]), status=int(info[2]), order=order[:n], tpc=tpc[:n])
