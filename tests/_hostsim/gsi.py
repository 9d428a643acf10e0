"""tests/_hostsim/gsi.py -- TEST INFRASTRUCTURE ONLY: the host build of csrc/y7t_gsi.h (y7t_hostsim_gsi.cpp): the interpolation and the per-track smoother the
device's workgroups run, so that both and tracker/gsi.py's host side can be tested without a GPU.  HostGSI stands in for tracker.gsi.DeviceGSI."""
import ctypes
import os

import numpy as np

from tests._hostsim import _HERE, _build

_SO = os.path.join(_HERE, "liby7t_hostsim_gsi.so")
_lib = None


def build_gsi(force=False):
    return _build(_SO, "y7t_hostsim_gsi.cpp", force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_gsi())
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.hs_gsi_interpolate.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.hs_gsi_interpolate.restype = None
        L.hs_gsi_smooth.argtypes = [vp, vp, vp, ci, ci, cd, vp, vp]
        L.hs_gsi_smooth.restype = None
        _lib = L
    return _lib


def constants():
    return dict(lds_len=int(lib().hs_gsi_lds_len()), max_len=int(lib().hs_gsi_max_len()))


def interpolate(runs, offsets, interval=20, max_rows=1 << 16, max_len=4096):
    """-> dict(runs (count, 5), offsets (N + 1,), src (count,), count, status)"""
    runs = np.ascontiguousarray(runs, np.float64).reshape(-1, 5)
    offsets = np.ascontiguousarray(offsets, np.int32)
    out, off2, src = np.zeros((max_rows, 5), np.float64), np.zeros(len(offsets), np.int32), np.zeros(max_rows, np.int32)
    head = np.zeros(2, np.int32)
    lib().hs_gsi_interpolate(runs.ctypes.data, offsets.ctypes.data, len(offsets) - 1, int(interval), max_rows, max_len, out.ctypes.data, off2.ctypes.data, src.ctypes.data,
                             head.ctypes.data, head.ctypes.data + 4)
    m = min(int(head[0]), max_rows)
    return dict(runs=out[:m], offsets=off2, src=src[:m], count=int(head[0]), status=int(head[1]))


def smooth(runs, offsets, len_scale, reg=1e-10, longest=None):
    """-> (smoothed columns (R, 4), status word per track)"""
    runs = np.ascontiguousarray(runs, np.float64).reshape(-1, 5)
    offsets = np.ascontiguousarray(offsets, np.int32)
    ls = np.ascontiguousarray(len_scale, np.float64)
    n = len(offsets) - 1
    longest = int(np.diff(offsets).max()) if longest is None and n else int(longest or 0)
    out, status = np.zeros((len(runs), 4), np.float64), np.zeros(max(n, 1), np.int32)
    lib().hs_gsi_smooth(runs.ctypes.data, offsets.ctypes.data, ls.ctypes.data, n, longest, float(reg), out.ctypes.data, status.ctypes.data)
    return out, status[:n]


class HostGSI:
    """the interface of tracker.gsi.DeviceGSI on the host build"""

    def __init__(self, max_tracks=4096, max_rows=1 << 16, max_len=4096):
        self.max_tracks, self.max_rows, self.max_len = int(max_tracks), int(max_rows), int(max_len)

    def run(self, runs, offsets, len_scale, interval=20, reg=1e-10, longest=0):
        got = interpolate(runs, offsets, interval, self.max_rows, self.max_len)
        cols, status = smooth(got["runs"], got["offsets"], len_scale, reg, longest)
        got.update(cols=cols, track_status=status)
        return got
