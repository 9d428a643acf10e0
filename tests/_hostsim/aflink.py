"""tests/_hostsim/aflink.py -- TEST INFRASTRUCTURE ONLY: the candidate stage of csrc/y7t_aflink.h (gate, row-major compaction, pair transform) of the host build
(y7t_hostsim_aflink.cpp), so that the pair list and the transformed blocks can be tested without a GPU."""
import ctypes
import os

import numpy as np

from tests._hostsim import _HERE, _build

_SO = os.path.join(_HERE, "liby7t_hostsim_aflink.so")
_lib = None


def build_aflink(force=False):
    return _build(_SO, "y7t_hostsim_aflink.cpp", force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_aflink())
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.hs_afl_candidates.argtypes = [vp, vp, ci, cd, cd, cd, ci, vp, vp, vp, vp, vp]
        L.hs_afl_candidates.restype = None
        _lib = L
    return _lib


def constants():
    """the kernels' pairs per chunk and pairs per workgroup of the head (csrc/y7t_aflink.h)"""
    return dict(chunk=int(lib().hs_afl_chunk()), head_pairs=int(lib().hs_afl_head_pairs()))


def candidates(table, offsets, thrT=(0, 30), thrS=75, max_pairs=1 << 16):
    """-> dict(count, status, pairs (n, 2), x1, x2 (n, 30, 3)), n = min(count, max_pairs)"""
    table = np.ascontiguousarray(table, np.float64).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, np.int32)
    pairs = np.zeros((max_pairs, 2), np.int32)
    x1, x2 = np.zeros((max_pairs, 30, 3), np.float32), np.zeros((max_pairs, 30, 3), np.float32)
    head = np.zeros(2, np.int32)
    lib().hs_afl_candidates(table.ctypes.data, offsets.ctypes.data, len(offsets) - 1, float(thrT[0]), float(thrT[1]), float(thrS), max_pairs, pairs.ctypes.data,
                            x1.ctypes.data, x2.ctypes.data, head.ctypes.data, head.ctypes.data + 4)
    n = min(int(head[0]), max_pairs)
    return dict(count=int(head[0]), status=int(head[1]), pairs=pairs[:n], x1=x1[:n], x2=x2[:n])
