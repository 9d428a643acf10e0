"""tests/_hostsim/tta.py -- TEST INFRASTRUCTURE ONLY: the host build of csrc/y7t_tta.h (y7t_hostsim_tta.cpp): the scale + layout body of k_tta_scale_layout and the
de-scale / de-flip of k_decode_append, so that their arithmetic can be tested without a GPU and the device kernels compared with it bit for bit."""
import ctypes
import os

import numpy as np

from tests._hostsim import _HERE, _build

_SO = os.path.join(_HERE, "liby7t_hostsim_tta.so")
_lib = None


def build_tta(force=False):
    return _build(_SO, "y7t_hostsim_tta.cpp", force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_tta())
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.hs_tta_scale_layout.argtypes = [vp] + [ci] * 10 + [vp, ci]
        L.hs_tta_scale_layout.restype = None
        L.hs_tta_descale_deflip.argtypes = [vp, ci, cf, ci, cf]
        L.hs_tta_descale_deflip.restype = None
        L.hs_tta_taps.argtypes = [ci, ci, vp, vp, vp, vp]
        L.hs_tta_taps.restype = None
        L.hs_tta_rows.argtypes = [ci, ci, vp]
        L.hs_tta_rows.restype = None
        L.hs_tta_pad.restype = cf
        _lib = L
    return _lib


def scale_layout(img, flip, hs, ws, Hp, Wp, reorg):
    """img: (B, 3, H, W) float32 RGB or (B, H, W, 3) uint8 BGR -> (B, Ho, Wo, ldout) float16, what k_tta_scale_layout writes (ldout 16 with reorg, 8 without)"""
    img = np.ascontiguousarray(img)
    is_u8 = img.dtype == np.uint8
    if not is_u8:
        img = np.ascontiguousarray(img, np.float32)
    B = img.shape[0]
    H, W = (img.shape[1], img.shape[2]) if is_u8 else (img.shape[2], img.shape[3])
    ld = 16 if reorg else 8
    out = np.zeros((B, Hp // 2 if reorg else Hp, Wp // 2 if reorg else Wp, ld), np.float32)
    lib().hs_tta_scale_layout(img.ctypes.data, int(is_u8), B, H, W, int(flip or 0), hs, ws, Hp, Wp, int(bool(reorg)), out.ctypes.data, ld)
    return out.astype(np.float16)      # the kernel's one rounding per element (float32 -> fp16, nearest even, on both sides)


def descale_deflip(xywh, scale, flip, flip_extent):
    """(n, 4) float32 rows of {x, y, w, h} -> the rows after `/= scale` and the de-flip"""
    a = np.array(xywh, np.float32, order="C", copy=True).reshape(-1, 4)
    lib().hs_tta_descale_deflip(a.ctypes.data, len(a), float(scale), int(flip or 0), float(flip_extent))
    return a


def taps(n_in, n_out):
    i0, i1 = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    l0, l1 = np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    lib().hs_tta_taps(n_in, n_out, i0.ctypes.data, i1.ctypes.data, l0.ctypes.data, l1.ctypes.data)
    return i0, i1, l0, l1


def rows(n, row_base):
    """the rows of a pass of n anchors in the concatenation"""
    out = np.zeros(n, np.int32)
    lib().hs_tta_rows(n, int(row_base), out.ctypes.data)
    return out


def pad_value():
    return np.float32(lib().hs_tta_pad())
