"""tests/_hostsim/jpegdec.py -- TEST INFRASTRUCTURE ONLY: the host build of csrc/y7t_jpegdec.h (y7t_hostsim_jpegdec.cpp): the baseline JPEG decoder with the
functions the device kernels call and the launches of y7t_jpegdec_decode as loops, so that its arithmetic, its synchronisation rounds and its behaviour on
corrupt streams can be tested without a GPU and the kernels compared with it byte for byte."""
import ctypes
import os

import numpy as np

from tests._hostsim import _HERE, _build

_SO = os.path.join(_HERE, "liby7t_hostsim_jpegdec.so")
_lib = None
CANARY = 0xA5
GUARD = 4096
LANES = 256      # Y7T_JD_LANES


def build_jpegdec(force=False):
    return _build(_SO, "y7t_hostsim_jpegdec.cpp", force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_jpegdec())
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        L.hs_jpegdec_bytes.argtypes = [ci, ci, ci, sz, ci, ci]
        L.hs_jpegdec_bytes.restype = sz
        L.hs_jpegdec_nblocks.argtypes = [ci, ci, ci]
        L.hs_jpegdec_layout.argtypes = [ci, ci, ci, sz, ci, ci, vp]
        L.hs_jpegdec_decode.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def subseq_min():
    return int(lib().hs_jpegdec_subseq_min())


class Result:
    """status, rounds (launches that found work), iters (most rounds inside a run), launches, nsub; diffs / coefs (nblocks, 64) int16; frame; rc; clean: the guard
    bytes around the frame and the workspace were found as they were left"""


def decode(data, info, subseq_bytes=128, lanes=LANES):
    """data: the file's bytes (or any corruption of them); info: tracker.jpeg_decode.parse of a file of this geometry -> Result"""
    L = lib()
    data = bytes(data)
    desc = np.array(info.desc).copy()
    assert desc.dtype.itemsize == L.hs_jpegdec_desc_bytes()
    nblocks = L.hs_jpegdec_nblocks(info.H, info.W, info.sampling)
    ws_bytes = L.hs_jpegdec_bytes(info.H, info.W, info.sampling, max(int(desc["file_len"]), 1), subseq_bytes, lanes)
    assert ws_bytes
    src = np.frombuffer(data, np.uint8).copy() if data else np.zeros(1, np.uint8)
    ws = np.full(ws_bytes + 2 * GUARD, CANARY, np.uint8)
    ws[GUARD:-GUARD] = 0
    fr = np.full(info.H * info.W * 3 + 2 * GUARD, CANARY, np.uint8)
    diffs, coefs = np.zeros((nblocks, 64), np.int16), np.zeros((nblocks, 64), np.int16)
    out = np.zeros(5, np.int32)
    r = Result()
    r.rc = L.hs_jpegdec_decode(src.ctypes.data, desc.ctypes.data, info.H, info.W, info.sampling, subseq_bytes, lanes, ws[GUARD:].ctypes.data,
                               diffs.ctypes.data, coefs.ctypes.data, fr[GUARD:].ctypes.data, out.ctypes.data)
    r.status, r.rounds, r.iters, r.launches, r.nsub = [int(v) for v in out]
    r.diffs, r.coefs, r.frame = diffs, coefs, fr[GUARD:-GUARD].reshape(info.H, info.W, 3).copy()
    r.ws = ws[GUARD:-GUARD]
    r.clean = bool((ws[:GUARD] == CANARY).all() and (ws[-GUARD:] == CANARY).all() and (fr[:GUARD] == CANARY).all() and (fr[-GUARD:] == CANARY).all())
    return r


LAYOUT = ["rounds", "iters", "descs", "entry", "exit", "count", "first", "run_exit", "run_entry", "run_round", "run_iters", "coef", "total"]


def layout(info, max_file_bytes, subseq_bytes=128, lanes=LANES):
    """{array: its offset in a decoder object for ONE file of this geometry}"""
    out = np.zeros(13, np.uint64)
    assert lib().hs_jpegdec_layout(info.H, info.W, info.sampling, max_file_bytes, subseq_bytes, lanes, out.ctypes.data) == 0
    return dict(zip(LAYOUT, (int(v) for v in out)))
