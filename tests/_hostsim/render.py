"""tests/_hostsim/render.py -- TEST INFRASTRUCTURE ONLY: the host build of csrc/y7t_render.h (y7t_hostsim_render.cpp): the overlay and the baseline JPEG encoder
with the functions the device kernels call, so that their arithmetic can be tested without a GPU and the kernels compared with it byte for byte."""
import ctypes
import os

import numpy as np

from tests._hostsim import _HERE, _build

_SO = os.path.join(_HERE, "liby7t_hostsim_render.so")
_lib = None
# a row of the packed track table (include/y7t.h: y7t_render_track)
TRACK_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("w", np.float32), ("h", np.float32), ("id", np.int32), ("len", np.int32), ("label", np.uint8, (24,))])


def build_render(force=False):
    return _build(_SO, "y7t_hostsim_render.cpp", force=force)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_render())
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        L.hs_render_draw.argtypes = [vp, ci, ci, ci, vp, vp, vp]
        L.hs_render_draw.restype = None
        L.hs_jpeg_file_max.argtypes = [ci, ci, ci]
        L.hs_jpeg_file_max.restype = sz
        L.hs_jpeg_encode.argtypes = [vp, ci, ci, ci, ci, vp]
        L.hs_jpeg_encode.restype = sz
        _lib = L
    return _lib


def pack_tracks(tracks_per_frame):
    """[[(x, y, w, h, id, label bytes), ...] per frame] -> (rows of TRACK_DTYPE, offsets int32)"""
    n = sum(len(t) for t in tracks_per_frame)
    rows = np.zeros(n, TRACK_DTYPE)
    offsets = np.zeros(len(tracks_per_frame) + 1, np.int32)
    i = 0
    for b, tracks in enumerate(tracks_per_frame):
        for x, y, w, h, tid, label in tracks:
            label = bytes(label)[:24]
            rows[i] = (x, y, w, h, tid, len(label), np.frombuffer(label.ljust(24, b"\0"), np.uint8))
            i += 1
        offsets[b + 1] = i
    return rows, offsets


def draw(frames, tracks_per_frame):
    """frames (B, H, W, 3) uint8 -> the annotated frames"""
    frames = np.ascontiguousarray(frames, np.uint8)
    B, H, W, _ = frames.shape
    rows, offsets = pack_tracks(tracks_per_frame)
    assert len(offsets) == B + 1 and TRACK_DTYPE.itemsize == 48
    out = np.zeros_like(frames)
    lib().hs_render_draw(frames.ctypes.data, B, H, W, rows.ctypes.data if len(rows) else None, offsets.ctypes.data, out.ctypes.data)
    return out


def encode(frame, quality=95, subsampling="420"):
    """(H, W, 3) uint8 BGR -> the JPEG file's bytes"""
    frame = np.ascontiguousarray(frame, np.uint8)
    H, W, _ = frame.shape
    sub = {"420": 0, "444": 1}[subsampling]
    out = np.zeros(lib().hs_jpeg_file_max(H, W, sub), np.uint8)
    n = lib().hs_jpeg_encode(frame.ctypes.data, H, W, int(quality), sub, out.ctypes.data)
    assert n > 0, "the host build's code length and its code disagree"
    return out[:n].tobytes()
