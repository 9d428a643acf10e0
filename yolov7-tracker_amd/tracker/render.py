"""Annotated frames on the device: what the reference's `plot_img` and `save_videos` do per frame (tracker/track.py:275-340 there) -- a rectangle and a label per
track, a JPEG per frame, a video per sequence -- without the frame ever leaving the device as pixels.

The device does the overlay and the encoding (include/y7t.h: y7t_render_draw, y7t_jpeg_encode; csrc/y7t_render.hip); the host assembles the labels, writes the
files and, for --save_videos, joins the very same JPEG byte strings into a Motion-JPEG AVI.  DESIGN.md section 4 "Rendering" is the specification: this project's
own outline rule and bitmap font (not cv2's rasteriser or its Hershey glyphs), sequential baseline JPEG with the Annex K tables and a restart interval of one MCU row.
"""
import ctypes
import os
import struct
import weakref

import numpy as np

from .. import _lib

SUBSAMPLING = {"420": 0, "444": 1}      # Y7T_JPEG_SUB_420, Y7T_JPEG_SUB_444
LABEL_BYTES = 24                        # Y7T_RENDER_LABEL_BYTES
# a row of the packed track table (include/y7t.h: y7t_render_track)
TRACK_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("w", np.float32), ("h", np.float32), ("id", np.int32), ("len", np.int32), ("label", np.uint8, (LABEL_BYTES,))])


def label_for(cls, track_id, category_dict=None):
    """plot_img's f'{CATEGORY_DICT[cls]}-{id}'; a class the dictionary does not name is written as its number"""
    name = (category_dict or {}).get(int(cls))
    text = "%s-%d" % (name if name is not None else int(cls), int(track_id))
    return text.encode("ascii", "replace")[:LABEL_BYTES]


def pack_tracks(tracks_per_frame):
    """[[(x, y, w, h, id, label bytes), ...] per frame] -> (rows of TRACK_DTYPE, offsets int32 of len(frames) + 1)"""
    rows = np.zeros(sum(len(t) for t in tracks_per_frame), TRACK_DTYPE)
    offsets = np.zeros(len(tracks_per_frame) + 1, np.int32)
    i = 0
    for b, tracks in enumerate(tracks_per_frame):
        for x, y, w, h, tid, label in tracks:
            label = bytes(label)[:LABEL_BYTES]
            rows[i] = (x, y, w, h, tid, len(label), np.frombuffer(label.ljust(LABEL_BYTES, b"\0"), np.uint8))
            i += 1
        offsets[b + 1] = i
    return rows, offsets


def tracks_from_results(ids, tlwhs, clses, category_dict=None):
    """a frame's entry of track.py's `results` -> the rows DeviceRenderer draws"""
    return [(t[0], t[1], t[2], t[3], int(i), label_for(c, i, category_dict)) for i, t, c in zip(ids, tlwhs, clses)]


class DeviceRenderer:
    """DeviceRenderer(H, W).save(frames, tracks_per_frame, paths): frames (B, H, W, 3) uint8 BGR, a device or a host tensor / array (uploaded once); any B (batches
    longer than max_batch are taken in parts, with the same bytes)."""

    def __init__(self, H, W, quality=95, subsampling="420", max_batch=8):
        import torch
        _lib.require_gpu()
        self._L = _lib.load()
        self.H, self.W, self.quality, self.subsampling, self.max_batch = int(H), int(W), int(quality), str(subsampling), int(max_batch)
        if self.subsampling not in SUBSAMPLING:
            raise ValueError("subsampling %r: '420' or '444'" % (subsampling,))
        if not 1 <= self.quality <= 100:
            raise ValueError("quality %r: 1 .. 100" % (quality,))
        sub, out_bytes = SUBSAMPLING[self.subsampling], ctypes.c_size_t()
        nbytes = int(self._L.y7t_jpeg_bytes(self.H, self.W, sub, self.max_batch, ctypes.byref(out_bytes)))
        if nbytes == 0:
            raise ValueError("frames of %d x %d in batches of %d are out of the encoder's range" % (self.H, self.W, self.max_batch))
        self._obj = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        weakref.finalize(self._obj, DeviceRenderer._release, self._L, int(self._obj.data_ptr()))
        _lib.check(self._L.y7t_jpeg_init(_lib.ptr(self._obj), nbytes, self.H, self.W, self.quality, sub, self.max_batch, _lib.stream_ptr()))
        self._out_bytes = int(out_bytes.value)
        self._out = torch.empty(self._out_bytes, dtype=torch.uint8, device="cuda")
        self._lens = torch.zeros(self.max_batch + 1, dtype=torch.int32, device="cuda")
        self._guess = max(4096, self.H * self.W // 2)      # bytes of a file the first read-back brings along with the lengths; grows with what is seen
        self._host = None

    @staticmethod
    def _release(L, address):
        try:
            L.y7t_jpeg_release(address)
        except Exception:
            pass

    def _frames(self, frames):
        import torch
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        if t.dim() == 3:
            t = t[None]
        if t.dtype != torch.uint8 or t.dim() != 4 or tuple(t.shape[1:]) != (self.H, self.W, 3):
            raise ValueError("frames must be (B, %d, %d, 3) uint8, got %s %s" % (self.H, self.W, tuple(t.shape), t.dtype))
        return t.cuda().contiguous()

    def draw(self, frames, tracks_per_frame):
        """-> the annotated frames, a new (B, H, W, 3) uint8 device tensor; `frames` is not modified"""
        import torch
        f = self._frames(frames)
        if len(tracks_per_frame) != f.shape[0]:
            raise ValueError("%d frames, %d track lists" % (f.shape[0], len(tracks_per_frame)))
        rows, offsets = pack_tracks(tracks_per_frame)
        d_rows = torch.from_numpy(rows.view(np.uint8).reshape(-1)).cuda() if len(rows) else None
        d_off = torch.from_numpy(offsets).cuda()
        out = torch.empty_like(f)
        _lib.check(self._L.y7t_render_draw(_lib.ptr(f), f.shape[0], self.H, self.W, _lib.ptr(d_rows) if d_rows is not None else None, _lib.ptr(d_off), _lib.ptr(out),
                                           _lib.stream_ptr()))
        return out

    def _pinned(self, n):
        import torch
        if self._host is None or self._host.numel() < n:
            self._host = torch.empty(n, dtype=torch.uint8).pin_memory()
        return self._host

    def encode(self, frames):
        """-> one `bytes` per frame: a complete JFIF file"""
        import torch
        f = self._frames(frames)
        files = []
        for b0 in range(0, f.shape[0], self.max_batch):
            part = f[b0:b0 + self.max_batch]
            if part.data_ptr() & 3:      # (the kernels read dwords: a part that starts at an odd frame of an odd size moves to an aligned address)
                part = part.clone()
            B = part.shape[0]
            _lib.check(self._L.y7t_jpeg_encode(_lib.ptr(self._obj), _lib.ptr(part), B, _lib.ptr(self._out), self._out_bytes, _lib.ptr(self._lens), _lib.stream_ptr()))
            # one copy brings the lengths and, unless the files are larger than any before, the bytes: lengths first, then the image, into one pinned buffer
            head = 4 * (self.max_batch + 1)
            want = min(self._out_bytes, B * self._guess)
            host = self._pinned(head + self._out_bytes)
            stage = torch.cat([self._lens.view(torch.uint8), self._out[:want]])
            host[:head + want].copy_(stage, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            lens = host[:head].numpy().view(np.int32)[:B + 1].copy()
            total = int(lens[B])
            if total > want:      # larger files than the guess: the rest comes in a second copy, and the guess grows
                host[head + want:head + total].copy_(self._out[want:total], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                self._guess = max(self._guess, (total + B - 1) // B * 5 // 4)
            data = host[head:head + total].numpy()
            files += [data[int(lens[b]):int(lens[b + 1])].tobytes() for b in range(B)]
        return files

    def save(self, frames, tracks_per_frame, paths):
        """draw, encode and write paths[b] for every frame -> the files' bytes"""
        if len(paths) != len(tracks_per_frame):
            raise ValueError("%d paths, %d track lists" % (len(paths), len(tracks_per_frame)))
        files = self.encode(self.draw(frames, tracks_per_frame))
        for path, data in zip(paths, files):
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "wb") as fh:
                fh.write(data)
        return files


def write_mjpeg_avi(path, jpeg_bytes_list, size, fps=15):
    """a Motion-JPEG AVI (RIFF: hdrl with avih and one strl of fourcc MJPG, movi with one 00dc chunk per frame, idx1) whose chunks are the given JPEG files, byte
    for byte; size = (width, height).  Chunks of odd length are padded to even with a zero byte, as RIFF asks."""
    W, H = int(size[0]), int(size[1])
    n = len(jpeg_bytes_list)
    biggest = max([len(j) for j in jpeg_bytes_list], default=0)

    def chunk(tag, payload):
        return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")

    def riff_list(kind, payload):
        return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload

    avih = struct.pack("<14I", 1000000 // int(fps), biggest * int(fps), 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)      # 0x10: AVIF_HASINDEX
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, 1, int(fps), 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = riff_list(b"hdrl", chunk(b"avih", avih) + riff_list(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    frames, index, at = b"", b"", 4      # idx1 offsets count from the 'movi' fourcc
    for j in jpeg_bytes_list:
        index += b"00dc" + struct.pack("<III", 0x10, at, len(j))      # 0x10: AVIIF_KEYFRAME
        c = chunk(b"00dc", bytes(j))
        frames += c
        at += len(c)
    body = b"AVI " + hdrl + riff_list(b"movi", frames) + chunk(b"idx1", index)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path
