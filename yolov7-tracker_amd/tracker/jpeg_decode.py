"""JPEG frames decoded on the device: the file's bytes go to the GPU (about a ninth of the raw frame's) and come out as the (H, W, 3) uint8 BGR frame that
`PIL.Image.open(p).convert("RGB")[..., ::-1]` returns on the host, byte for byte -- libjpeg-turbo's defaults: the accurate integer inverse DCT, "fancy" chroma
upsampling, YCbCr -> RGB (include/y7t.h: y7t_jpegdec_decode; csrc/y7t_jpegdec.hip; DESIGN.md section 4 "JPEG decoding" is the specification).

The host reads markers and lengths only (`parse`: a few hundred bytes a file); entropy decoding, the inverse DCT, upsampling and colour conversion run on the
device.  Baseline sequential files with 8-bit samples, one scan, one or three components and 4:4:4 / 4:2:2 / 4:2:0 sampling are in scope; for everything else
`parse` returns None and the caller decodes on the host, as before.  EXIF orientation is ignored, as tracker_dataloader.TrackerLoader ignores it.
"""
import ctypes
import re
import weakref
from collections import namedtuple

import numpy as np

from .. import _lib

SAMPLING = {"444": 0, "422": 1, "420": 2, "gray": 3}      # Y7T_JPEGDEC_444, _422, _420, _GRAY
MAX_SIDE = 16384                                          # Y7T_JPEGDEC_MAX_SIDE
MAX_FILE_BYTES = 1 << 28
SUBSEQ_MIN, SUBSEQ_DEFAULT = 16, 64                       # Y7T_JPEGDEC_SUBSEQ_MIN, Y7T_JPEGDEC_SUBSEQ_DEFAULT
# y7t_jpegdec_desc (include/y7t.h), 80 bytes
DESC_DTYPE = np.dtype([("file_off", np.uint32), ("file_len", np.uint32), ("scan_off", np.uint32), ("scan_len", np.uint32), ("restart_interval", np.uint32),
                       ("dqt_off", np.uint32, (4,)), ("dc_off", np.uint32, (4,)), ("ac_off", np.uint32, (4,)),
                       ("tq", np.uint8, (4,)), ("td", np.uint8, (4,)), ("ta", np.uint8, (4,))])
assert DESC_DTYPE.itemsize == 80

JpegInfo = namedtuple("JpegInfo", "H W components sampling desc")      # desc: one row of DESC_DTYPE with file_off = 0
_SCAN_END = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")      # the first marker in entropy-coded data that is neither a stuffed zero, RSTm nor a fill byte


def parse(data):
    """the markers of a JPEG file -> JpegInfo, or None for what the device decoder does not take: any SOF other than SOF0 (progressive, extended, lossless,
    arithmetic), 12-bit samples, 16-bit quantisation tables, four components or an Adobe colour transform other than YCbCr, more than one scan, sampling other than
    4:4:4 / 4:2:2 / 4:2:0 / one component, DNL, a side above MAX_SIDE, or a file that is no JPEG at all"""
    data = bytes(data)
    n = len(data)
    if n < 4 or n > MAX_FILE_BYTES or data[:2] != b"\xff\xd8":
        return None
    desc = np.zeros((), DESC_DTYPE)
    sof, dri, adobe, pos = None, 0, None, 2
    while True:
        while pos < n and data[pos] != 0xFF:      # (garbage between segments: libjpeg skips it too)
            pos += 1
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return None
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or pos + 2 > n:
            return None
        ln = data[pos] << 8 | data[pos + 1]
        if ln < 2 or pos + ln > n:
            return None
        seg = data[pos + 2:pos + ln]
        if m == 0xDB:
            k = 0
            while k < len(seg):
                pq, tq = seg[k] >> 4, seg[k] & 15
                if pq != 0 or tq > 3 or k + 65 > len(seg):      # 16-bit tables: out of scope
                    return None
                desc["dqt_off"][tq] = pos + 2 + k + 1
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                tc, th = seg[k] >> 4, seg[k] & 15
                if tc > 1 or th > 3 or k + 17 > len(seg):
                    return None
                nv = sum(seg[k + 1:k + 17])
                if nv > 256 or k + 17 + nv > len(seg):
                    return None
                desc["ac_off" if tc else "dc_off"][th] = pos + 2 + k + 1
                k += 17 + nv
        elif m == 0xC0:
            if sof is not None or len(seg) < 6:
                return None
            prec, H, W, nf = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if prec != 8 or nf not in (1, 3) or len(seg) != 6 + 3 * nf or not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):      # H == 0: DNL
                return None
            sof = (H, W, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif 0xC1 <= m <= 0xCF:      # SOF1 .. SOF15, JPG, DAC (DHT is handled above)
            return None
        elif m == 0xDC:      # DNL
            return None
        elif m == 0xDD:
            if len(seg) != 2:
                return None
            dri = seg[0] << 8 | seg[1]
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]      # the colour transform: 1 is YCbCr; 0 with three components is RGB, 2 is YCCK
        elif m == 0xDA:
            break
        pos += ln
    if sof is None:
        return None
    H, W, comps = sof
    if adobe is not None and len(comps) == 3 and adobe != 1:
        return None
    ns = seg[0] if seg else 0
    if ns != len(comps) or len(seg) != 4 + 2 * ns or seg[1 + 2 * ns] != 0 or seg[2 + 2 * ns] != 63 or seg[3 + 2 * ns] != 0:
        return None
    for i, (cid, h, v, tq) in enumerate(comps):
        if seg[1 + 2 * i] != cid or tq > 3:      # the scan's components in the frame's order
            return None
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if td > 3 or ta > 3 or not desc["dqt_off"][tq] or not desc["dc_off"][td] or not desc["ac_off"][ta]:
            return None
        desc["tq"][i], desc["td"][i], desc["ta"][i] = tq, td, ta
    if len(comps) == 1:
        if comps[0][1:3] != (1, 1):
            return None
        sampling = SAMPLING["gray"]
    else:
        if [c[0] for c in comps] == [82, 71, 66]:      # components named R, G, B: libjpeg takes them as RGB
            return None
        if comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1) or comps[0][1:3] not in ((1, 1), (2, 1), (2, 2)):
            return None
        sampling = {(1, 1): SAMPLING["444"], (2, 1): SAMPLING["422"], (2, 2): SAMPLING["420"]}[comps[0][1:3]]
    scan_off = pos + ln
    end = _SCAN_END.search(data, scan_off)
    if end is not None and data[end.start() + 1] != 0xD9:      # another scan, DNL, tables between scans: not a one-scan file
        return None
    scan_end = end.start() if end is not None else n      # (no EOI: the file is cut short; the device reports it)
    desc["file_len"], desc["scan_off"], desc["scan_len"], desc["restart_interval"] = n, scan_off, scan_end - scan_off, dri
    return JpegInfo(H, W, len(comps), sampling, desc)


def decode_host(data):
    """the host path this module replaces, and the fallback for what `parse` rejects: (H, W, 3) uint8 BGR like cv2.imread"""
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))[:, :, ::-1].copy()


class DeviceJpegDecoder:
    """DeviceJpegDecoder(H, W, components, sampling, max_batch).decode(list of file bytes) -> ((B, H, W, 3) uint8 BGR device tensor, (B,) int32 device status);
    any B (longer lists go in parts).  sampling: a value or a key of SAMPLING.  max_file_bytes: the longest file a call may hold (default: three quarters of the raw
    frame plus 64 KiB); subseq_bytes: 0 = the library's default."""

    def __init__(self, H, W, components=3, sampling="420", max_batch=8, max_file_bytes=None, subseq_bytes=0):
        import torch
        _lib.require_gpu()
        self._L = _lib.load()
        self.H, self.W, self.components, self.max_batch = int(H), int(W), int(components), int(max_batch)
        self.sampling = SAMPLING[sampling] if isinstance(sampling, str) else int(sampling)
        self.max_file_bytes = int(max_file_bytes) if max_file_bytes else self.H * self.W * 3 // 4 + 65536
        self.subseq_bytes = int(subseq_bytes)
        nbytes = int(self._L.y7t_jpegdec_bytes(self.H, self.W, self.components, self.sampling, self.max_batch, self.max_file_bytes, self.subseq_bytes))
        if nbytes == 0:
            raise ValueError("a decoder for %d x %d, %d components, sampling %r, batches of %d, files of %d bytes, subsequences of %d is out of range"
                             % (self.H, self.W, self.components, sampling, self.max_batch, self.max_file_bytes, self.subseq_bytes))
        self._obj = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        weakref.finalize(self._obj, DeviceJpegDecoder._release, self._L, int(self._obj.data_ptr()))
        _lib.check(self._L.y7t_jpegdec_init(_lib.ptr(self._obj), nbytes, self.H, self.W, self.components, self.sampling, self.max_batch, self.max_file_bytes,
                                            self.subseq_bytes, _lib.stream_ptr()))
        self._host, self._copied, self._turn = [None, None], [None, None], 0      # two pinned buffers in turn, each with the event of its last copy

    @staticmethod
    def _release(L, address):
        try:
            L.y7t_jpegdec_release(address)
        except Exception:
            pass

    def matches(self, info):
        return (info.H, info.W, info.components, info.sampling) == (self.H, self.W, self.components, self.sampling) and int(info.desc["file_len"]) <= self.max_file_bytes

    def upload(self, files, infos=None):
        """the files back to back (each from a 4-byte boundary) through one pinned buffer -> (device bytes, the records with their file_off)"""
        import torch
        infos = [parse(f) for f in files] if infos is None else list(infos)
        descs = np.zeros(len(files), DESC_DTYPE)
        at = 0
        for b, (f, info) in enumerate(zip(files, infos)):
            if info is None or not self.matches(info):
                raise ValueError("file %d is not a baseline JPEG of this decoder's geometry (%d x %d, %d components, sampling %d, <= %d bytes)"
                                 % (b, self.H, self.W, self.components, self.sampling, self.max_file_bytes))
            descs[b] = info.desc
            descs[b]["file_off"] = at
            at += (len(f) + 3) & ~3
        k = self._turn = self._turn ^ 1
        if self._copied[k] is not None:      # the copy that last read this buffer has finished before it is written again
            self._copied[k].synchronize()
        if self._host[k] is None or self._host[k].numel() < at:
            self._host[k] = torch.empty(max(at, 1), dtype=torch.uint8).pin_memory()
        view = self._host[k].numpy()
        for f, d in zip(files, descs):
            view[int(d["file_off"]):int(d["file_off"]) + len(f)] = np.frombuffer(f, np.uint8)
        dev = self._host[k][:max(at, 1)].cuda(non_blocking=True)
        self._copied[k] = torch.cuda.Event()
        self._copied[k].record()
        return dev, descs

    def decode_uploaded(self, dev, descs, out=None):
        """one call of y7t_jpegdec_decode: len(descs) <= max_batch files that lie in `dev`"""
        import torch
        B = len(descs)
        frames = out if out is not None else torch.empty((B, self.H, self.W, 3), dtype=torch.uint8, device="cuda")
        status = torch.zeros(max(B, 1), dtype=torch.int32, device="cuda")
        descs = np.ascontiguousarray(descs)
        _lib.check(self._L.y7t_jpegdec_decode(_lib.ptr(self._obj), _lib.ptr(dev), ctypes.c_void_p(descs.ctypes.data), B, _lib.ptr(frames), _lib.ptr(status),
                                              _lib.stream_ptr()))
        return frames, status[:B]

    def decode(self, files, infos=None):
        import torch
        files = [bytes(f) for f in files]
        frames = torch.empty((len(files), self.H, self.W, 3), dtype=torch.uint8, device="cuda")
        status = torch.zeros(len(files), dtype=torch.int32, device="cuda")
        for b0 in range(0, len(files), self.max_batch):
            part = files[b0:b0 + self.max_batch]
            dev, descs = self.upload(part, None if infos is None else infos[b0:b0 + self.max_batch])
            out = frames[b0:b0 + len(part)]
            if out.data_ptr() & 3:      # (the kernels store dwords: a part that starts at an odd frame of an odd size is decoded into a buffer of its own)
                got, st = self.decode_uploaded(dev, descs)
                out.copy_(got)
            else:
                _, st = self.decode_uploaded(dev, descs, out=out)
            status[b0:b0 + len(part)] = st
        return frames, status

    def rounds(self, B):
        """after a call: per file, the last launch of the synchronisation that found work, plus one (a read-back: for measurements)"""
        return self._obj[256:256 + 4 * B].cpu().numpy().view(np.int32).copy()


_decoders = {}


def decode_batch(files, max_batch=8, counts=None):
    """a batch of a sequence's files -> (B, H, W, 3) uint8 BGR on the device (ValueError when the frames differ in size, which a batch of raw frames cannot either).
    Files of one geometry are decoded in one call; a file `parse` rejects, or whose status is not zero, is decoded on the host and uploaded, as before.
    counts (a dict) receives how many frames went each way: counts['device'], counts['host']."""
    import torch
    files = [bytes(f) for f in files]
    infos = [parse(f) for f in files]
    host = {b: decode_host(files[b]) for b, info in enumerate(infos) if info is None}
    shapes = {(i.H, i.W) for i in infos if i is not None} | {h.shape[:2] for h in host.values()}
    if len(shapes) != 1:
        raise ValueError("the frames of a batch differ in size: %s" % sorted(shapes))
    H, W = shapes.pop()
    out = torch.empty((len(files), H, W, 3), dtype=torch.uint8, device="cuda")
    groups = {}
    for b, info in enumerate(infos):
        if info is not None:
            groups.setdefault((info.components, info.sampling), []).append(b)
    for (components, sampling), idx in groups.items():
        key = (H, W, components, sampling, int(max_batch))
        need = max(int(infos[b].desc["file_len"]) for b in idx)
        dec = _decoders.get(key)
        if dec is None or dec.max_file_bytes < need:
            _decoders.clear()      # (a sequence's frames share one geometry: keep one decoder alive)
            dec = _decoders[key] = DeviceJpegDecoder(H, W, components, sampling, max_batch=int(max_batch), max_file_bytes=max(need * 2, H * W * 3 // 4 + 65536))
        frames, status = dec.decode([files[b] for b in idx], [infos[b] for b in idx])
        out[torch.as_tensor(idx, device="cuda")] = frames
        for b, st in zip(idx, status.cpu().tolist()):      # the one read-back of the path: four bytes a file
            if st:
                host[b] = decode_host(files[b])
    for b, frame in host.items():
        out[b] = torch.from_numpy(frame).cuda()
    if counts is not None:
        counts["host"] = counts.get("host", 0) + len(host)
        counts["device"] = counts.get("device", 0) + len(files) - len(host)
    return out
