"""tests/jpegdec_cases.py -- TEST INFRASTRUCTURE ONLY: the JPEG files the decoder tests share (Pillow writes them from seeded frames; nothing is read from disk)."""
import functools
import io

import numpy as np

SIZES = [(1, 1), (3, 5), (8, 8), (17, 33), (37, 53), (48, 70), (6, 31)]
SAMPLINGS = ["444", "422", "420", "gray"]
# the stream of tests/test_jpegdec_cpu.py::test_slow_to_synchronise_stream: a 24 x 40 noise frame of this seed, quality 100, 4:4:4, optimised tables.  Found by
# counting rounds in the restatement (jpegdec_np.sync_rounds at 16-byte subsequences) over seeds 0 .. 199: the one that needs the most rounds inside a run (178 for 177 lanes: no lane is right before its predecessor is)
SLOW_SEED = 83


def frame(h, w, kind, seed=0):
    if kind == "noise":
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], -1).astype(np.uint8)


def write(rgb, sampling="420", quality=75, optimize=False, restart=0, progressive=False, mode=None):
    """an (H, W, 3) RGB frame -> the bytes Pillow writes"""
    from PIL import Image
    im = Image.fromarray(rgb)
    kw = dict(quality=quality, optimize=optimize)
    if sampling == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[sampling]
    if mode:
        im = im.convert(mode)
    if restart:
        kw["restart_marker_blocks"] = restart
    if progressive:
        kw["progressive"] = True
    f = io.BytesIO()
    im.save(f, "JPEG", **kw)
    return f.getvalue()


def pillow_bgr(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


@functools.lru_cache(maxsize=None)
def matrix():
    """{(size, sampling): [(name, bytes), ...]}: every size x sampling, and per geometry smooth / noise x optimize x quality 30 / 100 x restart absent / 1 / 3"""
    out = {}
    for h, w in SIZES:
        for sampling in SAMPLINGS:
            files = []
            for kind in ("ramp", "noise"):
                rgb = frame(h, w, kind, seed=h * 131 + w)
                for optimize in (False, True):
                    for quality in (30, 100):
                        for restart in (0, 1, 3):
                            files.append(("%s-o%d-q%d-r%d" % (kind, optimize, quality, restart), write(rgb, sampling, quality, optimize, restart)))
            out[((h, w), sampling)] = files
    return out


@functools.lru_cache(maxsize=None)
def multi_run_stream():
    """160 x 160 noise, quality 100, 4:4:4, no restart markers: long enough that several workgroup runs must agree"""
    return write(frame(160, 160, "noise", seed=7), "444", 100)


@functools.lru_cache(maxsize=None)
def slow_stream(seed=SLOW_SEED):
    return write(frame(24, 40, "noise", seed=seed), "444", 100, optimize=True)


@functools.lru_cache(maxsize=None)
def reference(data):
    """the restatement's stages for a file, computed once: (DC differences, DC values, frame)"""
    from tests import jpegdec_np
    return jpegdec_np.decode(data, stages=True)
