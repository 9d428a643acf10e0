"""tests/render_scenes.py -- TEST INFRASTRUCTURE ONLY: the frames, shapes and overlay cases the rendering tests share (CPU: host build against the NumPy
restatement and Pillow; GPU: the kernels against the host build).  Every shape is the smallest at which one mechanism can go wrong; every scene drives one path
of the entropy coder."""
import numpy as np

QUALITIES = (50, 95, 100)
SUBSAMPLINGS = ("420", "444")
SCENES = ("ramps", "flat", "random", "basis77", "alternate")


def shapes(subsampling):
    """(W, H): one block (the 4:2:0 MCU padded from 8 to 16); one 4:2:0 MCU; odd sides, replication on both axes; several MCUs; more than 8 MCU rows (the RST index
    wraps); sides that are multiples of 8 but not of 16; a 1920-wide strip of one MCU row: more than 256 blocks, the entropy kernel's chunks with a carried bit offset"""
    return [(8, 8), (16, 16), (17, 33), (48, 64), (24, 152) if subsampling == "420" else (24, 88), (200, 120), (1920, 16)]


def scene(name, W, H, seed=0):
    """-> (H, W, 3) uint8 BGR"""
    rng = np.random.default_rng([seed, W, H, SCENES.index(name)])
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "ramps":      # smooth ramps plus noise
        f = np.stack([40 + xx * 150 // max(W - 1, 1), 30 + yy * 180 // max(H - 1, 1), 220 - (xx + yy) * 160 // max(W + H - 2, 1)], -1) + rng.integers(-6, 7, (H, W, 3))
    elif name == "flat":      # EOB only, DC difference 0 after the first block
        f = np.broadcast_to(np.array([90, 140, 200]), (H, W, 3))
    elif name == "random":      # 0 / 255 at random, per pixel (the longest codes, the worst case for the segment slot, 0xFF bytes in the stream) and, in a third of
        f = rng.integers(0, 2, (H, W, 3)) * 255      # the blocks, per block (black next to white: DC category 11)
        solid = rng.integers(0, 6, (H // 8 + 1, W // 8 + 1))
        solid = np.repeat(np.repeat(solid, 8, 0), 8, 1)[:H, :W, None]
        f = np.where(solid == 0, 0, np.where(solid == 1, 255, f))
    elif name == "basis77":      # every block only the (7, 7) basis pattern: 62 zeros before the one coefficient, ZRL three times
        c = np.cos((2 * (np.arange(8)) + 1) * 7 * np.pi / 16)
        tile = np.rint(128 + 100 * np.outer(c, c))
        f = np.repeat(np.tile(tile, (H // 8 + 1, W // 8 + 1))[:H, :W, None], 3, -1)
    elif name == "alternate":      # black and white blocks in turn: the extreme DC differences in both signs
        f = np.repeat(((xx // 8 + yy // 8) % 2 * 255)[..., None], 3, -1)
    else:
        raise KeyError(name)
    return np.clip(f, 0, 255).astype(np.uint8)


def overlay_frame(W, H, seed=0):
    return np.random.default_rng([seed, W, H]).integers(0, 256, (H, W, 3)).astype(np.uint8)


# name -> (W, H, [(x, y, w, h, id, label)]): the cases of the issue, one mechanism each
OVERLAY_CASES = {
    "none": (40, 30, []),
    "inside": (64, 48, [(10.0, 20.0, 30.0, 15.0, 1, b"3-1")]),
    "partly_left_top": (64, 48, [(-12.5, -7.25, 30.0, 25.0, 2, b"0-2")]),
    "partly_right_bottom": (64, 48, [(50.0, 35.0, 40.0, 40.0, 3, b"0-3")]),
    "outside_left": (64, 48, [(-60.0, 10.0, 20.0, 20.0, 4, b"0-4")]),
    "outside_right": (64, 48, [(90.0, 10.0, 20.0, 20.0, 5, b"0-5")]),
    "outside_top": (64, 48, [(10.0, -80.0, 20.0, 20.0, 6, b"0-6")]),
    "outside_bottom": (64, 48, [(10.0, 90.0, 20.0, 20.0, 7, b"0-7")]),
    "trunc_toward_zero": (64, 48, [(-0.5, -0.99, 20.9, 12.5, 8, b"")]),
    "zero_area": (64, 48, [(30.0, 30.0, 0.0, 0.0, 9, b"")]),
    "label_clipped_top": (64, 48, [(5.0, 4.0, 20.0, 20.0, 10, b"car-10")]),
    "label_clipped_right": (64, 48, [(40.0, 20.0, 20.0, 20.0, 11, b"pedestrian-11")]),
    "overlap_later_wins": (64, 48, [(10.0, 20.0, 30.0, 20.0, 12, b"van-12"), (8.0, 8.0, 30.0, 20.0, 13, b"bus-13")]),
    "ids": (96, 64, [(4.0, 14.0, 16.0, 10.0, 0, b"0-0"), (28.0, 14.0, 16.0, 10.0, 1, b"0-1"), (52.0, 14.0, 16.0, 10.0, 85, b"0-85"),
                     (4.0, 44.0, 60.0, 10.0, 2 ** 31 - 1, b"0-2147483647")]),
    "label_24_and_empty": (220, 40, [(4.0, 14.0, 30.0, 10.0, 14, b"ABCDEFGHIJKLMNOPQRSTUVWX"), (4.0, 30.0, 30.0, 6.0, 15, b"")]),
    "all_glyphs": (220, 80, [(2.0, 12.0 + 13 * i, 3.0, 1.0, 16 + i, bytes(range(0x20 + 24 * i, min(0x20 + 24 * i + 24, 0x7F)))) for i in range(4)]),
    "odd_sides": (45, 37, [(3.0, 12.0, 30.0, 20.0, 21, b"7-21"), (20.5, 5.5, 40.0, 10.0, 22, b"8-22")]),      # a width that is no multiple of 4: the kernel's byte path
    "300_boxes_one_tile":(64, 64, [(float(i % 7), float(i % 5), 50.0 + i % 11, 50.0 + i % 13, i, b"%d-%d" % (i % 10, i)) for i in range(300)]),
}


def overlay_case(name):
    W, H, tracks = OVERLAY_CASES[name]
    return overlay_frame(W, H), tracks
