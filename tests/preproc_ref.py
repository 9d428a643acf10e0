"""References and the geometry table of the uint8 frame samplers (tests/test_preprocess_cpu.py, tests/test_preprocess_gpu.py): plain numpy, no GPU.

Two references of the letterbox resize (cv2.INTER_LINEAR's geometry: half-pixel centres, edge-clamped taps, result rounded to uint8):
  letterbox_f32   oracle/letterbox_np.py, the float32 restatement.  csrc/y7t_post.hip and csrc/y7t_stem.hip are compiled without FMA contraction, so the device
                  samplers are the same sequence of IEEE float32 operations: the claim is bit equality.
  resize_f64      the same formula in float64 with the exact scale H0 / new_h, plus an a-priori bound `delta` on what the float32 pipeline can be off by.  Where the
                  float64 value is further than delta from a rounding tie the pixel is DECIDED: rint(v) is the only right answer, whatever the float32 code does."""
import numpy as np

from oracle import letterbox_np as lb

U = 2.0 ** -24      # unit roundoff of float32


def letterbox_f32(frame, img_size, stride):
    """(H0, W0, 3) uint8 BGR -> the letterboxed (H, W, 3) uint8 BGR image of the float32 restatement"""
    return lb.letterbox(frame, new_shape=(img_size, img_size), stride=stride)


def layout_tensor(img_bgr_u8, reorg):
    """letterboxed (H, W, 3) uint8 BGR -> what the layout kernels write, real channels only: (H, W, 3) RGB, or ReOrg'd (H/2, W/2, 12) with channel g*3 + ch,
    g = row parity + 2 * column parity (the cat order of ReOrg.forward), as float16 (float32 division by 255, then one rounding to fp16)"""
    x = lb.to_model_input(img_bgr_u8)                                   # (3, H, W) RGB float32 / 255
    if reorg:
        x = np.concatenate([x[:, ::2, ::2], x[:, 1::2, ::2], x[:, ::2, 1::2], x[:, 1::2, 1::2]], 0)
    return np.ascontiguousarray(x.transpose(1, 2, 0)).astype(np.float16)


def u8_to_f16(v):
    """grey level -> the fp16 value of the layout tensor (float32 division as in k_input_layout; test_preprocess_cpu.py checks that the float64 route agrees)"""
    return (np.asarray(v, np.float32) / np.float32(255.0)).astype(np.float16)


def _axis(n_src, n_dst):
    """float64 source coordinate of every destination index, its two clamped taps, the weight of the second, and the taps one further out on each side"""
    f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
    i0 = np.floor(f).astype(np.int64)
    w = f - i0
    c = lambda i: np.clip(i, 0, n_src - 1)
    return f, c(i0), c(i0 + 1), w, c(i0 - 1), c(i0 + 2)


def resize_f64(frame, new_h, new_w):
    """-> (v, delta), both (new_h, new_w, 3) float64: the bilinear value before rounding and the bound on |float32 pipeline - v| (before ITS rounding).

    delta = 4u max(|fx|, 1) Dx + 4u max(|fy|, 1) Dy + 8u 255, u = 2^-24:
      * source coordinate fx = fl(fl((x + 0.5) fl(s)) - 0.5): x + 0.5 is exact; the scale, the product and the subtraction round once each:
        |error| <= 2u (|fx| + 0.5) + u |fx| <= 4u max(|fx|, 1).  The weight wx = fx - floor(fx) is then exact for fx >= 0 (for fx < 0 both taps clamp to
        pixel 0 and the weight does not matter).  A bilinear surface is continuous and piecewise linear in fx with slope (difference of the tap pair), so
        a coordinate error e moves the value by at most e Dx, Dx = the larger |difference| of the two horizontal tap pairs of this pixel.  If the float64
        coordinate is within e of an integer, the float32 one may fall into the neighbouring cell: Dx then also covers that cell's tap pairs.  Same along y.
      * the blend: 1 - wx rounds once (<= u, times a grey level <= 255), the two products round to <= u 255 together (their magnitudes sum to <= 255), the
        sum once: 3u 255 per horizontal blend; the vertical blend adds its own 3u 255 to the convex combination of the two: 6u 255 <= 8u 255.
    A pixel is decided when |frac(v) - 0.5| > delta."""
    H0, W0 = frame.shape[:2]
    im = frame.astype(np.float64)
    fy, y0, y1, wy, ym, yp = _axis(H0, new_h)
    fx, x0, x1, wx, xm, xp = _axis(W0, new_w)
    wy_, wx_ = wy[:, None, None], wx[None, :, None]
    g = lambda ys, xs: im[ys][:, xs]
    p00, p01, p10, p11 = g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)
    v = (1 - wy_) * ((1 - wx_) * p00 + wx_ * p01) + wy_ * ((1 - wx_) * p10 + wx_ * p11)
    ex, ey = 4 * U * np.maximum(np.abs(fx), 1.0), 4 * U * np.maximum(np.abs(fy), 1.0)
    Dx = np.maximum(np.abs(p00 - p01), np.abs(p10 - p11))
    Dy = np.maximum(np.abs(p00 - p10), np.abs(p01 - p11))
    # coordinates within their error of an integer: the neighbouring cell's pairs count too (rows y0 / y1 may move as well: take every pair of the 4 x 4 support)
    near_x = (np.minimum(wx, 1 - wx) <= ex)
    near_y = (np.minimum(wy, 1 - wy) <= ey)
    if near_x.any() or near_y.any():
        ys, xs = [ym, y0, y1, yp], [xm, x0, x1, xp]
        dx_all = np.max([np.abs(g(a, xs[j]) - g(a, xs[j + 1])) for a in ys for j in range(3)], 0)
        dy_all = np.max([np.abs(g(ys[j], b) - g(ys[j + 1], b)) for b in xs for j in range(3)], 0)
        near = (near_y[:, None] | near_x[None, :])[:, :, None]
        Dx, Dy = np.where(near, dx_all, Dx), np.where(near, dy_all, Dy)
    delta = ex[None, :, None] * Dx + ey[:, None, None] * Dy + 8 * U * 255.0
    return v, delta


def decided(v, delta):
    return np.abs(v - np.floor(v) - 0.5) > delta


# ---------------------------------------------------------------------------------------------------------------- geometry table
# name, frames, (H0, W0), img_size, stride, (H, W, new_h, new_w, top, left) as Detector.letterbox_params gives them (written out, so that a change of the rule
# shows: test_preprocess_cpu.py::test_geometry_table), the stem instantiation a yolov7-w6 plan of (H, W) runs it through (None: stand-alone kernel only), and
# whether every float32 operation of the resize is exact (scale 2, 1/2, 3/2).
class Row:
    def __init__(self, name, B, shape, img_size, stride, geom, stem, exact=False, what="", noise_span=256):
        self.name, self.B, self.shape, self.img_size, self.stride, self.geom, self.stem, self.exact, self.what = name, B, shape, img_size, stride, geom, stem, exact, what
        self.noise_span = noise_span        # grey levels the noise image spans
        self.resampled = (geom[2], geom[3]) != tuple(shape)

    def __repr__(self):
        return self.name


DIRECT, RESIZE = "stem_u8<direct>", "stem_u8<letterbox-resize>"
GEOMETRIES = [
    Row("23x37", 1, (23, 37), 128, 64, (128, 128, 80, 128, 24, 0), RESIZE, what="upscale x3.46: both y clamps and both x clamps are live"),
    Row("37x23", 1, (37, 23), 128, 64, (128, 128, 128, 80, 0, 24), RESIZE, what="the same with left != 0"),
    Row("157x211", 1, (157, 211), 128, 64, (128, 128, 95, 128, 16, 0), RESIZE, what="odd sizes, irrational scale, bottom = 17 != top"),
    Row("211x157", 1, (211, 157), 128, 64, (128, 128, 128, 95, 0, 16), RESIZE, what="portrait, right = 17 != left"),
    Row("157x211/s32", 1, (157, 211), 128, 32, (96, 128, 95, 128, 0, 0), None, what="top = 0, bottom = 1 (yolov7-tiny's stride)"),
    Row("128x256", 1, (128, 256), 128, 64, (64, 128, 64, 128, 0, 0), RESIZE, exact=True, what="exact x2 shrink: every weight 0.5, a quarter of the pixels are ties"),
    Row("64x64", 1, (64, 64), 128, 64, (128, 128, 128, 128, 0, 0), RESIZE, exact=True, what="exact x2 enlargement: weights 0.25 / 0.75"),
    Row("1x5", 1, (1, 5), 64, 64, (64, 64, 13, 64, 25, 0), RESIZE, what="one source row: both taps clamp to it"),
    Row("5x1", 1, (5, 1), 64, 64, (64, 64, 64, 13, 0, 25), RESIZE, what="one source column"),
    Row("90x128", 1, (90, 128), 128, 64, (128, 128, 90, 128, 19, 0), DIRECT, what="no resampling, top odd"),
    Row("128x90", 1, (128, 90), 128, 64, (128, 128, 128, 90, 0, 19), RESIZE, what="left odd: letterbox-resize without resampling (weights exactly 0)"),
    Row("128x91", 1, (128, 91), 128, 64, (128, 128, 128, 91, 0, 18), RESIZE, what="W0 odd: the same fallback, left 18 != right 19"),
    Row("128x4", 1, (128, 4), 128, 64, (128, 64, 128, 4, 0, 30), DIRECT, what="direct with W0 - 2 = 2: the x clamp next to the pad"),
    Row("3x157x211", 3, (157, 211), 128, 64, (128, 128, 95, 128, 16, 0), RESIZE, what="batch stride of the source and of the output"),
    Row("9x300x300", 9, (300, 300), 512, 64, (512, 512, 512, 512, 0, 0), RESIZE, what="2304 tiles > 2048: a second tile per workgroup, ragged"),
    Row("9x512x512", 9, (512, 512), 512, 64, (512, 512, 512, 512, 0, 0), DIRECT, what="the same for direct"),
    Row("1500x1530/s32", 1, (1500, 1530), 1536, 32, (1536, 1536, 1506, 1536, 15, 0), None, what="2.36 M pixels > 8192 * 256: second grid-stride round (reorg = 0)",
        noise_span=64),     # delta grows with the coordinate (up to 1500 here): full-range noise would leave 8.6 % of the pixels undecided, 64 levels leave about 2 %
    Row("1080x1920", 1, (1080, 1920), 1280, 64, (768, 1280, 720, 1280, 24, 0), None, exact=True, what="scale exactly 1.5 at source coordinates near 1900"),
]
ROWS = {r.name: r for r in GEOMETRIES}
KINDS = ("noise", "sines")


def frames_for(row, kind):
    """(B, H0, W0, 3) uint8, seeded by the row and the kind; every frame of a batch differs from the others.
    noise: every tap matters.  sines: a smooth product of sines per channel (realistic gradients)."""
    B, (H0, W0) = row.B, row.shape
    rng = np.random.default_rng([GEOMETRIES.index(row), KINDS.index(kind), 20240])
    if kind == "noise":
        lo = (256 - row.noise_span) // 2
        return rng.integers(lo, lo + row.noise_span, (B, H0, W0, 3), dtype=np.uint8)
    y, x = np.arange(H0, dtype=np.float64)[None, :, None, None], np.arange(W0, dtype=np.float64)[None, None, :, None]
    ky, kx = rng.uniform(0.02, 0.3, (B, 1, 1, 3)), rng.uniform(0.02, 0.3, (B, 1, 1, 3))
    py, px = rng.uniform(0, 6.28, (B, 1, 1, 3)), rng.uniform(0, 6.28, (B, 1, 1, 3))
    return np.rint(127.5 + 127.5 * np.sin(ky * y + py) * np.sin(kx * x + px)).astype(np.uint8)


def stem_kernel_rule(shape, geom):
    """csrc/y7t_stem.hip::y7t_stem_u8_launch: the direct loader needs the network's geometry up to padding and 2-byte aligned pixel pairs"""
    (H0, W0), (_, _, new_h, new_w, _, left) = shape, geom
    return DIRECT if (new_h == H0 and new_w == W0 and left % 2 == 0 and W0 % 2 == 0 and W0 >= 2) else RESIZE
