"""Plain helpers for the tests of augmented inference (test-time augmentation): restatements of the reference's `scale_img` (utils/torch_utils.py:247-257) and of the
augmented branch of `Model.forward` (models/yolo.py:301-317), the pass-size arithmetic, a float64 bilinear on the float32 geometry csrc/y7t_tta.h states, the float32
restatement of the de-scale / de-flip, the network-input layout, and planted Detect head scenes for the appending decode.  No test lives here."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import post_scenes as ps

SCALES, FLIPS = (1, 0.83, 0.67), (None, 3, None)      # models/yolo.py:304-305
PAD = 0.447                                           # utils/torch_utils.py:257
F32 = np.float32

# (gs, (H, W)) -> per pass ((hs, ws) resampled, (Hp, Wp) padded): the sizes the reference's expressions give, written out (the table the feature was specified with)
TABLE = {
    (32, (128, 192)): (((128, 192), (128, 192)), ((106, 159), (128, 160)), ((85, 128), (96, 160))),      # the 0.67 pass: 128.64 rounds up to 5 cells, a 32-px pad column
    (32, (64, 96)): (((64, 96), (64, 96)), ((53, 79), (64, 96)), ((42, 64), (64, 96))),                  # three passes, ONE plan
    (64, (64, 64)): (((64, 64), (64, 64)), ((53, 53), (64, 64)), ((42, 42), (64, 64))),                  # one plan, one arena
    (64, (256, 256)): (((256, 256), (256, 256)), ((212, 212), (256, 256)), ((171, 171), (192, 192))),    # two plans
    (64, (1280, 1280)): (((1280, 1280), (1280, 1280)), ((1062, 1062), (1088, 1088)), ((857, 857), (896, 896))),
}

# (H, W) source -> (hs, ws) resampled inside (Hp, Wp): (1, 1) results, odd sizes, hs == H (a pad and nothing else), and the table's passes
GEOMS = [((3, 5), (1, 1), (2, 2)),
         ((1, 1), (1, 1), (2, 4)),
         ((37, 53), (30, 43), (32, 64)),                   # (37, 53) at gs 32, ratio 0.83
         ((37, 53), (24, 35), (32, 64)),                   # ... ratio 0.67
         ((64, 96), (64, 96), (64, 128)),                  # no resampling, only a pad
         ((64, 96), (64, 96), (64, 96)),                   # ... not even that: the flip alone
         ((128, 192), (106, 159), (128, 160)),
         ((128, 192), (85, 128), (96, 160)),
         ((64, 96), (53, 79), (64, 96)),
         ((64, 96), (42, 64), (64, 96)),
         ((64, 64), (53, 53), (64, 64)),
         ((64, 64), (42, 42), (64, 64)),
         ((256, 256), (212, 212), (256, 256)),
         ((256, 256), (171, 171), (192, 192))]
GEOM_IDS = ["%dx%d-to-%dx%d-in-%dx%d" % (g[0] + g[1] + g[2]) for g in GEOMS]


def pass_sizes(H, W, ratio, gs):
    """scale_img's two sizes in Python doubles, exactly as utils/torch_utils.py:252-256 writes them -> ((hs, ws), (Hp, Wp))"""
    if ratio == 1.0:
        return (H, W), (H, W)
    return (int(H * ratio), int(W * ratio)), tuple(math.ceil(x * ratio / gs) * gs for x in (H, W))


def scale_img_ref(img, ratio=1.0, same_shape=False, gs=32):
    """utils/torch_utils.py:247-257, restated: img (B, 3, H, W) float32 tensor"""
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    img = F.interpolate(img, size=s, mode="bilinear", align_corners=False)
    if not same_shape:
        h, w = [math.ceil(x * ratio / gs) * gs for x in (h, w)]
    return F.pad(img, [0, w - s[1], 0, h - s[0]], value=PAD)


def augment_ref(forward_once, x, gs, scales=SCALES, flips=FLIPS):
    """models/yolo.py:301-317, restated around any `forward_once(xi) -> (B, A_i, no)` callable: -> torch.cat over the passes, (B, A0 + A1 + A2, no)"""
    img_size = x.shape[-2:]
    y = []
    for si, fi in zip(scales, flips):
        xi = scale_img_ref(x.flip(fi) if fi else x, si, gs=gs)
        yi = forward_once(xi)
        yi[..., :4] /= si
        if fi == 2:
            yi[..., 1] = img_size[0] - yi[..., 1]
        elif fi == 3:
            yi[..., 0] = img_size[1] - yi[..., 0]
        y.append(yi)
    return torch.cat(y, 1)


def transform_ref(xywh, scale, flip, extent):
    """the float32 restatement of yolo.py:311-315 on (..., 4) rows of {x, y, w, h}: a float32 division by float32(scale), then extent - x (flip 3) or extent - y (flip 2)"""
    c = np.array(xywh, F32, copy=True)
    c[..., :4] = c[..., :4] / F32(scale)
    if flip == 3:
        c[..., 0] = F32(extent) - c[..., 0]
    elif flip == 2:
        c[..., 1] = F32(extent) - c[..., 1]
    return c


def float_image(img):
    """the (B, 3, H, W) float32 RGB image both sources stand for: a (B, H, W, 3) uint8 BGR frame is float32(u) / float32(255), channels reversed (k_input_layout's u8 branch)"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return np.ascontiguousarray((img.astype(F32) / F32(255.0))[..., ::-1].transpose(0, 3, 1, 2))
    return np.ascontiguousarray(img, F32)


def taps_f32(n_in, n_out):
    """the geometry of csrc/y7t_tta.h in float32, operation by operation: -> i0, i1 (int), l1 (float32)"""
    scale = F32(n_in) / F32(n_out)
    src = scale * (np.arange(n_out, dtype=F32) + F32(0.5)) - F32(0.5)
    src = np.maximum(src, F32(0))
    i0 = src.astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (src - i0.astype(F32)).astype(F32)


def bilinear64(img, flip, hs, ws):
    """float64 bilinear of the flipped float image on the float32 taps: (B, 3, H, W) -> (B, 3, hs, ws) float64.  The weights are the float32 l1 the device uses and
    1 - l1 taken EXACTLY, so that what separates the device's value from this one is its own float32 arithmetic and nothing else."""
    x = float_image(img).astype(np.float64)
    if flip == 2:
        x = x[:, :, ::-1]
    elif flip == 3:
        x = x[:, :, :, ::-1]
    H, W = x.shape[2:]
    y0, y1, ly = taps_f32(H, hs)
    x0, x1, lx = taps_f32(W, ws)
    ly, lx = ly.astype(np.float64)[None, None, :, None], lx.astype(np.float64)[None, None, None, :]
    r0 = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    r1 = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return (1 - ly) * r0 + ly * r1


def layout_ref(padded, reorg):
    """(B, 3, Hp, Wp) -> the network's NHWC input (B, Ho, Wo, ldout), same dtype: with ReOrg channel g * 3 + ch, g = (row parity) + 2 * (column parity), 12 + 4 zero
    channels; without, 3 + 5 zero channels"""
    B, _, Hp, Wp = padded.shape
    if not reorg:
        out = np.zeros((B, Hp, Wp, 8), padded.dtype)
        out[..., :3] = padded.transpose(0, 2, 3, 1)
        return out
    out = np.zeros((B, Hp // 2, Wp // 2, 16), padded.dtype)
    for g in range(4):
        out[..., g * 3:g * 3 + 3] = padded[:, :, (g & 1)::2, (g >> 1)::2].transpose(0, 2, 3, 1)
    return out


def pad_mask(hs, ws, Hp, Wp, reorg):
    """bool (Ho, Wo, ldout): True where the layout holds a pad cell (a colour channel of a pixel right of ws or below hs)"""
    m = np.zeros((1, 3, Hp, Wp), bool)
    m[:, :, hs:, :] = True
    m[:, :, :, ws:] = True
    return layout_ref(m, reorg)[0]


def zero_mask(Hp, Wp, reorg):
    """bool (Ho, Wo, ldout): True on the layout's zero channels"""
    return ~layout_ref(np.ones((1, 3, Hp, Wp), bool), reorg)[0]


def ulp_f16(v):
    """the spacing of fp16 at |v| (2^-24 in the subnormal range)"""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def source_image(kind, B, H, W, seed):
    """a seeded source of either kind: 'f32' (B, 3, H, W) float32 RGB in [0, 1] (0 and 1 included), 'u8' (B, H, W, 3) uint8 BGR"""
    rng = np.random.default_rng([seed, B, H, W, 5])
    if kind == "u8":
        return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    img = rng.random((B, 3, H, W), dtype=np.float32)
    img.reshape(-1)[::17] = 1.0
    img.reshape(-1)[5::23] = 0.0
    return img


# ------------------------------------------------------------------------------------------------ planted Detect heads, one set per pass (k_decode_append)
PASS_SHAPES = (((4, 6), (2, 3)), ((4, 5), (2, 3)), ((3, 5), (2, 2)))      # (ny, nx) per level of the three passes: 4 x 6, 4 x 5 and 3 x 5 cells at the fine level
PASS_NA, PASS_NO, PASS_B = 3, 9, 2


@functools.lru_cache(maxsize=None)
def decode_scenes(conf_thres=0.01, seed=0, obj_logit=None):
    """three head-logit scenes in the format of post_scenes.decode_scene (heads, strides, anchors, nl, na, no, B, A, shapes), one per pass, sharing strides and anchors
    (arbitrary, positive) as the passes of one detector do: N(0, 1.5) logits, the objectness shifted so that roughly half of the anchors pass at conf_thres
    (obj_logit: every objectness logit at that value), and no float64 objectness or confidence within post_scenes.BAND of conf_thres (rows are drawn again)."""
    rng = np.random.default_rng([seed, int(round(conf_thres * 1e4)), 77])
    nl, na, no, B = len(PASS_SHAPES[0]), PASS_NA, PASS_NO, PASS_B
    strides = rng.uniform(4, 40, nl).astype(F32)
    anchors = rng.uniform(5, 120, (nl, na, 2)).astype(F32)
    shift = F32(math.log(conf_thres / (1.0 - conf_thres)) + 0.7)      # about half of the objectness values above conf_thres
    out = []
    for shapes in PASS_SHAPES:
        heads = []
        for ny, nx in shapes:
            h = (rng.standard_normal((B, ny, nx, na, no)) * 1.5).astype(F32)
            h[..., 4] = obj_logit if obj_logit is not None else h[..., 4] + shift
            for _ in range(200):
                obj, conf = ps.scores64([h.reshape(B, ny, nx, na * no)], na, no)[0]
                bad = (np.abs(obj - conf_thres) < ps.BAND) | (np.abs(conf - conf_thres) < ps.BAND)
                if not bad.any():
                    break
                fresh = (rng.standard_normal((int(bad.sum()), no)) * 1.5).astype(F32)
                fresh[:, 4] = obj_logit if obj_logit is not None else fresh[:, 4] + shift
                h[bad] = fresh
            else:
                raise AssertionError("could not clear the band around conf_thres")
            heads.append(np.ascontiguousarray(h.reshape(B, ny, nx, na * no)))
        out.append({"heads": heads, "strides": strides, "anchors": anchors, "nl": nl, "na": na, "no": no, "B": B, "shapes": shapes,
                    "A": sum(na * ny * nx for ny, nx in shapes)})
    return tuple(out)


def decode_reference_tta(scenes, passes, conf_thres):
    """the restatement for planted heads: the oracle's Detect decode of every pass (oracle.detector_torch.decode_level), xywh through transform_ref, the passes
    concatenated, then the oracle's candidate filter.  passes: (scale, flip, extent) per scene.  -> per image: dict union row -> (xyxy, conf, cls, per-class conf)"""
    from oracle import detector_torch as dt
    ys = []
    for sc, (scale, flip, extent) in zip(scenes, passes):
        z = []
        for h, st, an in zip(sc["heads"], sc["strides"], sc["anchors"]):
            B, ny, nx, _ = h.shape
            x = torch.from_numpy(h.reshape(B, ny, nx, sc["na"], sc["no"])).permute(0, 3, 1, 2, 4).contiguous()
            z.append(dt.decode_level(x, torch.from_numpy(an), float(st)))
        y = torch.cat(z, 1).numpy()
        y[..., :4] = transform_ref(y[..., :4], scale, flip, extent)
        ys.append(y)
    dec = torch.from_numpy(np.concatenate(ys, 1))
    return [dt.candidates(dec[b], conf_thres) for b in range(scenes[0]["B"])]
