"""CPU: the float64 reference and the bar of the one-op convolution tests (tests/test_conv_forms_gpu.py; tests/test_conv_ref_cpu.py shows that the instrument has teeth).

Reference.  `conv_ref` is the convolution written out tap by tap in numpy float64 on the fp16 input values and the fp16-rounded weights, bias and activation in float64:
stride 1 and 2, k 1 and 3, pad = k // 2.  Channel slices are the caller's business (`concat_input` cuts the input slice and puts the nearest x2 of a half-resolution slice
into the upsampled channel range); `twin_ref` is the twin form (3x3 / stride 2, round to fp16, 1x1).  Next to every output it returns absum = sum_k |w_k x_k| + |b|.

Bar.  tests/teacher_forced.py::conv_tolerance(ref, absum, K, extra_tol) and no new number: 3e-4 + 6e-4 |ref| covers the fp16 store (2^-11 relative = 4.9e-4) and the
activation, 2 sqrt(K) 2^-24 absum the fp32 sum in any order; extra_tol = 2^-11 for the twin (the fp16 tensor between the layers may differ by one ulp per term).  fp32
outputs (Detect heads, split-K slabs) take the same function: its first two terms are loose there, so `f32_bound` -- the fp32-only bound of tests/op_refs.py,
(K + 2) 2^-24 absum + 2^-24 |ref| -- is printed beside it (printed, not asserted).

The SiLU of the device is v * rcp(1 + exp2(-log2e * v)) (csrc/y7t_conv_common.h::act_t).  With u = 2^-24: the product log2e * v is rounded once and log2e itself is a
rounded constant, so the exponent is off by at most 1.5 |log2e v| u and e = exp2(.) by the relative ln2 * 1.5 * 1.4427 |v| u < 1.5 |v| u, plus exp2's own ulp (2 u); the
sum 1 + e, the rcp (1 ulp) and the product round three more times.  e / (1 + e) <= 1 carries e's error into the sigmoid, so
        |silu_dev(v) - silu(v)| <= (1.5 |v| + 5) u |silu(v)|,
which for |v| <= 64 is below 6.1e-6 |silu(v)|: a hundredth of the bar's 6e-4 |ref| term.  For v < -64 silu is below 1e-26 in magnitude on both sides.  The pre-activation
error reaches the output through |silu'| <= 1.1.  So the SiLU needs no term of its own in the bar; `f32_bound` adds the line above when the activation is SiLU.

Decode.  `decode_bounds` is the Detect decode (models/yolo.py:49-56) in float64 from float64 logits, the restatement of oracle/detector_torch.py::decode_level on arrays,
with the per-anchor bounds that the logit bar leaves for objectness, scores and boxes (derived in its docstring); the candidate filter of non_max_suppression
(utils/general.py:629-662) is applied to them by the caller."""
import numpy as np

SILU, LEAKY = 1, 2
U24 = 2.0 ** -24


def activate(v, act):
    if act == SILU:
        return v / (1.0 + np.exp(-v))
    if act == LEAKY:
        return np.where(v > 0, v, 0.1 * v)
    return v


def pixel_rows(B, Ho, Wo, Mtile, seed, fraction=0.1):
    """the rows of a large case that are compared: every pixel of the first and the last `Mtile`-pixel tile of each image plus a seeded `fraction` of the rest"""
    hw = Ho * Wo
    keep = np.zeros(B * hw, bool)
    for b in range(B):
        keep[b * hw:b * hw + Mtile] = True
        keep[(b + 1) * hw - Mtile:(b + 1) * hw] = True
    keep[(B * hw - 1) // Mtile * Mtile:] = True                                      # the last tile of the launch, ragged or not
    keep |= np.random.default_rng(seed).random(B * hw) < fraction
    return np.nonzero(keep)[0]


def conv_ref(x, w, b, k, s, act, rows=None):
    """x (B, H, W, Cin) the fp16 input values; w (Cout, Cin, k, k) the fp16-rounded weights; b (Cout,).  -> (ref, absum), each (M, Cout) float64 with M = B * Ho * Wo in
    (b, ho, wo) order -- or (len(rows), Cout) for the pixel indices `rows`.  ref = act(conv + b), absum = sum |w x| + |b|."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert w.shape == (Cout, Cin, k, k) and k in (1, 3) and s in (1, 2)
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = np.zeros((B, H + 2 * p, W + 2 * p, Cin))
    xp[:, p:p + H, p:p + W] = x
    m = np.arange(B * Ho * Wo) if rows is None else np.asarray(rows)
    bi, ho, wo = m // (Ho * Wo), m % (Ho * Wo) // Wo, m % Wo
    acc, absum = np.zeros((len(m), Cout)), np.zeros((len(m), Cout))
    for kh in range(k):
        for kw in range(k):
            g = xp[bi, ho * s + kh, wo * s + kw]                                     # (n, Cin): the pixels under this tap
            acc += g @ w[:, :, kh, kw].T
            absum += np.abs(g) @ np.abs(w[:, :, kh, kw]).T
    return activate(acc + b, act), absum + np.abs(b)


def concat_input(buf, in_coff, Cin, up=None):
    """what a conv op reads: channels [in_coff, in_coff + Cin) of `buf` (B, H, W, ld); up = (lo, up_coff, up_c0, up_C): channels [up_c0, up_c0 + up_C) of that slice are
    never stored at full resolution -- they are pixel (y >> 1, x >> 1) of channels [up_coff, up_coff + up_C) of `lo` (B, H/2, W/2, ld2) (nn.Upsample(None, 2, 'nearest'))"""
    x = np.array(buf[..., in_coff:in_coff + Cin], np.float64)
    if up is not None:
        lo, up_coff, up_c0, up_C = up
        x[..., up_c0:up_c0 + up_C] = np.repeat(np.repeat(np.asarray(lo[..., up_coff:up_coff + up_C], np.float64), 2, axis=1), 2, axis=2)
    return x


def twin_ref(x, w1, b1, w2, b2, act, rows=None):
    """3x3 / stride 2 + act, rounded to fp16 (the tensor between the layers lives in LDS as fp16), then 1x1 + act.  -> (ref, absum of the second layer); K = C_mid"""
    B, H, W, _ = x.shape
    mid, _ = conv_ref(x, w1, b1, 3, 2, act)
    mid = mid.astype(np.float16).astype(np.float64).reshape(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, -1)
    return conv_ref(mid, w2, b2, 1, 1, act, rows)


def tolerance(ref, absum, K, extra_tol=0.0):
    """tests/teacher_forced.py::conv_tolerance on arrays"""
    import torch
    from tests.teacher_forced import conv_tolerance
    return conv_tolerance(torch.from_numpy(np.ascontiguousarray(ref)), torch.from_numpy(np.ascontiguousarray(absum)), K, extra_tol).numpy()


def f32_bound(ref, absum, K, act=0):
    """the fp32-only bound of tests/op_refs.py for a K-term sum kept in fp32 (+ the SiLU line of the module docstring)"""
    t = (K + 2) * U24 * absum + U24 * np.abs(ref)
    if act == SILU:
        t = 1.1 * t + (1.5 * 64 + 5) * U24 * np.abs(ref)
    return t


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol; inf when `got` holds a NaN or an infinity"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / tol).max())


# ------------------------------------------------------------------------------------------------ Detect decode + candidate filter
def decode_bounds(logits, tol, na, no, ny, nx, stride, anchors, row0=0):
    """the Detect decode in float64 with what a logit error of at most `tol` (same shape as `logits`: the conv bar per logit) can do to it, anchor by anchor.
    logits, tol (B, ny, nx, na * no); anchors (na, 2) in pixels.  With |sigmoid'| <= 1/4 a probability moves by at most tol / 4: that is the band of the objectness
    test.  A score is the product of two probabilities, both <= 1, so it moves by at most t_obj / 4 + t_cls / 4 -- the quarter of the logit bound once per factor.
    cx = (2 sx - 0.5 + x) stride moves by stride t_x / 2; w = (2 sw)^2 aw by 8 sw aw t_w / 4 <= 2 aw t_w; a corner cx -+ w / 2 by stride t_x / 2 + aw t_w (y alike),
    plus the fp32 evaluation of the decode itself: 8 ulp (2^-23) of |cx| + w + 1.
    -> dict of arrays over (B, ny, nx, na): cidx (ny, nx, na) = row0 + (a ny + y) nx + x, obj, d_obj, sc (.., nc), d_sc (.., nc), box (.., 4) xyxy, d_box (.., 4)"""
    v = np.asarray(logits, np.float64).reshape(-1, ny, nx, na, no)
    t = np.asarray(tol, np.float64).reshape(v.shape)
    sg = 1.0 / (1.0 + np.exp(-v))
    an = np.asarray(anchors, np.float64)
    yy, xx, aa = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(na), indexing="ij")
    obj, d_obj = sg[..., 4], t[..., 4] / 4
    sc, d_sc = sg[..., 5:] * obj[..., None], (t[..., 5:] + t[..., 4:5]) / 4
    cx, cy = (sg[..., 0] * 2 - 0.5 + xx) * stride, (sg[..., 1] * 2 - 0.5 + yy) * stride
    w, h = (sg[..., 2] * 2) ** 2 * an[aa, 0], (sg[..., 3] * 2) ** 2 * an[aa, 1]
    dx = stride * t[..., 0] / 2 + an[aa, 0] * t[..., 2] + 8 * 2.0 ** -23 * (np.abs(cx) + w + 1)
    dy = stride * t[..., 1] / 2 + an[aa, 1] * t[..., 3] + 8 * 2.0 ** -23 * (np.abs(cy) + h + 1)
    return dict(cidx=row0 + (aa * ny + yy) * nx + xx, obj=obj, d_obj=d_obj, sc=sc, d_sc=d_sc, box=np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1),
                d_box=np.stack([dx, dy, dx, dy], -1))


def append_candidates(found, B, cap, HoWo, BM=128, fault=None):
    """the slot bookkeeping of the fused Detect epilogue (csrc/y7t_conv.hip, EPI == 1) on the host.  found: list of (m, cidx) in any order, m the pixel row of the launch.
    Every 128-pixel workgroup counts its candidates per image, reserves ONE block per image with a single add to count[b] and ranks its candidates inside the block;
    a slot >= cap is dropped but counted.  -> (count (B,), slots (B, cap) of cidx, -1 where nothing was written).  fault: the two mistakes that
    tests/test_conv_ref_cpu.py plants ("two candidates share a slot": the second candidate of an image in a workgroup takes the first one's rank; "block based on the
    previous image's counter": lbase[i] read from count[b0 + i - 1])"""
    count, slots = np.zeros(B, np.int64), np.full((B, cap), -1, np.int64)
    tiles = {}
    for m, cidx in found:
        tiles.setdefault(m // BM, []).append((m // HoWo, cidx))
    for t in sorted(tiles):
        b0 = t * BM // HoWo
        lcount = {}
        ranked = []
        for b, cidx in tiles[t]:
            r = lcount.get(b - b0, 0)
            ranked.append((b, 0 if r == 1 and fault == "two candidates share a slot" else r, cidx))
            lcount[b - b0] = r + 1
        lbase = {}
        for i, c in lcount.items():
            lbase[i] = count[b0 + i - 1] if fault == "block based on the previous image's counter" and i > 0 else count[b0 + i]
            count[b0 + i] += c
        for b, rank, cidx in ranked:
            slot = lbase[b - b0] + rank
            if slot < cap:
                slots[b, slot] = cidx
    return count, slots
