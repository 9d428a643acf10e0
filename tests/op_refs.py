"""Plain numpy float64 references of the small kernels around the convolutions -- the ReID op-list kernels of csrc/y7t_reid.hip one op at a time and the
input layout of csrc/y7t_post.hip -- with, next to every sum, the sum of the absolute values of its terms: the quantity a forward error bound is stated in.

tests/test_op_refs_cpu.py pins each of them against torch.nn.functional in float64, so that a wrong reference can neither hide nor invent a failure of the
GPU tests built on them (tests/test_reid_ops_gpu.py, tests/test_membound_gpu.py, tests/test_tiny_pinned_gpu.py).

Layouts are the device's: activations NHWC (N, H, W, C), dense weights (Co, kh, kw, Ci), depthwise weights (C, 3, 3).

The bound.  A length-K sum of products evaluated in fp32 in ANY order, every product and every partial sum rounded once (u = 2^-24), is off by at most
(K + 1) u sum|terms| to first order; a fused multiply-add only removes roundings.  The bars are therefore
    |got - ref| <= (K + 2) u sum|terms| + u |ref|
(one spare rounding for a trailing scale or division, and the representation of the result itself).  ReLU and max are 1-Lipschitz and exact."""
import zlib

import numpy as np

U32 = 2.0 ** -24


def rng_for(*key):
    """a generator seeded by the case itself (stable across processes, unlike hash() of a string)"""
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def sum_bound(K, abs_sum, ref):
    """worst-case forward bound of a length-K fp32 sum in any order (module docstring)"""
    return (K + 2) * U32 * np.asarray(abs_sum, np.float64) + U32 * np.abs(ref)


# ------------------------------------------------------------------------------------------------ input layout (csrc/y7t_post.hip)
def reorg(x_nchw):
    """ReOrg.forward (space-to-depth, cat order: even/even, odd/even, even/odd, odd/odd rows/columns)"""
    return np.concatenate([x_nchw[..., ::2, ::2], x_nchw[..., 1::2, ::2], x_nchw[..., ::2, 1::2], x_nchw[..., 1::2, 1::2]], 1)


def input_layout(img, is_u8, do_reorg, ldout):
    """y7t_input_layout: (B, 3, H, W) float32 RGB, or (B, H, W, 3) uint8 BGR (BGR -> RGB, / 255 in fp32: one correctly rounded division), -> NHWC float16 with
    ldout channels, the pad channels zero.  Exact: a conversion and at most one IEEE division on both sides."""
    if is_u8:
        x = (img[..., ::-1].astype(np.float32) / np.float32(255)).astype(np.float16).transpose(0, 3, 1, 2)
    else:
        x = img.astype(np.float16)
    if do_reorg:
        x = reorg(x)
    x = x.transpose(0, 2, 3, 1)
    out = np.zeros(x.shape[:3] + (ldout,), np.float16)
    out[..., :x.shape[3]] = x
    return out


# ------------------------------------------------------------------------------------------------ ReID op list, fp32 kernels
def _pad_hw(x, p, value=0.0):
    return np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)), constant_values=value) if p else x


def conv(x, w, bias, k, s, p, relu):
    """k_reid_conv.  x (N, H, W, Ci), w (Co, k, k, Ci), bias (Co) or None -> (ref, sum|terms|, K) with K = k k Ci products (+ the bias)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, H, W, Ci = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = _pad_hw(x, p)
    ref = np.zeros((N, Ho, Wo, w.shape[0]))
    ab = np.zeros_like(ref)
    for kh in range(k):
        for kw in range(k):
            tap = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
            ref += tap @ w[:, kh, kw].T
            ab += np.abs(tap) @ np.abs(w[:, kh, kw]).T
    K = k * k * Ci
    if bias is not None:
        ref, ab, K = ref + np.asarray(bias, np.float64), ab + np.abs(np.asarray(bias, np.float64)), K + 1
    return (np.maximum(ref, 0.0) if relu else ref), ab, K


def dwconv3(x, w, bias, relu):
    """k_reid_dwconv3: depthwise 3x3, padding 1.  w (C, 3, 3) -> (ref, sum|terms|, K = 10)"""
    x, w, bias = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    N, H, W, C = x.shape
    xp = _pad_hw(x, 1)
    ref, ab = np.zeros_like(x) + bias, np.zeros_like(x) + np.abs(bias)
    for kh in range(3):
        for kw in range(3):
            tap = xp[:, kh:kh + H, kw:kw + W]
            ref += tap * w[:, kh, kw]
            ab += np.abs(tap * w[:, kh, kw])
    return (np.maximum(ref, 0.0) if relu else ref), ab, 10


def maxpool3s2(x, relu_first=False):
    """k_reid_pool mode 0 / k_h_maxpool3s2_relu: MaxPool2d(3, 2, padding=1) with -inf padding (after a ReLU for the fp16 kernel); exact"""
    x = np.asarray(x, np.float64)
    if relu_first:
        x = np.maximum(x, 0.0)
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    xp = _pad_hw(x, 1, -np.inf)
    out = np.full((N, Ho, Wo, C), -np.inf)
    for kh in range(3):
        for kw in range(3):
            out = np.maximum(out, xp[:, kh:kh + (Ho - 1) * 2 + 1:2, kw:kw + (Wo - 1) * 2 + 1:2])
    return out


def avgpool2(x):
    """k_reid_pool mode 1: AvgPool2d(2) (floor) -> (ref, sum|terms|, K = 4)"""
    x = np.asarray(x, np.float64)
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    t = x[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C)
    return t.sum((2, 4)) * 0.25, np.abs(t).sum((2, 4)) * 0.25, 4


def gap(x):
    """k_reid_gap: mean over the map.  x (N, HW, C) -> (ref (N, C), sum|terms|, K = HW)"""
    x = np.asarray(x, np.float64)
    return x.mean(1), np.abs(x).mean(1), x.shape[1]


def gate(pooled, w1, b1, w2, b2, pooled_err=0.0):
    """k_reid_gate: sigmoid(fc2(relu(fc1(pooled)))), w1 (R, C), w2 (C, R) -> (ref (N, C), bound).  The bound is the sum bound carried through both layers
    (pooled_err: what the pooled vector may already be off by), times the sigmoid's slope (<= 1/4), plus 4 u for expf and the division."""
    p, w1, b1, w2, b2 = (np.asarray(a, np.float64) for a in (pooled, w1, b1, w2, b2))
    R, C = w1.shape
    a1 = p @ w1.T + b1
    e1 = np.broadcast_to(pooled_err, p.shape) @ np.abs(w1).T + sum_bound(C + 1, np.abs(p) @ np.abs(w1).T + np.abs(b1), a1)
    h = np.maximum(a1, 0.0)
    a2 = h @ w2.T + b2
    e2 = e1 @ np.abs(w2).T + sum_bound(R + 1, h @ np.abs(w2).T + np.abs(b2), a2)
    return 1.0 / (1.0 + np.exp(-a2)), 0.25 * e2 + 4 * U32


def scale_acc(x, g, acc=None):
    """k_reid_scale_acc: (acc +) x * gate[n][c].  x (N, HW, C), g (N, C) -> (ref, sum|terms|, K = 1 or 2)"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    v = x * g[:, None, :]
    if acc is None:
        return v, np.abs(v), 1
    acc = np.asarray(acc, np.float64)
    return acc + v, np.abs(acc) + np.abs(v), 2


def add_relu(a, b):
    """k_reid_add_relu: relu(a + b) -> (ref, sum|terms|, K = 2)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.maximum(a + b, 0.0), np.abs(a) + np.abs(b), 2


def fc(x, w, bias, relu):
    """k_reid_fc: x (N, C), w (O, C) -> (ref, sum|terms|, K = C + 1)"""
    x, w, bias = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    ref = x @ w.T + bias
    return (np.maximum(ref, 0.0) if relu else ref), np.abs(x) @ np.abs(w).T + np.abs(bias), x.shape[1] + 1


def l2norm(x):
    """k_reid_l2norm: x / |x|_2 per row -> (ref, sum|terms|, K = C).  The C squares are positive, so their fp32 sum is RELATIVELY accurate to (C + 1) u, its
    root to half of that, and the quotient adds one rounding: the error is at most (C + 2) u |ref|, i.e. the sum bound with sum|terms| = |ref|."""
    x = np.asarray(x, np.float64)
    ref = x / np.sqrt((x * x).sum(1, keepdims=True))
    return ref, np.abs(ref), x.shape[1]


# ------------------------------------------------------------------------------------------------ ReID op list, fp16 helpers
def h_pack(x):
    """k_h_pack: fp32 (N, H, W, 3) -> fp16 (N, H, W, 16), channels 3..15 zero; one fp32 -> fp16 rounding: exact"""
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape[:3] + (16,), np.float16)
    out[..., :3] = x.astype(np.float16)
    return out


def h_add_relu(a, b=None):
    """k_h_add_relu: float16(max(float32(a) + float32(b), 0)) (b None: relu(a)); exact"""
    a = np.asarray(a, np.float16)
    if b is None:
        return np.maximum(a, np.float16(0))
    return np.maximum(a.astype(np.float32) + np.asarray(b, np.float16).astype(np.float32), np.float32(0)).astype(np.float16)


def h_gap_l2norm(x):
    """k_h_gap_l2norm: fp16 (N, HW, C) -> mean over the map, then x / |x|_2 -> (ref (N, C), bound).  The mean of channel c is off by at most
    e_c = (HW + 2) u mean|x| (sum bound); the norm of the means by |e|_2 plus its own (C + 2) u relative error (see l2norm); the quotient adds one rounding:
    |got - ref| <= e_c / nrm + |ref_c| (|e|_2 / nrm + (C + 4) u)."""
    x = np.asarray(x, np.float64)
    HW, C = x.shape[1], x.shape[2]
    m = x.mean(1)
    e = (HW + 2) * U32 * np.abs(x).mean(1) + U32 * np.abs(m)
    nrm = np.sqrt((m * m).sum(1, keepdims=True))
    ref = m / nrm
    return ref, e / nrm + np.abs(ref) * (np.sqrt((e * e).sum(1, keepdims=True)) / nrm + (C + 4) * U32)


# ------------------------------------------------------------------------------------------------ the shapes both test files use
# (H, W, Ci, Co, k, s, p, bias, relu)
CONV_SHAPES = [
    (17, 9, 3, 16, 7, 2, 3, 1, 1),       # the stem's geometry on an odd map
    (6, 5, 24, 40, 1, 1, 0, 1, 0),       # 1x1 (run with both weight layouts)
    (6, 5, 8, 12, 3, 1, 1, 1, 1),
    (6, 5, 8, 12, 3, 2, 1, 1, 0),
    (6, 5, 16, 24, 1, 2, 0, 1, 0),       # DeepSORT's shortcut: 1x1 / stride 2 / no padding
    (6, 5, 8, 12, 3, 1, 1, 0, 1),        # no bias (b_off = -1)
    (6, 5, 24, 40, 1, 1, 0, 0, 0),
]
DWCONV_SHAPES = [(1, 1, 16), (2, 7, 16), (8, 4, 16)]                       # (H, W, C), each with relu 0 / 1
POOL_SHAPES = [(8, 4, 16), (7, 5, 16), (1, 1, 16)]                         # (H, W, C); the average pool skips 1 x 1
GAP_SHAPES = [(32, 128), (32, 96), (1, 16), (6, 300), (32, 512)]           # (HW, C): C | 256, C does not divide 256, one pixel, a ragged second grid.y slice, two full slices
GATE_SHAPES = [(16, 1), (64, 4), (96, 6), (256, 16)]                       # (C, R)
FC_SHAPES = [(128, 512), (20, 7)]                                          # (C, O), each with relu 0 / 1
L2NORM_SHAPES = [5, 256, 512, 700]
H_GAP_SHAPES = [(32, 64), (32, 512), (32, 1024)]                           # (HW, C)
