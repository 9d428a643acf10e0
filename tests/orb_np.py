"""tests/orb_np.py -- the NumPy restatement (integers and float64) of the feature-based camera-motion estimate, DESIGN.md section 4 "GMC / features":
plane -> FAST-9/16 -> mask -> capacity -> orientation -> smoothing -> rotated BRIEF -> Hamming best-two -> the reference's filters -> 2000 RANSAC hypotheses ->
closed-form refinement.  The device kernels (csrc/y7t_orb.hip) and their host build (tests/_hostsim/orb.py) are compared with this ARRAY-EQUAL, stage by stage.
Written for clarity, not speed: whole-array operations, the mask as the reference builds it (an image, with real NumPy slices)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_H = os.path.join(ROOT, "yolov7-tracker_amd", "csrc", "y7t_orb_pattern.h")
PATTERN_SEED = 0xB21EF
FAST_T, EDGE, HALF, N_HYP, MAX_KEYPOINTS = 20, 31, 15, 2000, 8192
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
TAPS = np.array([72, 134, 195, 222, 195, 134, 72], np.int64)      # 7 taps of exp(-i^2 / 8), sum 2^10; both passes, then (s + 2^19) >> 20
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3)]      # (dx, dy)
OK, NO_MATCHES, NOT_ENOUGH, NO_MODEL = 0, 1, 2, 3
WARNINGS = {NOT_ENOUGH: 'Warning: not enough matching points', NO_MODEL: 'Warning: find transform failed. Set warp as identity'}
EYE = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


# -- the pattern: one table, csrc/y7t_orb_pattern.h ---------------------------------------------------------------------------------------------------------
def generate_pattern():
    """BRIEF's isotropic Gaussian draw: 256 x (ax, ay, bx, by), sigma = 31 / 5, rounded to nearest, clipped to +-13"""
    rng = np.random.default_rng(PATTERN_SEED)
    return np.clip(np.rint(rng.normal(0.0, 31.0 / 5.0, (256, 4))), -13, 13).astype(np.int8)


def pattern_header_text():
    p = generate_pattern()
    rows = ["    " + " ".join("{%3d,%3d,%3d,%3d}," % tuple(int(v) for v in r) for r in p[i:i + 4]) for i in range(0, 256, 4)]
    return ("// y7t_orb_pattern.h -- GENERATED (tests/orb_np.py: pattern_header_text; tests/test_orb_cpu.py regenerates and compares it).  The 256 point pairs of the\n"
            "// rotated-BRIEF descriptor, our own draw: numpy.random.default_rng(0x%X).normal(0, 31 / 5, (256, 4)), rounded to nearest (half to even), clipped to +-13;\n"
            "// row i = {ax, ay, bx, by}, bit i of a descriptor = I(rot(a_i)) < I(rot(b_i)).  This is NOT OpenCV's learned bit_pattern_31_.\n"
            "#pragma once\n#include <stdint.h>\n#ifndef Y7T_ORB_TABLE\n#define Y7T_ORB_TABLE static const\n#endif\n"
            "Y7T_ORB_TABLE int8_t y7t_orb_pattern[256][4] = {\n%s\n};\n" % (PATTERN_SEED, "\n".join(rows)))


def read_pattern():
    """the table the kernels compile, parsed from the header"""
    body = open(PATTERN_H).read().split("y7t_orb_pattern[256][4] = {")[1]
    v = np.array([int(t) for t in re.findall(r"-?\d+", body)], np.int64)
    assert v.size == 1024
    return v.reshape(256, 4)


# -- 1. plane -------------------------------------------------------------------------------------------------------------------------------------------------
def gray(bgr):
    p = bgr.astype(np.int64)
    return ((114 * p[..., 0] + 587 * p[..., 1] + 299 * p[..., 2] + 500) // 1000).astype(np.uint8)


def _taps(n_src, n_dst):
    s = (np.arange(n_dst, dtype=np.float64) + 0.5) * (float(n_src) / float(n_dst)) - 0.5
    fl = np.floor(s)
    fr, a = s - fl, fl.astype(np.int64)
    lo, hi = a < 0, a >= n_src - 1
    a = np.where(lo, 0, np.where(hi, n_src - 1, a))
    fr = np.where(lo | hi, 0.0, fr)
    return a, np.minimum(a + 1, n_src - 1), fr


def plane(bgr, ds):
    g = gray(bgr)
    if ds <= 1:
        return g
    H, W = g.shape
    h, w = H // ds, W // ds
    x0, x1, fx = _taps(W, w)
    y0, y1, fy = _taps(H, h)
    G = g.astype(np.float64)
    fx, fy = fx[None, :], fy[:, None]
    top = (1.0 - fx) * G[y0][:, x0] + fx * G[y0][:, x1]
    bot = (1.0 - fx) * G[y1][:, x0] + fx * G[y1][:, x1]
    return np.floor((1.0 - fy) * top + fy * bot + 0.5).astype(np.uint8)


# -- 2. FAST-9/16 ---------------------------------------------------------------------------------------------------------------------------------------------
def fast_scores(P):
    """score map: the largest, over the 16 arcs of 9 contiguous ring pixels and both signs, of the arc's minimum signed difference to the centre; 0 unless > 20"""
    h, w = P.shape
    I = P.astype(np.int64)
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])
    best = np.zeros_like(c)
    for sign in (1, -1):
        for s in range(16):
            arc = np.stack([sign * d[(s + k) % 16] for k in range(9)]).min(0)
            best = np.maximum(best, arc)
    out = np.zeros((h, w), np.uint8)
    out[3:h - 3, 3:w - 3] = np.where(best > FAST_T, best, 0)
    return out


def nms(S):
    h, w = S.shape
    p = np.pad(S.astype(np.int64), 1)
    keep = S > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= S > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


# -- 3. mask (botsort.py:126-132, as the reference builds it) and ORB's border ---------------------------------------------------------------------------------
def det_boxes(dets, ds):
    if dets is None or len(dets) == 0:
        return np.zeros((0, 4), np.int64)
    q = np.asarray(dets, np.float32)[:, :4].astype(np.float64) / float(ds)
    q = np.where(np.isnan(q), 0.0, np.clip(q, -1e9, 1e9))
    return q.astype(np.int64)      # (truncation toward zero)


def mask_image(h, w, dets, ds):
    mask = np.zeros((h, w), np.uint8)
    mask[int(0.02 * h): int(0.98 * h), int(0.02 * w): int(0.98 * w)] = 255
    for tlbr in det_boxes(dets, ds):
        mask[tlbr[1]:tlbr[3], tlbr[0]:tlbr[2]] = 0
    edge = np.zeros((h, w), bool)
    edge[EDGE:h - EDGE, EDGE:w - EDGE] = True
    return (mask > 0) & edge


# -- 5. orientation, 6. smoothing, 7. descriptor ----------------------------------------------------------------------------------------------------------------
def moments(P, kp):
    """(n, 2) int64: m10, m01 over the disc on the unblurred plane"""
    dy, dx = np.mgrid[-HALF:HALF + 1, -HALF:HALF + 1]
    disc = np.abs(dx) <= np.array(UMAX)[np.abs(dy)]
    I = P.astype(np.int64)[kp[:, 1, None, None] + dy[None], kp[:, 0, None, None] + dx[None]] * disc[None]
    return np.stack([(I * dx[None]).sum((1, 2)), (I * dy[None]).sum((1, 2))], 1)


def direction(m):
    """(n, 2) float64: c, s"""
    m10, m01 = m[:, 0], m[:, 1]
    r = np.sqrt((m10 * m10 + m01 * m01).astype(np.float64))
    zero = r == 0.0
    r = np.where(zero, 1.0, r)
    return np.stack([np.where(zero, 1.0, m10.astype(np.float64) / r), np.where(zero, 0.0, m01.astype(np.float64) / r)], 1)


def smooth(P):
    h, w = P.shape
    p = np.pad(P.astype(np.int64), 3, mode="reflect")
    rows = sum(TAPS[k] * p[:, k:k + w] for k in range(7))
    cols = sum(TAPS[k] * rows[k:k + h] for k in range(7))
    return ((cols + (1 << 19)) >> 20).astype(np.uint8)


def descriptors(S, kp, cs):
    """(n, 8) uint32: bit i at word i // 32, position i % 32"""
    pat = read_pattern().astype(np.float64)
    c, s = cs[:, 0, None], cs[:, 1, None]

    def sample(px, py):
        rx = np.rint(px[None] * c - py[None] * s).astype(np.int64)
        ry = np.rint(px[None] * s + py[None] * c).astype(np.int64)
        return S[kp[:, 1, None] + ry, kp[:, 0, None] + rx]
    bits = sample(pat[:, 0], pat[:, 1]) < sample(pat[:, 2], pat[:, 3])
    if len(kp) == 0:
        return np.zeros((0, 8), np.uint32)
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def extract(bgr, ds=2, dets=None, max_keypoints=MAX_KEYPOINTS):
    """-> dict: plane, scores, keypoints (n, 2) int (x, y) row-major, total, truncated, moments, smooth, desc, h, w"""
    P = plane(np.ascontiguousarray(bgr), ds)
    h, w = P.shape
    S = fast_scores(P)
    keep = nms(S) & mask_image(h, w, dets, ds)
    yx = np.argwhere(keep)
    total = len(yx)
    kp = yx[:max_keypoints, ::-1].astype(np.int64)
    m = moments(P, kp)
    G = smooth(P)
    return dict(plane=P, scores=S, keep=keep, kp=kp, total=total, truncated=int(total > max_keypoints), moments=m, smooth=G,
                desc=descriptors(G, kp, direction(m)), h=h, w=w)


# -- 8. matching ------------------------------------------------------------------------------------------------------------------------------------------------
def hamming(a, b):
    ua = np.unpackbits(np.ascontiguousarray(a, "<u4").view(np.uint8), axis=1).astype(np.int32)
    ub = np.unpackbits(np.ascontiguousarray(b, "<u4").view(np.uint8), axis=1).astype(np.int32)
    return ua @ (1 - ub).T + (1 - ua) @ ub.T


def best_two(prev_desc, cur_desc):
    """(n_prev, 4) int: j1, d1, j2, d2, candidates ordered by (distance, index)"""
    d = hamming(prev_desc, cur_desc)
    o = np.argsort(d, axis=1, kind="stable")[:, :2]
    r = np.arange(len(d))
    return np.stack([o[:, 0], d[r, o[:, 0]], o[:, 1], d[r, o[:, 1]]], 1).astype(np.int64)


# -- 9. filters (botsort.py:169-195) -------------------------------------------------------------------------------------------------------------------------------
def mean_std(d):
    """from the exact integer sums, one fixed float64 formula: mean = S / n, std = sqrt(n S2 - S^2) / n (np.std differs in the last bits only)"""
    n, s, s2 = len(d), int(d.sum()), int((d * d).sum())
    return np.float64(s) / np.float64(n), np.sqrt(np.float64(n * s2 - s * s)) / np.float64(n)


def filters(m, prev_kp, cur_kp, h, w):
    """-> (good (n_good, 4) int: px, py, cx, cy in the order of the previous keypoints; n_first, the survivors of the ratio and distance tests)"""
    ok = m[:, 1].astype(np.float64) < 0.9 * m[:, 3].astype(np.float64)
    p, c = prev_kp, cur_kp[m[:, 0]]
    dx, dy = p[:, 0] - c[:, 0], p[:, 1] - c[:, 1]
    ok &= (np.abs(dx).astype(np.float64) < 0.25 * float(w)) & (np.abs(dy).astype(np.float64) < 0.25 * float(h))
    if not ok.any():
        return np.zeros((0, 4), np.int64), 0
    mx, sx = mean_std(dx[ok])
    my, sy = mean_std(dy[ok])
    good = ok & ((dx.astype(np.float64) - mx) < 2.5 * sx) & ((dy.astype(np.float64) - my) < 2.5 * sy)
    return np.concatenate([p[good], c[good]], 1).astype(np.int64), int(ok.sum())


# -- 10. RANSAC ------------------------------------------------------------------------------------------------------------------------------------------------------
def fmix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def pick(k, c, n):
    """index c (0 or 1) of hypothesis k among n points: fmix32(((2k + c) * 0x9E3779B1) ^ (n * 0x85EBCA77)) mod n"""
    with np.errstate(over="ignore"):
        u = (np.asarray(2 * k + c).astype(np.uint32) * np.uint32(0x9E3779B1)) ^ (np.uint32(n) * np.uint32(0x85EBCA77))
        return (fmix32(u) % np.uint32(n)).astype(np.int64)


def hypothesis_inliers(good, k):
    """boolean inlier row of hypothesis k (all False for a degenerate pair), in exact integers: with D = dx^2 + dy^2 of the pair's source points, D * model(p) is an
    integer vector, and the point is an inlier iff |D model(p) - D q|^2 <= 9 D^2"""
    n = len(good)
    i, j = int(pick(k, 0, n)), int(pick(k, 1, n))
    x1, y1, u1, v1 = (int(t) for t in good[i])
    x2, y2, u2, v2 = (int(t) for t in good[j])
    dx, dy, ex, ey = x2 - x1, y2 - y1, u2 - u1, v2 - v1
    D = dx * dx + dy * dy
    if D == 0:
        return np.zeros(n, bool)
    A, B = dx * ex + dy * ey, dx * ey - dy * ex
    g = good.astype(object)      # Python integers: no overflow to think about
    rx = A * (g[:, 0] - x1) - B * (g[:, 1] - y1) - D * (g[:, 2] - u1)
    ry = B * (g[:, 0] - x1) + A * (g[:, 1] - y1) - D * (g[:, 3] - v1)
    return np.array([a * a + b * b <= 9 * D * D for a, b in zip(rx, ry)], bool)


def all_hypotheses(good):
    """(2000, n) boolean: hypothesis_inliers for every k at once, in int64.  A residual component above 3 D is no inlier; below that the squares stay under 2^58
    (coordinates are below 2^13), so nothing overflows.  tests/test_orb_cpu.py compares rows of this with hypothesis_inliers' Python integers."""
    n = len(good)
    k = np.arange(N_HYP)
    p, q = good[pick(k, 0, n)], good[pick(k, 1, n)]
    d = q - p
    D = d[:, 0] ** 2 + d[:, 1] ** 2
    A, B = d[:, 0] * d[:, 2] + d[:, 1] * d[:, 3], d[:, 0] * d[:, 3] - d[:, 1] * d[:, 2]
    r = good[None, :, :] - p[:, None, :]                                    # (2000, n, 4): x - x1, y - y1, u - u1, v - v1
    A, B, D = A[:, None], B[:, None], D[:, None]
    rx = np.abs(A * r[..., 0] - B * r[..., 1] - D * r[..., 2])
    ry = np.abs(B * r[..., 0] + A * r[..., 1] - D * r[..., 3])
    small = (rx <= 3 * D) & (ry <= 3 * D)
    rx, ry = np.where(small, rx, 0), np.where(small, ry, 0)
    return small & (rx * rx + ry * ry <= 9 * D * D) & (D != 0)


def ransac(good):
    """-> (counts (2000,), winner k, inlier row of the winner)"""
    rows = all_hypotheses(good)
    counts = rows.sum(1).astype(np.int64)
    k = int(np.argmax(counts))      # (the first of the largest)
    return counts, k, rows[k]


# -- 11. refinement ----------------------------------------------------------------------------------------------------------------------------------------------------
def refine(pts, ds):
    """closed-form least-squares similarity over (n, 4) integer points, from exact integer sums -> (6,) float64 or None when the source points coincide"""
    g = pts.astype(object)
    n = len(g)
    x, y, u, v = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    sx, sy, su, sv = int(x.sum()), int(y.sum()), int(u.sum()), int(v.sum())
    q = n * int((x * x + y * y).sum()) - sx * sx - sy * sy
    sa = n * int((x * u + y * v).sum()) - sx * su - sy * sv
    sb = n * int((x * v - y * u).sum()) - sx * sv + sy * su
    if q == 0:
        return None
    f = np.float64
    a, b = f(sa) / f(q), f(sb) / f(q)
    tx = ((f(su) - a * f(sx)) + b * f(sy)) / f(n)
    ty = ((f(sv) - b * f(sx)) - a * f(sy)) / f(n)
    return np.array([a, 0.0 - b, tx * f(ds), b, a, ty * f(ds)], np.float64)


def estimate(prev, cur, ds=2):
    """prev, cur: dicts of extract().  -> dict: warp (6,), status (6,) = n_prev, n_cur, n_good, n_inliers, flag, truncated, and the intermediates"""
    h, w = cur["h"], cur["w"]
    n_prev, n_cur = len(prev["kp"]), len(cur["kp"])
    out = dict(warp=EYE.copy(), matches=None, good=np.zeros((0, 4), np.int64), counts=None, winner=-1)
    trunc = cur["truncated"] | (prev["truncated"] << 1)

    def done(flag, n_good=0, n_in=0):
        out["status"] = np.array([n_prev, n_cur, n_good, n_in, flag, trunc], np.float64)
        return out
    if n_prev == 0 or n_cur < 2:
        return done(NO_MATCHES)
    out["matches"] = best_two(prev["desc"], cur["desc"])
    out["good"], out["n_first"] = filters(out["matches"], prev["kp"], cur["kp"], h, w)
    n_good = len(out["good"])
    if n_good <= 4:
        return done(NOT_ENOUGH, n_good)
    out["counts"], out["winner"], inl = ransac(out["good"])
    n_in = int(inl.sum())
    warp = refine(out["good"][inl], ds) if n_in >= 2 else None
    if warp is None:
        return done(NO_MODEL, n_good, n_in)
    out["warp"] = warp
    return done(OK, n_good, n_in)


class Features:
    """the whole estimator, frame after frame (what GMC('features') does with a backend)"""

    def __init__(self, ds=2, max_keypoints=MAX_KEYPOINTS):
        self.ds, self.cap, self.prev, self.last = ds, max_keypoints, None, None

    def apply(self, bgr, dets=None):
        cur = extract(bgr, self.ds, dets, self.cap)
        if self.prev is None:
            self.prev = cur
            return EYE.copy().reshape(2, 3)
        self.last = estimate(self.prev, cur, self.ds)
        self.prev = cur
        return self.last["warp"].reshape(2, 3)
