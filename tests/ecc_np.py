"""tests/ecc_np.py -- TEST INFRASTRUCTURE ONLY: the yardstick of the camera-motion estimate.

A NumPy float64 restatement of what GMC.applyEcc of the reference asks OpenCV for (tracker/botsort.py:78-109: cvtColor BGR2GRAY, GaussianBlur 3x3 sigma 1.5,
resize to (W // 2, H // 2), findTransformECC with MOTION_EUCLIDEAN, 100 iterations, eps 1e-5, gaussFiltSize 1), in exact arithmetic: OpenCV's fixed-point
8-bit tables and the 1/32 px weights of warpAffine are NOT imitated (DESIGN.md section 4 "GMC / ECC").  Written from OpenCV's documented behaviour
(modules/video/src/ecc.cpp), independently of the kernels: whole-image array operations, two passes per iteration (the masked means first, the zero-mean
images second), no slabs.

`dtype`: the precision of the PER-PIXEL stage (warp coordinates, bilinear weights, samples, Jacobian row).  float64 is the yardstick; float32 is the same
program with that one stage rounded like the device's, which is how the tests MEASURE the noise float32 pixels cause (sums stay float64 in both)."""
import numpy as np

MAX_ITERS, EPS = 100, 1e-5                       # botsort.py:31-32
CONVERGED, EXHAUSTED, FAILED = 1, 2, 3


# ---- frame preparation -------------------------------------------------------------------------------------------------------------------------------
def gray(bgr):
    """Y = 0.114 B + 0.587 G + 0.299 R rounded half up -> int64 (integer arithmetic: a tie is decided exactly)"""
    b = bgr.astype(np.int64)
    return (114 * b[..., 0] + 587 * b[..., 1] + 299 * b[..., 2] + 500) // 1000


def _reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i) if n > 1 else np.zeros_like(i)


def gauss_taps():
    e = np.exp(-1.0 / 4.5)                       # getGaussianKernel(3, 1.5): exp(-x^2 / (2 sigma^2)) at x = -1, 0, 1, normalised
    a = e / (1.0 + 2.0 * e)
    return a, 1.0 - 2.0 * a


def blur(g):
    """3x3 Gaussian sigma 1.5, separable (rows, then columns), border reflect-101, rounded half up -> float64 integers"""
    a, b = gauss_taps()
    g = g.astype(np.float64)
    H, W = g.shape
    xs, ys = np.arange(W), np.arange(H)
    r = a * (g[:, _reflect101(xs - 1, W)] + g[:, _reflect101(xs + 1, W)]) + b * g
    v = a * (r[_reflect101(ys - 1, H)] + r[_reflect101(ys + 1, H)]) + b * r
    return np.floor(v + 0.5)


def _resize_taps(n_src, n_dst):
    s = (np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5
    i0 = np.floor(s)
    f = s - i0
    i0 = i0.astype(np.int64)
    f = np.where(i0 < 0, 0.0, f)
    i0 = np.maximum(i0, 0)
    f = np.where(i0 >= n_src - 1, 0.0, f)
    i0 = np.minimum(i0, n_src - 1)
    return i0, np.minimum(i0 + 1, n_src - 1), f


def resize(img, h, w):
    """cv2.resize(img, (w, h)), INTER_LINEAR: pixel centres, clamped, rounded half up -> float64 integers"""
    H, W = img.shape
    x0, x1, fx = _resize_taps(W, w)
    y0, y1, fy = _resize_taps(H, h)
    top = (1.0 - fx) * img[y0][:, x0] + fx * img[y0][:, x1]
    bot = (1.0 - fx) * img[y1][:, x0] + fx * img[y1][:, x1]
    return np.floor((1.0 - fy)[:, None] * top + fy[:, None] * bot + 0.5)


def gradients(I):
    """taps [-0.5, 0, 0.5], border reflect-101 -> gx, gy"""
    h, w = I.shape
    xs, ys = np.arange(w), np.arange(h)
    gx = 0.5 * (I[:, _reflect101(xs + 1, w)] - I[:, _reflect101(xs - 1, w)])
    gy = 0.5 * (I[_reflect101(ys + 1, h)] - I[_reflect101(ys - 1, h)])
    return gx, gy


def prepare(bgr, downscale=2):
    """-> (h, w, 3) float64 plane {I, gx, gy}: applyEcc's frame preparation + the gradients findTransformECC takes of the input image"""
    g = gray(np.asarray(bgr))
    H, W = g.shape
    if downscale > 1:
        I = resize(blur(g), H // downscale, W // downscale)
    else:
        I = g.astype(np.float64)
    gx, gy = gradients(I)
    return np.stack([I, gx, gy], axis=-1)


# ---- one iteration -----------------------------------------------------------------------------------------------------------------------------------
def _warp_sample(plane, p, dtype):
    """-> mask (bool), Iw, gxw, gyw, the Jacobian (h, w, 3): the per-pixel stage in `dtype`"""
    h, w = plane.shape[:2]
    f = dtype
    ct, st = f(np.cos(p[0])), f(np.sin(p[0]))
    tx, ty = f(p[1]), f(p[2])
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.astype(f), ys.astype(f)
    xw = ct * xs - st * ys + tx
    yw = st * xs + ct * ys + ty
    with np.errstate(invalid="ignore"):
        xr, yr = np.floor(xw + f(0.5)), np.floor(yw + f(0.5))
        mask = (xr >= 0) & (xr < w) & (yr >= 0) & (yr < h)
    xw, yw = np.where(mask, xw, f(0)), np.where(mask, yw, f(0))
    x0f, y0f = np.floor(xw), np.floor(yw)
    fx, fy = xw - x0f, yw - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    src = np.zeros((h + 2, w + 2, 3), f)                                   # constant 0 border
    src[1:-1, 1:-1] = plane.astype(f)
    p00, p01, p10, p11 = src[y0 + 1, x0 + 1], src[y0 + 1, x0 + 2], src[y0 + 2, x0 + 1], src[y0 + 2, x0 + 2]
    one = f(1)
    w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    val = w00[..., None] * p00 + w01[..., None] * p01 + w10[..., None] * p10 + w11[..., None] * p11
    Iw, gxw, gyw = val[..., 0], val[..., 1], val[..., 2]
    j0 = -gxw * (xs * st + ys * ct) + gyw * (xs * ct - ys * st)
    J = np.stack([j0, gxw, gyw], axis=-1)
    assert val.dtype == f and J.dtype == f
    return mask, Iw, J


def raw_sums(T, plane, p, dtype=np.float64):
    """the 21 raw sums over the mask, float64: N, sum I, sum I^2, sum T, sum T^2, sum I T, sum J (3), sum J I (3), sum J T (3), sum J J^T (00 01 02 11 12 22)"""
    mask, Iw, J = _warp_sample(plane, p, dtype)
    m = mask.astype(np.float64)
    I, J, T = Iw.astype(np.float64) * m, J.astype(np.float64) * m[..., None], np.asarray(T, np.float64) * m
    out = [m.sum(), I.sum(), (I * I).sum(), T.sum(), (T * T).sum(), (I * T).sum()]
    out += [J[..., k].sum() for k in range(3)] + [(J[..., k] * I).sum() for k in range(3)] + [(J[..., k] * T).sum() for k in range(3)]
    out += [(J[..., a] * J[..., b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return np.array(out)


def inv3(Hm):
    """cv::Mat::inv of a 3x3: the cofactor formula, zeros when the determinant is zero"""
    d = (Hm[0, 0] * (Hm[1, 1] * Hm[2, 2] - Hm[1, 2] * Hm[2, 1]) - Hm[0, 1] * (Hm[1, 0] * Hm[2, 2] - Hm[1, 2] * Hm[2, 0])
         + Hm[0, 2] * (Hm[1, 0] * Hm[2, 1] - Hm[1, 1] * Hm[2, 0]))
    if d == 0.0:
        return np.zeros((3, 3))
    c = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            s = [k for k in range(3) if k != j]
            c[j, i] = (-1.0) ** (i + j) * (Hm[r[0], s[0]] * Hm[r[1], s[1]] - Hm[r[0], s[1]] * Hm[r[1], s[0]])
    return c / d


class Failed(Exception):
    """what OpenCV throws: rho is NaN, or lambda_d <= 0"""


def iteration(T, plane, p, dtype=np.float64):
    """one Gauss-Newton iteration at p -> (rho, dp).  Two passes as ecc.cpp: the masked means and deviations, then the zero-mean images and their products."""
    mask, Iw, J = _warp_sample(plane, p, dtype)
    n = int(mask.sum())
    Iw, J, T = Iw.astype(np.float64), J.astype(np.float64) * mask[..., None], np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        mI, mT = (Iw[mask].mean(), T[mask].mean()) if n else (np.nan, np.nan)
        Izm, Tzm = np.where(mask, Iw - mI, 0.0), np.where(mask, T - mT, 0.0)
        sI, sT = (np.sqrt((Izm[mask] ** 2).mean()), np.sqrt((Tzm[mask] ** 2).mean())) if n else (np.nan, np.nan)
        img_norm, tmp_norm = np.sqrt(n * sI * sI), np.sqrt(n * sT * sT)
        Jf = J.reshape(-1, 3)
        Hm = Jf.T @ Jf
        JI, JT = Jf.T @ Izm.ravel(), Jf.T @ Tzm.ravel()
        corr = float(Tzm.ravel() @ Izm.ravel())
        rho = corr / (img_norm * tmp_norm)
        if not np.isfinite(rho):
            raise Failed("rho")
        Hi = inv3(Hm)
        lam_n = img_norm * img_norm - JI @ (Hi @ JI)
        lam_d = corr - JI @ (Hi @ JT)
        if lam_d <= 0.0:
            raise Failed("lambda_d")
        lam = lam_n / lam_d
        dp = Hi @ (Jf.T @ (lam * Tzm - Izm).ravel())
    return rho, dp


def align(T, plane, max_iters=MAX_ITERS, eps=EPS, dtype=np.float64, trace=None):
    """findTransformECC(T, I, identity, MOTION_EUCLIDEAN, (COUNT | EPS, max_iters, eps)) -> (2x3 warp, iterations, flag, rho, |rho - rho_last|, p).
    Identity and FAILED where OpenCV throws (the reference catches that, botsort.py:104-107).  trace: a list that receives (rho, p) per iteration."""
    p = np.zeros(3)
    rho, last = -1.0, -eps
    i = 0
    while i + 1 <= max_iters and abs(rho - last) >= eps:
        i += 1
        try:
            r, dp = iteration(T, plane, p, dtype)
        except Failed:
            return np.eye(2, 3), i, FAILED, np.nan, np.nan, p
        last, rho = rho, r
        p = np.array([np.arcsin(np.sin(p[0])) + dp[0], p[1] + dp[1], p[2] + dp[2]])
        if trace is not None:
            trace.append((rho, p.copy()))
    flag = CONVERGED if not abs(rho - last) >= eps else EXHAUSTED
    return warp_matrix(p), i, flag, rho, abs(rho - last), p


def warp_matrix(p):
    c, s = np.cos(p[0]), np.sin(p[0])
    return np.array([[c, -s, p[1]], [s, c, p[2]]])


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------------
def plane_truth(theta, tx, ty, H, W, downscale):
    """the planted full-resolution warp (theta, tx, ty) of an (H, W) frame in the coordinates of its downscaled plane: plane pixel u sits at
    X = s u + (s - 1) / 2 with s = W / (W // downscale) (and likewise in y; for odd sizes the two scales differ in the third digit, and the rotation in plane
    coordinates is Euclidean to that accuracy)"""
    sx, sy = (W / (W // downscale), H / (H // downscale)) if downscale > 1 else (1.0, 1.0)
    ox, oy = (sx - 1) / 2.0, (sy - 1) / 2.0
    c, s = np.cos(theta), np.sin(theta)
    return np.array([theta, (tx + (c * ox - s * oy) - ox) / sx, (ty + (s * ox + c * oy) - oy) / sy])
