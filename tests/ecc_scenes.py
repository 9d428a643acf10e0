"""tests/ecc_scenes.py -- TEST INFRASTRUCTURE ONLY: the fixture scenes, the restatement's results on them (computed once, shared) and the tolerance constants
of the camera-motion tests (tests/test_ecc_cpu.py, tests/test_ecc_gpu.py)."""
import functools

import numpy as np

from tests import ecc_np
from yolov7_tracker_amd import synth

# name -> (H, W, downscale, theta, tx, ty): the smallest shapes at which each mechanism can break.  The planted motion is in full-resolution pixels.
FIXTURES = {
    "odd": (95, 123, 2, 0.01, 1.7, -2.3),        # 61 x 47 plane: the general resize formula, one ragged workgroup pair, ragged lanes
    "even": (96, 128, 2, 0.01, 1.7, -2.3),       # 64 x 48 plane: exactly the 2 x 2 mean
    "multi": (273, 401, 2, 0.01, 1.7, -2.3),     # 200 x 136 plane: 14 workgroups, the last slab ragged
    "full": (48, 64, 1, 0.01, 1.7, -2.3),        # downscale 1: blur and resize skipped
    "corner": (273, 401, 2, 0.05, 1.7, -2.3),    # the mask cuts the corners, the border-0 taps matter
}
SEED = 3
P_SUMS = (0.004, 0.6, -0.8)                      # the parameters of the single-iteration comparison (at the identity every sample is exact)
KS = (1, 5, 20)                                  # fixed iteration counts (eps < 0)

# The tolerance.  The device (and its host build) differ from the float64 restatement in ONE respect: the per-pixel stage -- warp coordinates, bilinear weights,
# samples, Jacobian row -- is float32.  That noise is MEASURED ON THE RESTATEMENT ITSELF: ecc_np with dtype=float32 against dtype=float64 (sums float64 in both)
# over the five fixtures, at P_SUMS for the sums and at k = 1, 5, 20 fixed iterations for the parameters and rho
# (test_ecc_cpu.py::test_noise_constants_are_the_restatements_own re-measures them):
NOISE_SUMS_REL = 1.6e-4      # largest |s32 - s64| / |s64| over the 21 sums        (measured 1.58e-4: sum J2*T of "multi", a sum that nearly cancels)
NOISE_P = 6.0e-6             # largest |p32 - p64| over (theta, tx, ty) and k       (measured 6.00e-6: "corner", k = 20)
NOISE_RHO = 3.7e-7           # largest |rho32 - rho64| over k                       (measured 3.66e-7: "odd", k = 5)
# allowed: 4 x the noise -- summation order and fused multiply-add contraction differ between NumPy and the device, and neither is under the test's control
TOL_SUMS_REL, TOL_P, TOL_RHO = 4 * NOISE_SUMS_REL, 4 * NOISE_P, 4 * NOISE_RHO

# pairs of unrelated 128 x 96 uint8 noise frames (rng seed): the restatement fails on the first three (lambda_d <= 0 after 3, 6 and 4 iterations) and runs out of its
# 100 iterations on the last.  Chosen on the CPU among seeds 500 - 523: 22 of those fail within 6 iterations, 515 exhausts, and on one (500) the iteration wanders
# chaotically -- float64 happens to stop at 53, the same program with float32 pixels at 100 -- so its outcome is no property of either program and it is not used.
NOISE_SEEDS = (505, 510, 522, 515)


@functools.lru_cache(maxsize=None)
def frames(name):
    """-> (template frame, image frame) uint8 BGR: the analytic scene and its copy under the planted warp (image(W X) shows what template(X) shows)"""
    H, W, ds, th, tx, ty = FIXTURES[name]
    f0 = synth.render_camera_frame((H, W), synth.euclidean_warp(0.0, 0.0, 0.0), SEED)
    inv = np.linalg.inv(np.vstack([synth.euclidean_warp(th, tx, ty), [0.0, 0.0, 1.0]]))[:2]
    return f0, synth.render_camera_frame((H, W), inv, SEED)


@functools.lru_cache(maxsize=None)
def planes(name):
    """the restatement's planes (h, w, 3) float64 of the two frames"""
    f0, f1 = frames(name)
    ds = FIXTURES[name][2]
    return ecc_np.prepare(f0, ds), ecc_np.prepare(f1, ds)


def truth(name):
    H, W, ds, th, tx, ty = FIXTURES[name]
    return ecc_np.plane_truth(th, tx, ty, H, W, ds)


@functools.lru_cache(maxsize=None)
def ref_sums(name, dtype=np.float64):
    P0, P1 = planes(name)
    return ecc_np.raw_sums(P0[..., 0], P1, P_SUMS, dtype)


@functools.lru_cache(maxsize=None)
def ref_align(name, k=None, dtype=np.float64):
    """k None: the reference's criteria (100 iterations, eps 1e-5); else k fixed iterations -> (warp, iterations, flag, rho, |rho - rho_last|, p)"""
    P0, P1 = planes(name)
    return ecc_np.align(P0[..., 0], P1, dtype=dtype) if k is None else ecc_np.align(P0[..., 0], P1, k, -1.0, dtype)


def params_of(warp6):
    """(theta, tx, ty) of a row-major Euclidean 2x3"""
    w = np.asarray(warp6, np.float64).reshape(6)
    return np.array([np.arctan2(w[3], w[0]), w[2], w[5]])


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))


def check_iterations(name, iters, rho, p):
    """the termination rule of the tests: the count equals the restatement's, or differs by one when the restatement's |rho - rho_last| at its stopping iteration (or the
    one before) lies within the measured noise of eps -- each difference carries the noise of two rhos.  The final rho and parameters agree within the noise; where the
    counts differ by that one iteration, rho may also differ by eps and the parameters by the restatement's own last step."""
    trace = []
    P0, P1 = planes(name)
    _, it, flag, r, d, pr = ecc_np.align(P0[..., 0], P1, trace=trace)
    rhos = [-1.0] + [t[0] for t in trace]
    near = [abs(abs(rhos[i] - rhos[i - 1]) - ecc_np.EPS) <= 2 * TOL_RHO for i in (it - 1, it) if i >= 1]
    if any(near):
        assert abs(int(iters) - it) <= 1, (name, iters, it)
    else:
        assert int(iters) == it, (name, iters, it, d)
    off = int(iters) != it
    last_step = np.abs(trace[-1][1] - trace[-2][1]).max() if len(trace) > 1 else 0.0
    assert abs(rho - r) <= TOL_RHO + (ecc_np.EPS if off else 0.0), (name, rho, r)
    assert (np.abs(np.asarray(p) - pr) <= TOL_P + (last_step if off else 0.0)).all(), (name, p, pr)
    return it
