"""CPU: the camera-motion estimate (ECC, tracker/gmc.py) without a GPU -- the NumPy float64 restatement (tests/ecc_np.py) against closed forms and planted warps,
and the host build of the kernel bodies (tests/_hostsim/ecc.py: csrc/y7t_ecc.h compiled with g++) against the restatement.  The tolerances are the float32 noise
measured on the restatement itself (tests/ecc_scenes.py)."""
import numpy as np
import pytest

from tests import ecc_np, ecc_scenes as sc

NAMES = list(sc.FIXTURES)


@pytest.fixture(scope="module")
def hs():
    from tests._hostsim import ecc
    ecc.lib()
    return ecc


@pytest.fixture(scope="module")
def host_planes(hs):
    return {n: (hs.prepare(sc.frames(n)[0], sc.FIXTURES[n][2]), hs.prepare(sc.frames(n)[1], sc.FIXTURES[n][2])) for n in NAMES}


# ---- the restatement itself --------------------------------------------------------------------------------------------------------------------------
def test_restatement_stages_have_their_closed_forms():
    # gray: 0.114 B + 0.587 G + 0.299 R rounded half up
    px = np.array([[[10, 20, 30], [5, 0, 0], [0, 0, 255], [255, 255, 255], [0, 1, 0], [50, 100, 13]]], np.uint8)
    assert ecc_np.gray(px).tolist() == [[22, 1, 76, 255, 1, 68]]      # 21.85, 0.57, 76.245, 255, 0.587, 68.287
    a, b = ecc_np.gauss_taps()
    assert abs(a - 0.3078013291) < 1e-9 and abs(2 * a + b - 1) < 1e-15
    # blur of an impulse of 200 on 8 x 6: the outer product of the taps, rounded half up (29.55, 23.66, 18.95)
    imp = np.zeros((6, 8), np.int64)
    imp[3, 3] = 200
    assert ecc_np.blur(imp)[2:5, 2:5].tolist() == [[19, 24, 19], [24, 30, 24], [19, 24, 19]] and ecc_np.blur(imp).sum() == 4 * 19 + 4 * 24 + 30
    # blur of the ramp 10 x: unchanged inside (symmetric taps that sum to 1), reflect-101 at the ends: a (10 + 10) = 6.16 and 70 - 6.16
    ramp = np.tile(10 * np.arange(8), (6, 1))
    assert ecc_np.blur(ramp).tolist() == [[6, 10, 20, 30, 40, 50, 60, 64]] * 6
    # resize 8 x 6 -> 4 x 3 is the 2 x 2 mean (20 u + 5); 7 -> 3 follows the general formula: sources 2/3, 3, 16/3 -> 6.67, 30, 53.33
    assert ecc_np.resize(ramp.astype(np.float64), 3, 4).tolist() == [[5, 25, 45, 65]] * 3
    assert ecc_np.resize(ramp[:, :7].astype(np.float64), 3, 3).tolist() == [[7, 30, 53]] * 3
    ties = np.array([[1, 2], [2, 1]], np.float64)                     # mean 1.5: rounded half up
    assert ecc_np.resize(ties, 1, 1).tolist() == [[2]]
    # gradients of the ramp: 10 inside, 0 at the reflected ends, gy = 0
    gx, gy = ecc_np.gradients(ramp.astype(np.float64))
    assert gx.tolist() == [[0, 10, 10, 10, 10, 10, 10, 0]] * 6 and not gy.any()
    gx, gy = ecc_np.gradients(imp.astype(np.float64))
    assert gx[3, 2] == 100 and gx[3, 4] == -100 and gy[2, 3] == 100 and gy[4, 3] == -100 and gx[3, 3] == 0


@pytest.mark.parametrize("name", NAMES)
def test_restatement_recovers_the_planted_warp(name):
    """its own error to the truth (recorded in DESIGN.md section 4): every corner of the plane lands within half a plane pixel of where the planted warp puts it -- the
    boxes the warp is applied to are rounded to whole pixels (track.py:234-244).  The error is the method's (central-difference gradients of an 8-bit image, no pyramid)."""
    _, it, flag, rho, _, p = sc.ref_align(name)
    t = sc.truth(name)
    print("%s: %d iterations, rho %.6f, p - truth = %s" % (name, it, rho, p - t))
    assert flag == ecc_np.CONVERGED and it < ecc_np.MAX_ITERS
    h, w = sc.planes(name)[0].shape[:2]
    for cx, cy in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        d = (ecc_np.warp_matrix(p) - ecc_np.warp_matrix(t)) @ np.array([cx, cy, 1.0])
        assert np.hypot(*d) < 0.5, (name, cx, cy, d)


def test_noise_constants_are_the_restatements_own():
    """NOISE_* of tests/ecc_scenes.py: float32 against float64 per-pixel stage of the RESTATEMENT, never of the code under test"""
    s = max(sc.rel(sc.ref_sums(n, np.float32), sc.ref_sums(n)).max() for n in NAMES)
    p = max(np.abs(sc.ref_align(n, k, np.float32)[5] - sc.ref_align(n, k)[5]).max() for n in NAMES for k in sc.KS)
    r = max(abs(sc.ref_align(n, k, np.float32)[3] - sc.ref_align(n, k)[3]) for n in NAMES for k in sc.KS)
    print("measured noise: sums %.3g (rel), parameters %.3g, rho %.3g" % (s, p, r))
    assert 0.5 * sc.NOISE_SUMS_REL < s <= sc.NOISE_SUMS_REL and 0.5 * sc.NOISE_P < p <= sc.NOISE_P and 0.5 * sc.NOISE_RHO < r <= sc.NOISE_RHO


# ---- the host build of the kernel bodies against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_prepared_plane_is_exact(name, host_planes):
    for got, want in zip(host_planes[name], sc.planes(name)):
        assert got.shape == want.shape[:2] + (4,) and got.dtype == np.float32
        assert np.array_equal(got[..., 0], want[..., 0])                                   # integers
        assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 2], want[..., 2])      # half-integers
        assert not got[..., 3].any()


def test_host_prepare_on_the_ramp_and_the_impulse(hs):
    ramp = np.repeat(np.tile(10 * np.arange(8), (6, 1))[..., None], 3, axis=2).astype(np.uint8)
    imp = np.zeros((6, 8, 3), np.uint8)
    imp[3, 3] = 200
    for img in (ramp, imp):
        for ds in (1, 2):
            assert np.array_equal(hs.prepare(img, ds)[..., :3], ecc_np.prepare(img, ds))


@pytest.mark.parametrize("name", NAMES)
def test_host_sums_of_one_iteration(name, hs, host_planes):
    got, want = hs.sums(*host_planes[name], sc.P_SUMS), sc.ref_sums(name)
    print(name, "largest relative difference of the 21 sums: %.3g (allowed %.3g)" % (sc.rel(got, want).max(), sc.TOL_SUMS_REL))
    assert got[0] == want[0]                                                                # the mask count
    assert (sc.rel(got, want) <= sc.TOL_SUMS_REL).all(), sc.rel(got, want)


def test_the_sums_exercise_the_slab_combine(hs):
    h, w = sc.planes("multi")[0].shape[:2]
    assert hs.num_wg(h, w) == 14 and (h * w) % 2048 and hs.num_wg(47, 61) == 2 and hs.num_wg(540, 960) == 254 and hs.num_wg(4000, 4000) == 256


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", NAMES)
def test_host_warp_after_k_fixed_iterations(name, k, hs, host_planes):
    warp, status = hs.align(*host_planes[name], k, -1.0)
    _, it, flag, rho, _, p = sc.ref_align(name, k)
    assert status[0] == it == k and status[1] == flag == ecc_np.EXHAUSTED                   # running out of iterations is not a failure
    d = np.abs(sc.params_of(warp) - p)
    print(name, k, "parameters differ by %.3g (allowed %.3g), rho by %.3g" % (d.max(), sc.TOL_P, abs(status[2] - rho)))
    assert (d <= sc.TOL_P).all() and abs(status[2] - rho) <= sc.TOL_RHO
    assert warp[0] == warp[4] and warp[1] == -warp[3] and abs(warp[0] ** 2 + warp[3] ** 2 - 1) < 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_host_termination_matches(name, hs, host_planes):
    warp, status = hs.align(*host_planes[name], ecc_np.MAX_ITERS, ecc_np.EPS)
    assert status[1] == ecc_np.CONVERGED and status[3] < ecc_np.EPS
    sc.check_iterations(name, status[0], status[2], sc.params_of(warp))


# ---- failure paths -----------------------------------------------------------------------------------------------------------------------------------------
def test_constant_image_fails_with_the_identity(hs):
    c = np.full((48, 64, 3), 100, np.uint8)
    assert ecc_np.align(ecc_np.prepare(c)[..., 0], ecc_np.prepare(c))[2] == ecc_np.FAILED
    warp, status = hs.align(hs.prepare(c), hs.prepare(c))
    assert status[1] == ecc_np.FAILED and status[0] == 1 and not np.isfinite(status[2])
    assert warp.tolist() == [1, 0, 0, 0, 1, 0]


@pytest.mark.parametrize("seed", sc.NOISE_SEEDS)
def test_unrelated_noise_images_end_as_the_restatement_decides(seed, hs):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    want = ecc_np.align(ecc_np.prepare(a)[..., 0], ecc_np.prepare(b))
    warp, status = hs.align(hs.prepare(a), hs.prepare(b))
    assert want[2] in (ecc_np.FAILED, ecc_np.EXHAUSTED) and status[1] == want[2] and status[0] == want[1]
    if want[2] == ecc_np.FAILED:
        assert warp.tolist() == [1, 0, 0, 0, 1, 0]


def test_singular_hessian_gives_no_step(hs):
    S = sc.ref_sums("even").copy()
    S[6:] = 0.0                                   # no gradient anywhere: J = 0, the Hessian is singular and inverts to zeros (cv::Mat::inv)
    assert not ecc_np.inv3(np.zeros((3, 3))).any()
    p, rho, flag = hs.solve(S, p=(0.01, 0.5, -0.25))
    assert p.tolist() == [0.01, 0.5, -0.25] and flag == 0 and 0 < rho < 1
    S2 = sc.ref_sums("even").copy()
    S2[15:] = [4.0, 2.0, 0.0, 1.0, 0.0, 0.0]      # rank 1
    p, rho, flag = hs.solve(S2, p=(0.0, 0.0, 0.0))
    assert p.tolist() == [0.0, 0.0, 0.0] and flag == 0


def test_own_sine_cosine_and_principal_angle(hs):
    for th in (0.0, 1e-9, 0.01, -0.05, 0.7, 0.79, 1.5, -2.0, 3.0, 3.2, -6.0, 10.0):
        s, c = hs.sincos(th)
        assert abs(s - np.sin(th)) < 4e-16 and abs(c - np.cos(th)) < 4e-16, th
        assert abs(hs.lib().hs_ecc_principal(th) - np.arcsin(np.sin(th))) < 2e-15, th
    assert hs.sincos(0.0) == (0.0, 1.0) and hs.lib().hs_ecc_principal(0.3) == 0.3


# ---- the GMC surface, through the host build ----------------------------------------------------------------------------------------------------------------
def test_gmc_surface(hs, capsys):
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker.gmc import GMC
    frames, planted = synth.make_camera_frames(3, (96, 128), 1)
    assert planted[0].tolist() == np.eye(2, 3).tolist()
    pl = [hs.prepare(f, 2) for f in frames]
    faithful, upstream = GMC('ecc', backend=hs.HostEcc()), GMC('ecc', faithful=False, backend=hs.HostEcc())
    for g in (faithful, upstream):
        first = g.apply(frames[0])
        assert first.shape == (2, 3) and first.dtype == np.float64 and first.tolist() == np.eye(2, 3).tolist()
    for t in (1, 2):
        a, b = faithful.apply(frames[t], None), upstream.apply(frames[t])
        assert np.array_equal(a.ravel(), hs.align(pl[0], pl[t])[0])                          # frame 0 stays the template, the translation is in plane pixels
        want = hs.align(pl[t - 1], pl[t])[0] * [1, 1, 2, 1, 1, 2]                            # previous-frame template, full-resolution translation
        assert np.array_equal(b.ravel(), want)
        assert np.abs(b - planted[t])[:, 2].max() < 0.5 and np.abs(b - planted[t])[:, :2].max() < 5e-3
    assert faithful.prevFrame is not None and np.array_equal(faithful.prevFrame, pl[0]) and np.array_equal(upstream.prevFrame, pl[2])
    assert np.array_equal(GMC('ecc', downscale=1, backend=hs.HostEcc()).apply(frames[0]), np.eye(2, 3))
    assert np.array_equal(GMC('none').apply(frames[0]), np.eye(2, 3))
    for m in ('orb', 'sift', 'file'):
        with pytest.raises(NotImplementedError, match="scope"):
            GMC(m)
    with pytest.raises(ValueError):
        GMC('homography')
    capsys.readouterr()
    g = GMC('ecc', backend=hs.HostEcc())
    flat = np.full((48, 64, 3), 90, np.uint8)
    g.apply(flat)
    assert g.apply(flat).tolist() == np.eye(2, 3).tolist()
    assert 'Warning: find transform failed. Set warp as identity' in capsys.readouterr().out      # botsort.py:107


def test_camera_frames_are_the_scene_under_the_planted_warps():
    from yolov7_tracker_amd import synth
    frames, warps = synth.make_camera_frames(3, (40, 56), 2)
    assert frames.shape == (3, 40, 56, 3) and frames.dtype == np.uint8 and warps.shape == (3, 2, 3)
    f2, w2 = synth.make_camera_frames(3, (40, 56), 2)
    assert np.array_equal(frames, f2) and np.array_equal(warps, w2) and not np.array_equal(frames, synth.make_camera_frames(3, (40, 56), 3)[0])
    # frame_t is the analytic scene at pose_t = pose_{t-1} W_t^-1, evaluated (never interpolated): frame_t at W_t X shows what frame_{t-1} shows at X
    pose = np.eye(3)
    for t in range(3):
        pose = pose @ np.linalg.inv(np.vstack([warps[t], [0.0, 0.0, 1.0]]))
        assert np.array_equal(frames[t], synth.render_camera_frame((40, 56), pose[:2], 2))
        assert abs(np.linalg.det(warps[t][:, :2]) - 1) < 1e-12 and abs(warps[t][0, 1] + warps[t][1, 0]) < 1e-15       # Euclidean
    lv = synth.camera_background(np.array([3.25, 17.5]), np.array([8.125, 2.0]), 2)
    assert lv.shape == (2, 3) and np.abs(lv - 128).max() <= 90                                    # never clipped
    assert frames[0].std() > 8 and len(np.unique(frames[0])) > 30                                 # textured
