"""GPU: the camera-motion estimate through the C ABI (y7t_ecc_prepare_u8, y7t_ecc_align, y7t_ecc_iteration_sums_f64) against the NumPy float64 restatement
(tests/ecc_np.py, the tolerances of tests/ecc_scenes.py) and, bit for bit, against the host build of the same kernel bodies (tests/_hostsim/ecc.py), which mirrors
the device's reduction order; then the GMC class inside StrongSORT, BoT-SORT and the tracker CLI."""
import ctypes
import os
import types

import numpy as np
import pytest

from tests import ecc_np, ecc_scenes as sc

pytestmark = pytest.mark.gpu
NAMES = list(sc.FIXTURES)


class Dev:
    def __init__(self):
        import torch
        from yolov7_tracker_amd import _lib
        _lib.require_gpu()
        self.torch, self._lib, self.L = torch, _lib, _lib.load()

    def prepare(self, frame, ds):
        t, _lib = self.torch, self._lib
        f = t.from_numpy(np.ascontiguousarray(frame)).cuda()
        H, W = frame.shape[:2]
        plane = t.full((H // ds, W // ds, 4), float("nan"), dtype=t.float32, device="cuda")
        _lib.check(self.L.y7t_ecc_prepare_u8(_lib.ptr(f), H, W, ds, _lib.ptr(plane), _lib.stream_ptr()))
        t.cuda.synchronize()
        return plane

    def workspace(self, h, w):
        nb = ctypes.c_size_t()
        self._lib.check(self.L.y7t_ecc_workspace_bytes(h, w, ctypes.byref(nb)))
        return self.torch.full((nb.value // 8 + 1,), float("nan"), dtype=self.torch.float64, device="cuda")      # (needs no initialisation)

    def sums(self, tmpl, img, p):
        t, _lib = self.torch, self._lib
        h, w = img.shape[:2]
        ws, out = self.workspace(h, w), t.zeros(21, dtype=t.float64, device="cuda")
        _lib.check(self.L.y7t_ecc_iteration_sums_f64(_lib.ptr(tmpl), _lib.ptr(img), h, w, p[0], p[1], p[2], _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr()))
        return out.cpu().numpy()

    def align(self, tmpl, img, max_iters=ecc_np.MAX_ITERS, eps=ecc_np.EPS, motion=1):
        t, _lib = self.torch, self._lib
        h, w = img.shape[:2]
        ws, warp, status = self.workspace(h, w), t.zeros(6, dtype=t.float64, device="cuda"), t.zeros(4, dtype=t.float64, device="cuda")
        rc = self.L.y7t_ecc_align(_lib.ptr(tmpl), _lib.ptr(img), h, w, motion, max_iters, eps, _lib.ptr(ws), _lib.ptr(warp), _lib.ptr(status), _lib.stream_ptr())
        if rc:
            return rc, None
        return warp.cpu().numpy(), status.cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    return Dev()


@pytest.fixture(scope="module")
def hs():
    from tests._hostsim import ecc
    ecc.lib()
    return ecc


@pytest.fixture(scope="module")
def dev_planes(dev):
    return {n: tuple(dev.prepare(f, sc.FIXTURES[n][2]) for f in sc.frames(n)) for n in NAMES}


@pytest.fixture(scope="module")
def host_planes(hs):
    return {n: tuple(hs.prepare(f, sc.FIXTURES[n][2]) for f in sc.frames(n)) for n in NAMES}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_prepared_plane_is_exact(name, dev_planes, host_planes):
    for got, want, host in zip(dev_planes[name], sc.planes(name), host_planes[name]):
        got = got.cpu().numpy()
        assert got.shape == want.shape[:2] + (4,)
        assert np.array_equal(got[..., 0], want[..., 0]) and np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 2], want[..., 2])
        assert np.array_equal(got, host)                                                     # (the padding lane too: no NaN of the fill survives)


@pytest.mark.parametrize("name", NAMES)
def test_sums_of_one_iteration(name, dev, hs, dev_planes, host_planes):
    got, want = dev.sums(*dev_planes[name], sc.P_SUMS), sc.ref_sums(name)
    print(name, "largest relative difference of the 21 sums: %.3g (allowed %.3g)" % (sc.rel(got, want).max(), sc.TOL_SUMS_REL))
    assert got[0] == want[0] and (sc.rel(got, want) <= sc.TOL_SUMS_REL).all(), sc.rel(got, want)
    assert same_bits(got, hs.sums(*host_planes[name], sc.P_SUMS))                           # the host build mirrors the reduction order


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", NAMES)
def test_warp_after_k_fixed_iterations(name, k, dev, hs, dev_planes, host_planes):
    warp, status = dev.align(*dev_planes[name], k, -1.0)
    _, it, flag, rho, _, p = sc.ref_align(name, k)
    assert status[0] == it == k and status[1] == flag == ecc_np.EXHAUSTED
    d = np.abs(sc.params_of(warp) - p)
    print(name, k, "parameters differ by %.3g (allowed %.3g), rho by %.3g" % (d.max(), sc.TOL_P, abs(status[2] - rho)))
    assert (d <= sc.TOL_P).all() and abs(status[2] - rho) <= sc.TOL_RHO
    hw, hst = hs.align(*host_planes[name], k, -1.0)
    assert same_bits(warp, hw) and same_bits(status, hst)


@pytest.mark.parametrize("name", NAMES)
def test_termination_and_reproducibility(name, dev, hs, dev_planes, host_planes):
    warp, status = dev.align(*dev_planes[name])
    assert status[1] == ecc_np.CONVERGED and status[3] < ecc_np.EPS
    sc.check_iterations(name, status[0], status[2], sc.params_of(warp))
    hw, hst = hs.align(*host_planes[name])
    assert same_bits(warp, hw) and same_bits(status, hst)
    warp2, status2 = dev.align(*dev_planes[name])                                           # the same estimate twice: identical bits
    assert same_bits(warp, warp2) and same_bits(status, status2)


def test_failure_paths_and_refused_arguments(dev, hs):
    c = np.full((48, 64, 3), 100, np.uint8)
    pc = dev.prepare(c, 2)
    warp, status = dev.align(pc, pc)
    assert status[1] == ecc_np.FAILED and status[0] == 1 and not np.isfinite(status[2]) and warp.tolist() == [1, 0, 0, 0, 1, 0]
    for seed in sc.NOISE_SEEDS:
        rng = np.random.default_rng(seed)
        a, b = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
        want = ecc_np.align(ecc_np.prepare(a)[..., 0], ecc_np.prepare(b))
        warp, status = dev.align(dev.prepare(a, 2), dev.prepare(b, 2))
        assert want[2] in (ecc_np.FAILED, ecc_np.EXHAUSTED) and status[1] == want[2] and status[0] == want[1], seed
        hw, hst = hs.align(hs.prepare(a), hs.prepare(b))
        assert same_bits(warp, hw) and np.array_equal(status[:2], hst[:2])
        if want[2] == ecc_np.FAILED:
            assert warp.tolist() == [1, 0, 0, 0, 1, 0]
    for motion in (0, 2, 3):                                                                # translation, affine, homography: not in scope
        assert dev.align(pc, pc, motion=motion)[0] == -1                                    # Y7T_E_ARG
    assert b"motion" in dev.L.y7t_last_error()


def _camera_sequence():
    from yolov7_tracker_amd import synth
    frames, planted = synth.make_camera_frames(8, (192, 256), 4)
    dets = synth.make_detections(8, 20, 192, seq_idx=4)
    return frames, planted, dets


def _opts(**kw):
    o = types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="default", img_size=256, iou_thresh=0.5)
    o.__dict__.update(kw)
    return o


def _rows(cur):
    return [(t.track_id, np.asarray(t.tlwh, np.float64).tolist()) for t in cur]


def test_apply_device_equals_apply_and_stays_on_the_device(dev):
    from yolov7_tracker_amd.tracker.gmc import GMC
    torch = dev.torch
    frames, planted, _ = _camera_sequence()
    for faithful in (True, False):
        a, b = GMC('ecc', faithful=faithful), GMC('ecc', faithful=faithful)
        for t in range(4):
            on_host = a.apply(frames[t])
            on_dev = b.apply_device(torch.from_numpy(frames[t]).cuda())                     # a device frame; apply took the NumPy one
            assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.dtype == torch.float64 and on_dev.shape == (6,)
            assert on_host.shape == (2, 3) and same_bits(on_host.ravel(), on_dev.cpu().numpy())
            if t == 0:
                assert on_host.tolist() == np.eye(2, 3).tolist()
        assert b.last_status is not None and b.last_status.is_cuda and int(b.last_status[1]) == ecc_np.CONVERGED
    assert same_bits(GMC('none').apply_device(frames[0]).cpu().numpy(), np.eye(2, 3).ravel())


def test_estimated_warps_against_the_planted_ones(dev):
    """no further from the truth than the restatement's own error plus the measured noise (translations are scaled by the downscale of 2, and so is their noise; where the
    iteration counts differ by the one iteration the termination rule allows, the restatement's last step is added)"""
    from yolov7_tracker_amd.tracker.gmc import GMC
    frames, planted, _ = _camera_sequence()
    g = GMC('ecc', faithful=False)
    g.apply(frames[0])
    for t in range(1, 5):
        est = sc.params_of(g.apply(frames[t]))
        iters = int(g.last_status[0])
        trace = []
        ref = ecc_np.align(ecc_np.prepare(frames[t - 1])[..., 0], ecc_np.prepare(frames[t]), trace=trace)
        assert abs(iters - ref[1]) <= 1
        step = np.abs(trace[-1][1] - trace[-2][1]) if iters != ref[1] else np.zeros(3)
        scale = np.array([1.0, 2.0, 2.0])
        truth = sc.params_of(planted[t])
        print(t, "device - truth", est - truth, "restatement - truth", ref[5] * scale - truth)
        assert (np.abs(est - truth) <= np.abs(ref[5] * scale - truth) + scale * (sc.TOL_P + step)).all()


def test_trackers_with_the_estimator_equal_trackers_fed_its_warps(dev):
    """the plumbing adds nothing: StrongSORT with ECC = GMC('ecc', faithful=False) and BoT-SORT with gmc = apply_device give the ids and boxes of the same trackers fed
    the estimator's matrices as explicit warp= inputs"""
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.botsort import BoTSORT
    from yolov7_tracker_amd.tracker.gmc import GMC
    from yolov7_tracker_amd.tracker.strongsort import StrongSORT
    torch = dev.torch
    frames, planted, dets = _camera_sequence()
    g = GMC('ecc', faithful=False)
    warps = [g.apply(f) for f in frames]
    assert max(np.abs(w - np.eye(2, 3)).max() for w in warps[1:]) > 0.1                     # the camera does move

    def strongsort():
        BaseTrack._count = 0
        t = StrongSORT(_opts(kalman_format="strongsort"), frame_rate=30, gamma=0.1)
        t.get_feature = lambda tlbrs, ori_img: synth.make_features(tlbrs)
        return t

    def botsort():
        BaseTrack._count = 0
        return BoTSORT(_opts(kalman_format="botsort"), frame_rate=30)

    a = strongsort()
    a.ECC = GMC('ecc', faithful=False)
    got = [_rows(a.update(d, f)) for d, f in zip(dets, frames)]
    b = strongsort()
    want = [_rows(b.update(d, f, warp=w)) for d, f, w in zip(dets, frames, warps)]
    assert got == want and sum(len(r) for r in got) > 40
    a = botsort()
    a.gmc = GMC('ecc', faithful=False).apply_device
    got = [_rows(a.update(d, torch.from_numpy(f).cuda())) for d, f in zip(dets, frames)]
    b = botsort()
    want = [_rows(b.update(d, f, warp=w)) for d, f, w in zip(dets, frames, warps)]
    assert got == want and sum(len(r) for r in got) > 40
    c = botsort()                                                                           # ... and the warps matter: without them the boxes differ
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        still = [_rows(c.update(d, f)) for d, f in zip(dets, frames)]
    assert still != want


def test_cli_with_the_estimator(tmp_path):
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    common = ["--dataset", "synthetic", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "256", "--synthetic_dets", "--synthetic_frames", "4",
              "--synthetic_objs", "20", "--results_root", str(tmp_path), "--gmc", "ecc"]
    folder = track.cli(common + ["--tracker", "strongsort", "--reid_model_path", "random:osnet"])
    lines = open(os.path.join(folder, "synthetic-000.txt")).read().splitlines()
    assert len(lines) > 10 and all(len(l.split(",")) == 10 for l in lines)
    with pytest.raises(ValueError, match="gmc"):
        track.cli(common + ["--tracker", "bytetrack"])
