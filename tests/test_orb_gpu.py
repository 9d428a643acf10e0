"""GPU: the feature-based camera-motion estimate through the C ABI (y7t_orb_extract_u8, y7t_orb_estimate; the intermediate arrays through y7t_orb_tap_layout)
ARRAY-EQUAL, stage by stage, with the NumPy restatement (tests/orb_np.py) on the fixtures of tests/orb_scenes.py, and bit for bit with the host build of the same
kernel bodies (tests/_hostsim/orb.py); then the GMC class inside BoT-SORT and the tracker CLI."""
import ctypes
import os
import types

import numpy as np
import pytest

from tests import orb_np, orb_scenes as sc
from tests.test_orb_cpu import check_estimate, check_extraction, same_bits

pytestmark = pytest.mark.gpu
NAMES = list(sc.FIXTURES)


class Dev:
    def __init__(self):
        import torch
        from yolov7_tracker_amd import _lib
        _lib.require_gpu()
        self.torch, self._lib, self.L = torch, _lib, _lib.load()

    def buffers(self, h, w, cap):
        """workspace and two states, filled with 0xFF: none needs initialisation"""
        t, nb = self.torch, ctypes.c_size_t()
        self._lib.check(self.L.y7t_orb_workspace_bytes(h, w, cap, ctypes.byref(nb)))
        ws = t.full((nb.value + 16,), 255, dtype=t.uint8, device="cuda")
        self._lib.check(self.L.y7t_orb_state_bytes(cap, ctypes.byref(nb)))
        return ws, [t.full((nb.value,), 255, dtype=t.uint8, device="cuda") for _ in range(2)]

    def layout(self, h, w, cap):
        off = (ctypes.c_size_t * 12)()
        self._lib.check(self.L.y7t_orb_tap_layout(h, w, cap, off))
        return [int(v) for v in off]

    def extract(self, frame, ds, dets, cap, ws, state):
        t, _lib = self.torch, self._lib
        f = t.from_numpy(np.ascontiguousarray(frame)).cuda()
        d = t.from_numpy(np.ascontiguousarray(dets, np.float32)).cuda() if dets is not None else None
        H, W = frame.shape[:2]
        rc = self.L.y7t_orb_extract_u8(_lib.ptr(f), H, W, ds, _lib.ptr(d) if d is not None else None, len(dets) if dets is not None else 0, cap, _lib.ptr(ws),
                                       _lib.ptr(state), _lib.stream_ptr())
        t.cuda.synchronize()
        return rc

    def estimate(self, prev, cur, h, w, ds, cap, ws):
        t, _lib = self.torch, self._lib
        out = t.full((12,), float("nan"), dtype=t.float64, device="cuda")
        _lib.check(self.L.y7t_orb_estimate(_lib.ptr(prev), _lib.ptr(cur), h, w, ds, cap, _lib.ptr(ws), _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + 48),
                                           _lib.stream_ptr()))
        out = out.cpu().numpy()
        return out[:6], out[6:]


@pytest.fixture(scope="module")
def dev():
    return Dev()


@pytest.fixture(scope="module")
def hs():
    from tests._hostsim import orb
    orb.lib()
    return orb


def device_run(dev, hs, name):
    """-> (taps of frame 0, taps of frame 1 with the estimate's arrays, warp, status)"""
    (H, W), ds, cap = sc.FIXTURES[name][0], sc.FIXTURES[name][1], sc.FIXTURES[name][5]
    h, w = H // ds, W // ds
    assert dev.layout(h, w, cap) == hs.layout(h, w, cap)
    ws, (a, b) = dev.buffers(h, w, cap)
    f = sc.frames(name)[0]
    assert dev.extract(f[0], ds, sc.dets(name), cap, ws, a) == 0
    ta = hs.read_taps(ws.cpu().numpy(), a.cpu().numpy(), h, w, cap)
    assert dev.extract(f[1], ds, sc.dets(name), cap, ws, b) == 0
    warp, status = dev.estimate(a, b, h, w, ds, cap, ws)
    warp2, status2 = dev.estimate(a, b, h, w, ds, cap, ws)                                   # the same estimate twice: identical bits
    assert same_bits(warp, warp2) and same_bits(status, status2)
    return ta, hs.read_taps(ws.cpu().numpy(), b.cpu().numpy(), h, w, cap), warp, status


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_restatement_stage_by_stage(name, dev, hs):
    ta, tb, warp, status = device_run(dev, hs, name)
    a, b = sc.extracted(name)
    check_extraction(ta, a)
    check_extraction(tb, b)
    check_estimate(tb, warp, status, sc.estimated(name))


def test_more_boxes_than_one_chunk_of_the_mask_pass(dev, hs):
    """300 seeded boxes (the mask pass converts 256 at a time), some reaching outside the frame: kept corners and keypoints equal the restatement's NumPy-sliced mask"""
    (H, W), ds, cap = sc.FIXTURES["wide"][0], 2, 8192
    h, w = H // ds, W // ds
    rng = np.random.default_rng(5)
    tl = np.stack([rng.uniform(-30, W, 300), rng.uniform(-30, H, 300)], 1)
    boxes = np.concatenate([tl, tl + rng.uniform(4, 40, (300, 2)), np.ones((300, 2))], 1).astype(np.float32)
    frame = sc.frames("wide")[0][0]
    want = orb_np.extract(frame, ds, boxes, cap)
    ws, (a, _) = dev.buffers(h, w, cap)
    assert dev.extract(frame, ds, boxes, cap, ws, a) == 0
    got = hs.read_taps(ws.cpu().numpy(), a.cpu().numpy(), h, w, cap)
    assert 20 < len(want["kp"]) < len(sc.extracted("wide")[0]["kp"]) - 20
    check_extraction(got, want)


def test_degenerate_cases_and_refused_arguments(dev, hs):
    (H, W), ds, cap = sc.FIXTURES["ragged"][0], 2, 8192
    h, w = H // ds, W // ds
    ws, (a, b) = dev.buffers(h, w, cap)
    f = sc.frames("ragged")[0]
    assert dev.extract(f[0], ds, None, cap, ws, a) == 0 and dev.extract(np.full((H, W, 3), 100, np.uint8), ds, None, cap, ws, b) == 0
    for prev, cur in ((a, b), (b, a)):                                                       # a flat frame has no corner: no matches, the identity
        warp, status = dev.estimate(prev, cur, h, w, ds, cap, ws)
        assert status[4] == orb_np.NO_MATCHES and warp.tolist() == [1, 0, 0, 0, 1, 0] and status[2] == status[3] == 0
    _, (c, d) = dev.buffers(h, w, 4)                                                         # capacity 4: at most 4 matches, "not enough points"
    assert dev.extract(f[0], ds, None, 4, ws, c) == 0 and dev.extract(f[1], ds, None, 4, ws, d) == 0
    warp, status = dev.estimate(c, d, h, w, ds, 4, ws)
    assert status.tolist()[:2] == [4, 4] and status[4] == orb_np.NOT_ENOUGH and status[5] == 3 and warp.tolist() == [1, 0, 0, 0, 1, 0]
    small = np.zeros((100, 124, 3), np.uint8)                                                # a 62-pixel plane: ORB's border leaves nothing, refused
    assert dev.extract(small, 2, None, cap, ws, a) == -1 and b"orb_dims_ok" in dev.L.y7t_last_error()
    assert dev.extract(f[0], ds, None, 0, ws, a) == -1


def _opts(**kw):
    o = types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="default", img_size=384, iou_thresh=0.5)
    o.__dict__.update(kw)
    return o


def _rows(cur):
    return [(t.track_id, np.asarray(t.tlwh, np.float64).tolist()) for t in cur]


def test_apply_device_equals_the_host_build_and_stays_on_the_device(dev, hs):
    from yolov7_tracker_amd.tracker.gmc import GMC
    torch = dev.torch
    frames, planted, dets = sc.sequence(4)
    on_dev, on_host, through_apply = GMC('features'), GMC('features', backend=hs.HostFeatures()), GMC('features')
    for t in range(4):
        got = on_dev.apply_device(torch.from_numpy(frames[t]).cuda(), torch.from_numpy(dets[t]).cuda())      # a device frame and device detections
        want = on_host.apply(frames[t], dets[t])
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and got.shape == (6,)
        assert same_bits(got.cpu().numpy(), want.ravel()) and same_bits(through_apply.apply(frames[t], dets[t]).ravel(), want.ravel())
        if t == 0:
            assert want.tolist() == np.eye(2, 3).tolist() and on_dev.last_status is None
        else:
            assert on_dev.last_status.is_cuda and np.array_equal(on_dev.last_status.cpu().numpy(), on_host.last_status) and on_host.last_status[4] == orb_np.OK


def test_botsort_with_the_estimator_equals_botsort_fed_the_host_builds_warps(dev, hs):
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.botsort import BoTSORT
    from yolov7_tracker_amd.tracker.gmc import GMC
    torch = dev.torch
    frames, planted, dets = sc.sequence(4)
    g = GMC('features', backend=hs.HostFeatures())
    warps = [g.apply(f, d) for f, d in zip(frames, dets)]
    assert max(np.abs(w - np.eye(2, 3)).max() for w in warps[1:]) > 0.1                     # the camera does move

    def botsort():
        BaseTrack._count = 0
        return BoTSORT(_opts(kalman_format="botsort"), frame_rate=30)

    a = botsort()
    a.gmc = GMC('features').apply_device
    got = [_rows(a.update(d, torch.from_numpy(f).cuda())) for d, f in zip(dets, frames)]
    b = botsort()
    want = [_rows(b.update(d, f, warp=w)) for d, f, w in zip(dets, frames, warps)]
    assert got == want and sum(len(r) for r in got) > 10


def test_cli_with_the_estimator(tmp_path):
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    common = ["--dataset", "synthetic", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "256", "--synthetic_dets", "--synthetic_frames", "4",
              "--synthetic_objs", "20", "--results_root", str(tmp_path), "--gmc", "features"]
    folder = track.cli(common + ["--tracker", "botsort"])
    lines = open(os.path.join(folder, "synthetic-000.txt")).read().splitlines()
    assert len(lines) > 10 and all(len(l.split(",")) == 10 for l in lines)
    with pytest.raises(ValueError, match="gmc"):
        track.cli(common + ["--tracker", "bytetrack"])
