"""DeepMOT on the MI355X: the Deep Hungarian Net's kernels (csrc/y7t_dhn.hip) through y7t_dhn_forward_f32 against the reference network's recorded outputs
(tests/golden/dhn_*.npz: within 4 E of the float64 evaluation, E the reference's own float32-versus-float64 gap), and the frame step (front program, network, back
program) through the C ABI and the Python class against the reference's golden vectors (tests/golden/tracker_deepmot_*.npz) and the CPU build of the same programs;
the refusals, the overflows, a shared network object and the tracker CLI with --tracker deepmot.

The give-up path of the recurrence's bounded waits is NOT exercised here: nothing may stall a card on purpose.  The CPU tests hand the back program a failed
status word (tests/test_deepmot_cpu.py)."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import util  # noqa: E402
from tests import tracker_case as tc  # noqa: E402
from tests._hostsim import deepmot as hdm  # noqa: E402
from tests.tracker_case import DHN_NAMES, GOLDEN  # noqa: E402
from yolov7_tracker_amd.tracker.deepmot import DeepMOT  # noqa: E402

NAMES = tc.NAMES["deepmot"]
load_golden = functools.partial(tc.load_golden, "deepmot")

_DHN = {}


def device_dhn(seed, scale):
    """one network object per weight set for the whole module (64 x 48 is the largest matrix any test runs)"""
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker.deepmot import DeviceDHN
    key = (int(seed), float(scale))
    if key not in _DHN:
        _DHN[key] = DeviceDHN(synth.make_dhn_weights(*key), 64, 48)
    return _DHN[key]


def new_tracker(g, threads=0, max_tracks=256, max_dets=256, **kw):
    return tc.new_tracker(DeepMOT, g["conf"], threads, g["kalman_format"], ctor=dict(dhn=device_dhn(g["seed"], g["scale"])), max_tracks=max_tracks, max_dets=max_dets, **kw)


def step(t, g, f):
    d = g["dets"][f]
    img = types.SimpleNamespace(shape=g["img_shape"] + (3,))      # (the frame supplies its shape only)
    return t.update_without_detection(None, None) if d is None else t.update(d, img)


@pytest.mark.parametrize("name", DHN_NAMES)
def test_dhn_forward_within_four_e_of_the_float64_reference(name):
    g = np.load(os.path.join(GOLDEN, "dhn_%s.npz" % name))
    net = device_dhn(int(g["seed"]), float(g["scale"]))
    out = net(g["D"]).cpu().numpy()
    err = float(np.abs(out.astype(np.float64) - g["out64"]).max())
    print("dhn %s: device max |out - out64| = %.3g, reference's own e_ref = %.3g, bound 4 E = %.3g" % (name, err, float(g["e_ref"]), 4 * float(g["E"])))
    assert out.shape == g["out64"].shape and out.dtype == np.float32
    assert err <= 4 * float(g["E"])


@pytest.mark.parametrize("name", ["3x5", "33x20"])
def test_dhn_forward_is_bit_identical_from_call_to_call(name):
    g = np.load(os.path.join(GOLDEN, "dhn_%s.npz" % name))
    net = device_dhn(int(g["seed"]), float(g["scale"]))
    first = net(g["D"]).cpu().numpy()
    other = net(np.random.default_rng(1).uniform(0, 1, (7, 9)).astype(np.float32))      # (another matrix in between: nothing of it may survive)
    assert other.shape == (7, 9)
    for _ in range(3):
        assert np.array_equal(net(g["D"]).cpu().numpy(), first)


def test_dhn_refuses_bad_arguments():
    from yolov7_tracker_amd import _lib
    net = device_dhn(7, 3.0)
    with pytest.raises(_lib.Y7TError, match="exceeds the workspace"):
        net(np.zeros((65, 48), np.float32))
    L = _lib.load()
    assert L.y7t_dhn_workspace_bytes(0, 5) == 0 and L.y7t_dhn_workspace_bytes(2048, 2048) == 0 and L.y7t_dhn_num_weights() == 4093825
    junk = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
    assert L.y7t_dhn_forward_f32(_lib.ptr(junk), _lib.ptr(d), 2, 2, _lib.ptr(d), _lib.stream_ptr()) == -4      # no network at that address


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("name", NAMES)
def test_deepmot_tracker_matches_reference_golden(name, threads):
    """ids, classes, scores and the tracked / lost lists exactly, tlwh at util's tolerance, on every frame"""
    g = load_golden(name)
    t = new_tracker(g, threads)
    for f in range(len(g["dets"])):
        tc.check_tracks(step(t, g, f), g, f, False, tc.id_lists(t))


def test_two_trackers_share_one_network_object():
    ga, gb = load_golden("default"), load_golden("miss")
    ta = new_tracker(ga)
    tb = DeepMOT(tc.opts(gb["conf"], 0, gb["kalman_format"], max_tracks=256, max_dets=256), frame_rate=30, dhn=ta.DHN)
    # the id counter is shared by the trackers of a process: compare the lists' sizes and the boxes, frame by frame, interleaved
    for f in range(12):
        ca, cb = step(ta, ga, f), step(tb, gb, f)
        for g, cur in ((ga, ca), (gb, cb)):
            np.testing.assert_allclose(np.array([t.tlwh for t in cur], np.float64).reshape(-1, 4), g["frames"][f][1], rtol=util.TLWH_RTOL, atol=util.TLWH_ATOL)
        assert [len(x) for x in tc.id_lists(ta)] == [len(ga["tracked"][f]), len(ga["lost"][f])] and [len(x) for x in tc.id_lists(tb)] == [len(gb["tracked"][f]), len(gb["lost"][f])]


def test_frames_that_skip_the_network_equal_the_host_build():
    """the first frame (empty pool), a frame without detections at all and one with low detections only run no network; the device and the CPU build agree"""
    g = load_golden("default")
    t = new_tracker(g)
    host = hdm.HostDeepMOT(hdm.torch_net(g["seed"], g["scale"]), g["img_shape"], conf_thresh=g["conf"], kalman_format=g["kalman_format"])
    low = g["dets"][3].copy()
    low[:, 4] = 0.17
    img = types.SimpleNamespace(shape=g["img_shape"] + (3,))
    for k, d in enumerate([g["dets"][0], g["dets"][1], np.zeros((0, 6), np.float32), low, g["dets"][4], g["dets"][5]]):
        cur, rows = t.update(d, img), host.update(d)
        assert [c.track_id for c in cur] == [r[0] for r in rows], k
        np.testing.assert_allclose(np.array([c.tlwh for c in cur], np.float64).reshape(-1, 4), np.array([r[1] for r in rows]).reshape(-1, 4), rtol=util.TLWH_RTOL, atol=util.TLWH_ATOL)
        sn = t._snapshot()
        assert (int(sn["hdr_n_tracked"]), int(sn["hdr_n_lost"])) == tuple(len(x) for x in tc.id_lists(host)), k
    assert len(host.net_shapes) == 3      # frames 1, 4 and 5 of the six


def test_entry_points_refuse_the_wrong_pool():
    """y7t_tracker_step with detections and y7t_tracker_step_frames return Y7T_E_STATE and set status bit 8 on a DeepMOT pool; y7t_tracker_step_batch sets bit 8 on the
    DeepMOT pool of a batch, returns no rows for it and steps the ByteTrack pool beside it; the DeepSORT and StrongSORT steps refuse it; y7t_tracker_step_deepmot refuses
    pools of other kinds; the predict-only step is accepted"""
    from yolov7_tracker_amd import _lib
    cap = 256
    dhn = device_dhn(7, 3.0)
    L, st, ids, out = tc.raw_pool("deepmot")
    d = torch.tensor([[10, 10, 60, 90, 0.9, 0]], dtype=torch.float32, device="cuda")
    cnt = ctypes.c_void_p(out.data_ptr() + cap * 64)
    assert L.y7t_tracker_step(_lib.ptr(st), None, -1, _lib.ptr(out), cap, cnt, 0, None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert tc.pool_status(L, st) == 0
    r = L.y7t_tracker_step(_lib.ptr(st), _lib.ptr(d), 1, _lib.ptr(out), cap, cnt, 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st) & 8 and b"DeepMOT" in L.y7t_last_error()
    _, st2, _, out2 = tc.raw_pool("deepmot")
    tab = torch.tensor([d.data_ptr(), out2.data_ptr(), out2.data_ptr() + cap * 64], dtype=torch.int64, device="cuda")
    n1 = torch.ones(1, dtype=torch.int32, device="cuda")
    r = L.y7t_tracker_step_frames(_lib.ptr(st2), _lib.ptr(tab[0:1]), _lib.ptr(n1), _lib.ptr(tab[1:2]), _lib.ptr(tab[2:3]), cap, 1, 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st2) & 8
    _, st3, _, out3 = tc.raw_pool("deepmot")
    _, st4, _, out4 = tc.raw_pool("bytetrack")
    states = torch.tensor([st3.data_ptr(), st4.data_ptr()], dtype=torch.int64, device="cuda")
    dets = torch.tensor([d.data_ptr(), d.data_ptr()], dtype=torch.int64, device="cuda")
    outs = torch.tensor([out3.data_ptr(), out4.data_ptr()], dtype=torch.int64, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    ndets = torch.ones(2, dtype=torch.int32, device="cuda")      # (bound to a name: it lives until the launches that read it are through)
    for threads in (0, 1024):
        _lib.check(L.y7t_tracker_step_batch(_lib.ptr(states), _lib.ptr(dets), _lib.ptr(ndets), _lib.ptr(outs),
                                            _lib.ptr(counts), cap, 2, threads, None, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert tc.pool_status(L, st3) & 8 and tc.pool_status(L, st4) == 0 and counts.tolist()[0] == 0
    # the appearance trackers' steps on a DeepMOT pool
    _, st5, _, out5 = tc.raw_pool("deepmot")
    cnt5 = ctypes.c_void_p(out5.data_ptr() + cap * 64)
    f = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
    fb = int(L.y7t_deepsort_feature_bytes(cap, cap, 128, 8))
    feat = torch.zeros(fb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_deepsort_init(_lib.ptr(feat), fb, cap, cap, 128, 8, _lib.stream_ptr()))
    r = L.y7t_tracker_step_deepsort(_lib.ptr(st5), _lib.ptr(feat), cap, _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(out5), cap, cnt5, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st5) & 8
    _, st6, _, out6 = tc.raw_pool("deepmot")
    sb = int(L.y7t_strongsort_feature_bytes(cap, cap, 128))
    sfeat = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_strongsort_init(_lib.ptr(sfeat), sb, cap, cap, 128, 0.1, _lib.stream_ptr()))
    r = L.y7t_tracker_step_strongsort(_lib.ptr(st6), _lib.ptr(sfeat), _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(out6), cap, ctypes.c_void_p(out6.data_ptr() + cap * 64), 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st6) & 8
    # the DeepMOT step on pools of other kinds
    held = [st, st2, st3, st4, st5, st6]
    for kind in ("bytetrack", "uavmot", "strongsort"):
        _, st7, _, out7 = tc.raw_pool(kind)
        r = L.y7t_tracker_step_deepmot(_lib.ptr(st7), dhn.ptr, _lib.ptr(d), 1, 720, 1280, _lib.ptr(out7), cap, ctypes.c_void_p(out7.data_ptr() + cap * 64), 0, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert r == -4 and tc.pool_status(L, st7) & 8, kind
        held.append(st7)
    for s_ in held:
        L.y7t_tracker_release(_lib.ptr(s_))


def test_overflows_set_the_status():
    """more returned tracks than out_cap: status bit 4 (Y7T_ERR_OUT), the count still the frame's; a pool smaller than the scene: the Python class raises; a pool x detection matrix larger than
    the network's workspace: status bit 32, no rows"""
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker.deepmot import DeviceDHN
    g = load_golden("default")
    dhn = device_dhn(g["seed"], g["scale"])
    cap = 256
    L, st, ids, out = tc.raw_pool("deepmot")
    cnt = ctypes.c_void_p(out.data_ptr() + cap * 64)
    for f in range(3):
        d = torch.from_numpy(g["dets"][f]).cuda()
        _lib.check(L.y7t_tracker_step_deepmot(_lib.ptr(st), dhn.ptr, _lib.ptr(d), d.shape[0], 720, 1280, _lib.ptr(out), cap if f < 2 else 2, cnt, 0, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool(tc.pool_status(L, st) & 4) == (f == 2)
    assert int(out[cap].view(torch.int32)[0]) == len(g["frames"][2][0]) > 2      # (the count is the frame's; the rows stop at out_cap)
    L.y7t_tracker_release(_lib.ptr(st))
    t = new_tracker(g, max_tracks=8)
    with pytest.raises(_lib.Y7TError, match="overflow"):
        for f in range(4):
            step(t, g, f)
    small = DeepMOT(tc.opts(g["conf"], max_tracks=256, max_dets=256), frame_rate=30, dhn=DeviceDHN(synth.make_dhn_weights(7, 3.0), 2, 2))
    step(small, g, 0)
    with pytest.raises(_lib.Y7TError, match="status 32"):
        step(small, g, 1)


def test_track_cli_deepmot_synthetic(tmp_path):
    """tracker/track.py --dataset synthetic --tracker deepmot --dhn_path random:dhn:7:4 --synthetic_dets runs to the end and writes the sequence's result file"""
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    folder = track.cli(["--dataset", "synthetic", "--tracker", "deepmot", "--dhn_path", "random:dhn:7:4", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "640",
                        "--synthetic_dets", "--synthetic_frames", "12", "--synthetic_objs", "20", "--results_root", str(tmp_path)])
    lines = open(os.path.join(folder, "synthetic-000.txt")).read().splitlines()
    assert len(lines) > 50 and lines[0].startswith("1,1,")
