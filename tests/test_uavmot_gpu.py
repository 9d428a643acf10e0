"""UAVMOT on the MI355X: the device frame step (csrc/y7t_track_step.h: y7t_tracker_step_body_t<true>, the AMF pass) through every entry point --
UAVMOT frame by frame, y7t_tracker_step_frames, y7t_tracker_step_batch -- against the reference's golden vectors (tests/golden/tracker_uavmot_*.npz) and
the CPU build of the same program; y7t_structure_distance_f64 (the device's atan2 among it) against a numpy restatement; the tracker CLI with
--tracker uavmot."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import _hostsim as hs  # noqa: E402
from tests import tracker_case as tc  # noqa: E402
from tests import util  # noqa: E402
from yolov7_tracker_amd.tracker.uavmot import UAVMOT  # noqa: E402

NAMES = tc.NAMES["uavmot"]
load_golden = functools.partial(tc.load_golden, "uavmot")
new_tracker = functools.partial(tc.new_tracker, UAVMOT)


@pytest.mark.parametrize("threads", [64, 256, 1024])
@pytest.mark.parametrize("name", NAMES)
def test_uavmot_tracker_matches_reference_golden(name, threads):
    g = load_golden(name)
    t = new_tracker(g["conf"], threads, kalman_format=g["kalman_format"])
    for f, d in enumerate(g["dets"]):
        cur = t.update(d, None)
        check = f % 10 == 9 or f == len(g["dets"]) - 1
        tc.check_tracks(cur, g, f, False, ([x.track_id for x in t.tracked_stracks], [x.track_id for x in t.lost_stracks]) if check else None)


def test_uavmot_track_views_have_get_xy():
    g = load_golden("default")
    t = new_tracker()
    for d in g["dets"][:5]:
        cur = t.update(d, None)
    tr = cur[0]
    assert np.array_equal(tr.get_xy(), tr.tlwh2xywh(tr.tlwh)[:2])
    assert all(hasattr(x, "get_xy") for x in t.tracked_stracks + t.lost_stracks)


def test_uavmot_update_without_detection():
    """update_without_detection is ByteTrack's (basetrack.py:489-537): the device step against the host build"""
    g = load_golden("misses")
    t, host = new_tracker(), hs.HostSimTracker("uavmot")
    seq = list(g["dets"][:30])
    seq[10:10] = [None, None]
    seq[20:20] = [None]
    for f, d in enumerate(seq):
        want = host.update(d)
        cur = t.update_without_detection(None, None) if d is None else t.update(d, None)
        assert [x.track_id for x in cur] == [r[0] for r in want], "frame %d" % f
        assert np.array_equal(np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4), np.array([r[1] for r in want]).reshape(-1, 4))


def test_uavmot_step_frames_equals_frame_by_frame():
    """y7t_tracker_step_frames (the list arena in LDS) over groups of frames == the frame-by-frame step"""
    g = load_golden("misses")
    t = new_tracker()
    dd = [torch.from_numpy(d).cuda() for d in g["dets"]]
    outs = [torch.zeros((t.cap_t + 1, 8), dtype=torch.float64, device="cuda") for _ in dd]
    for f0 in range(0, len(dd), 16):
        t._launch_frames(t.frames_table(dd[f0:f0 + 16], outs[f0:f0 + 16]))
    torch.cuda.synchronize()
    assert t._status() == 0
    for f, o in enumerate(outs):
        h = o.cpu().numpy()
        rows = h[:int(h[t.cap_t].view(np.int32)[0])]
        ids, tlwh, _, score = g["frames"][f]
        assert rows[:, 0].astype(np.int64).tolist() == ids.tolist(), "frame %d" % f
        np.testing.assert_allclose(rows[:, 1:5], tlwh, rtol=util.TLWH_RTOL, atol=util.TLWH_ATOL)
        assert np.array_equal(rows[:, 6].astype(np.float32), score)
    assert ([x.track_id for x in t.tracked_stracks], [x.track_id for x in t.lost_stracks]) == (g["tracked"][-1], g["lost"][-1])


@pytest.mark.parametrize("threads", [0, 1024])
def test_uavmot_batch_mixed_with_shared_id_counter_equals_single_runs(threads):
    """y7t_tracker_step_batch over UAVMOT, ByteTrack and C-BIoU pools with ONE id counter: every pool returns the rows of its single run (boxes, classes,
    scores, slots), each of its ids stands for one id of the single run, and no id is handed out twice"""
    from yolov7_tracker_amd import _lib, synth
    L = _lib.load()
    kinds = [hs.HostSimTracker.TRACKERS[k] for k in ("uavmot", "bytetrack", "uavmot", "c_biou", "uavmot")]
    nseq, nfr, cap = len(kinds), 25, 512
    seqs = [synth.make_detections(nfr, 20 + 25 * s, seq_idx=70 + s, miss=0.2) for s in range(nseq)]
    nbytes = int(L.y7t_tracker_state_bytes(cap, cap))

    def mk(ids):
        st = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nseq)]
        for s in range(nseq):
            _lib.check(L.y7t_tracker_init(_lib.ptr(st[s]), nbytes, kinds[s], 0, cap, cap, 0.2, 0.5, 30, 1, _lib.ptr(ids[s]), _lib.stream_ptr()))
        return st
    outs = torch.zeros((nseq, cap + 1, 8), dtype=torch.float64, device="cuda")
    own_ids = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(nseq)]      # one id counter per pool; the states keep their ADDRESSES: the tensors live as long as the states
    st = mk(own_ids)
    single = [[] for _ in range(nseq)]
    for f in range(nfr):
        for s in range(nseq):
            d = torch.from_numpy(seqs[s][f]).cuda()
            _lib.check(L.y7t_tracker_step(_lib.ptr(st[s]), _lib.ptr(d), d.shape[0], _lib.ptr(outs[s]), cap,
                                          ctypes.c_void_p(outs[s].data_ptr() + cap * 64), 0, None, _lib.stream_ptr()))
            torch.cuda.synchronize()
            h = outs[s].cpu().numpy()
            single[s].append(h[:int(h[cap].view(np.int32)[0])].copy())
    shared = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = mk([shared] * nseq)
    state_ptrs = torch.tensor([x.data_ptr() for x in st], dtype=torch.int64, device="cuda")
    out_ptrs = torch.tensor([outs[s].data_ptr() for s in range(nseq)], dtype=torch.int64, device="cuda")
    counts = torch.zeros(nseq, dtype=torch.int32, device="cuda")
    maps = [{} for _ in range(nseq)]
    for f in range(nfr):
        dd = [torch.from_numpy(seqs[s][f]).cuda() for s in range(nseq)]
        det_ptrs = torch.tensor([d.data_ptr() for d in dd], dtype=torch.int64, device="cuda")
        n_dev = torch.tensor([d.shape[0] for d in dd], dtype=torch.int32, device="cuda")
        _lib.check(L.y7t_tracker_step_batch(_lib.ptr(state_ptrs), _lib.ptr(det_ptrs), _lib.ptr(n_dev), _lib.ptr(out_ptrs), _lib.ptr(counts), cap,
                                            nseq, threads, None, _lib.stream_ptr()))
        torch.cuda.synchronize()
        c, h = counts.cpu().numpy(), outs.cpu().numpy()
        for s in range(nseq):
            got, want = h[s, :c[s]], single[s][f]
            assert c[s] == len(want)
            np.testing.assert_array_equal(got[:, 1:], want[:, 1:])
            for a, b in zip(want[:, 0].astype(int), got[:, 0].astype(int)):
                assert maps[s].setdefault(a, b) == b
    allid = [b for m in maps for b in m.values()]
    assert len(allid) == len(set(allid)) and int(shared.item()) >= max(allid)


@pytest.mark.parametrize("seed", range(3))
def test_uavmot_device_equals_host_build_on_crowds(seed):
    from yolov7_tracker_amd import synth
    dets = synth.make_detections(12, 500, seq_idx=95 + seed, miss=0.15, bounce=True)
    host = hs.HostSimTracker("uavmot")
    t = new_tracker(threads=512 if seed != 1 else 256)
    for f, d in enumerate(dets):
        want = host.update(d)
        cur = t.update(d, None)
        assert [x.track_id for x in cur] == [r[0] for r in want], "frame %d" % f
        assert np.array_equal(np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4), np.array([r[1] for r in want]).reshape(-1, 4))


def test_uavmot_pool_overflow_raises():
    from yolov7_tracker_amd import _lib, synth
    t = new_tracker(max_tracks=24)
    with pytest.raises(_lib.Y7TError, match="overflow"):
        for d in synth.make_detections(5, 60, seq_idx=3):
            t.update(d, None)


def test_uavmot_pool_refused_by_deepsort_step():
    from yolov7_tracker_amd import _lib
    t = new_tracker()
    L = t._L
    fb = int(L.y7t_deepsort_feature_bytes(t.cap_t, t.cap_d, 128, 8))
    feat = torch.zeros(fb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_deepsort_init(_lib.ptr(feat), fb, t.cap_t, t.cap_d, 128, 8, _lib.stream_ptr()))
    d = torch.tensor([[10, 10, 60, 90, 0.9, 0]], dtype=torch.float32, device="cuda")
    f = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
    r = L.y7t_tracker_step_deepsort(_lib.ptr(t._state), _lib.ptr(feat), t.cap_t, _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(t._out), t.cap_t, t._count_ptr, 0,
                                    _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r != 0 and t._status() & 8      # Y7T_ERR_KIND


# ---- y7t_structure_distance_f64: the device's angle and cosine arithmetic ----
def _vectors_lattice(xy, f32):
    """structure_representation of centres whose squares and sums are exact (half-pixel lattice, small offsets): there the reference's norms equal
    sqrt(dx^2 + dy^2) in either dtype, so the distances are vectorised; the angles go through math.atan2 (glibc) like the reference's"""
    xy = np.asarray(xy, np.float32 if f32 else np.float64)
    d = xy[:, None, :] - xy[None, :, :]
    lgt = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    ok = (lgt < 400) & (lgt > 0)
    out = np.full((len(xy), 3), 0.0001)
    from yolov7_tracker_amd.tracker.matching import angle
    for a in range(len(xy)):
        idx = np.nonzero(ok[a])[0]
        if len(idx) == 0:
            continue
        ls = lgt[a, idx]
        mx, mn = ls.max(), ls.min()
        out[a, 0], out[a, 1] = mx, mn
        if mx != mn:
            out[a, 2] = angle(xy[idx[np.argmax(ls)]] - xy[a], xy[idx[np.argmin(ls)]] - xy[a])
    return out


def _device_distance(txy, dxy):
    from yolov7_tracker_amd import _lib
    a = torch.as_tensor(np.ascontiguousarray(txy, np.float64)).cuda()
    b = torch.as_tensor(np.ascontiguousarray(dxy, np.float64)).cuda()
    out = torch.empty((len(txy), len(dxy)), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().y7t_structure_distance_f64(_lib.ptr(a), len(txy), _lib.ptr(b), len(dxy), _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu().numpy()


def test_structure_distance_on_half_pixel_lattice():
    """every offset (dx, dy) of a dense half-pixel lattice (|dx|, |dy| <= 24, both signs, the exact directions among them) as the far neighbour of a
    three-point cluster: the device's truncated degrees (ocml's atan2 plus the pinned exact directions) against glibc's through the cosine matrix, for
    the float64 (tracks) and the float32 (detections) arithmetic"""
    from yolov7_tracker_amd.tracker.matching import _structure_cosine
    lat = np.arange(-48, 49) / 2.0
    offs = np.array([(x, y) for x in lat for y in lat if (x, y) != (0.0, 0.0)])
    near = np.array([[0.5, 0.0], [0.0, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -1.0]])
    per_call, n_bad = 300, 0
    for c0 in range(0, len(offs), per_call):
        o = offs[c0:c0 + per_call]
        xy = []
        for k, off in enumerate(o):                      # clusters 1000 px apart: A, A + off (the far one), A + a short offset (the near one)
            A = np.array([1000.0 * (k % 20) + 500.5, 1000.0 * (k // 20) + 500.0])
            nr = near[k % len(near)]
            if abs(np.hypot(*nr) - np.hypot(*off)) < 1e-9:
                nr = nr * 3
            xy += [A, A + off, A + nr]
        xy = np.array(xy)
        want = _structure_cosine(_vectors_lattice(xy, False), _vectors_lattice(xy, True))
        got = _device_distance(xy, xy)
        n_bad += int((got != want).sum())
        assert np.array_equal(got, want), "offsets %d..: %d of %d entries differ" % (c0, int((got != want).sum()), got.size)
    assert n_bad == 0


def test_structure_distance_random_matches_port_restatement():
    """random float64 track centres and float32 detection centres (the 400 px boundary among them) against the port's literal restatement"""
    from yolov7_tracker_amd.tracker import matching as pm
    rng = np.random.default_rng(5)
    for n, m in ((1, 1), (3, 7), (60, 45), (120, 200)):
        t = rng.uniform(0, 1400, (n, 2))
        d = np.round(rng.uniform(0, 1400, (m, 2)) * 2).astype(np.float32) / 2
        if n > 2:
            t[1] = t[0] + [400.0, 0.0]
            t[2] = t[0] + [0.0, 399.99999999999994]
        want = pm._structure_cosine(pm._structure_vectors(t, np.float64), pm._structure_vectors(d, np.float32))
        assert np.array_equal(_device_distance(t, d.astype(np.float64)), want)


def test_local_relation_fuse_motion_through_the_device():
    from yolov7_tracker_amd.tracker import matching as pm
    from yolov7_tracker_amd.tracker.uavmot import AMF_STrack

    class T:
        def __init__(self, xy):
            self.mean = np.array([xy[0], xy[1], 0.5, 80.0, 0, 0, 0, 0])
    rng = np.random.default_rng(6)
    tracks = [T(p) for p in rng.uniform(0, 900, (30, 2))]
    dets = [AMF_STrack(0, np.array([x, y, 20, 40], np.float32), 0.9) for x, y in np.round(rng.uniform(0, 900, (25, 2)))]
    cost = rng.uniform(0, 1, (30, 25))
    s = pm._structure_cosine(pm.structure_representation(tracks), pm.structure_representation(dets, mode="detection"))
    assert np.array_equal(pm.structure_similarity_distance(tracks, dets), s)
    assert np.array_equal(pm.local_relation_fuse_motion(cost, tracks, dets), 0.98 * cost + (1 - 0.98) * s)
    assert math.isclose(1 - 0.98, 0.020000000000000018)


def _host_result_lines(dets, min_area=150):
    """the MOT result lines tracker/track.py writes, from the host build's rows"""
    host = hs.HostSimTracker("uavmot")
    lines = []
    for f, d in enumerate(dets):
        for tid, b, _, _ in host.update(d):
            if b[2] * b[3] > min_area:
                lines.append(f'{f + 1},{tid},{b[0]:.2f},{b[1]:.2f},{b[2]:.2f},{b[3]:.2f},1.0,-1,-1,-1\n')
    return "".join(lines)


@pytest.mark.parametrize("batch", [1, 8])
def test_track_cli_uavmot_synthetic(tmp_path, batch):
    """tracker/track.py --dataset synthetic --tracker uavmot --synthetic_dets: the result file of the host build on the same sequence"""
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    folder = track.cli(["--dataset", "synthetic", "--tracker", "uavmot", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "1280",
                        "--synthetic_dets", "--synthetic_frames", "100", "--synthetic_objs", "80", "--results_root", str(tmp_path), "--batch", str(batch)])
    got = open(os.path.join(folder, "synthetic-000.txt")).read()
    assert got == _host_result_lines(load_golden("default")["dets"])
