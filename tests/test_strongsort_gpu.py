"""StrongSORT on the MI355X: the three launches of a frame (k_ss_appearance, k_tracker_step_strongsort<MAXT>, k_ss_store) through the C ABI and the
Python class, against the reference's golden vectors (tests/golden/tracker_strongsort_*.npz) and the CPU build of the same program; the appearance kernel
alone against numpy's sequential float64 chain; the refusals, the overflows, the ReID seam and the tracker CLI with --tracker strongsort."""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import tracker_case as tc  # noqa: E402
from tests._hostsim import strongsort as hss  # noqa: E402
from yolov7_tracker_amd.tracker.strongsort import StrongSORT  # noqa: E402

NAMES = tc.NAMES["strongsort"]
load_golden = functools.partial(tc.load_golden, "strongsort")


def new_tracker(feature_fn=None, conf=0.2, threads=0, gamma=0.1, kalman_format="strongsort", **kw):
    return tc.new_tracker(StrongSORT, conf, threads, kalman_format, feature_fn, dict(gamma=gamma), **kw)


def run_golden(g, t):
    import warnings
    for f, d in enumerate(g["dets"]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # (scenes without warps: "use_ECC is set but no camera-motion matrix was supplied")
            cur = t.update_without_detection(None, None) if d is None else t.update(d, None, warp=None if g["warps"] is None else g["warps"][f])
        tc.check_tracks(cur, g, f, False, tc.id_lists(t))


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("name", NAMES)
def test_strongsort_tracker_matches_reference_golden(name, threads):
    """ids, classes and scores exactly, tlwh at util's tolerance, the tracked and lost lists exactly on every frame; the smoothed vectors of the tracked
    list after the last frame, read back through the track views, bit for bit"""
    g = load_golden(name)
    t = new_tracker(g["feature_fn"], g["conf"], threads, g["gamma"], kalman_format=g["kalman_format"])
    run_golden(g, t)
    views = {v.track_id: v for v in t.tracked_stracks}
    for tid, want in zip(g["final_ids"], g["final_features"]):
        v = views[tid]
        assert len(v.features) == 1 and v.features[0].dtype == np.float32 and np.array_equal(v.smooth_feat, v.features[0])
        assert np.array_equal(v.features[0].view(np.uint32), want.view(np.uint32)), "track %d: smoothed vector" % tid


def _sequential_cdist(u, v):
    """per pair the chain d = u[k] - v[k]; s += d * d over k = 0 .. dim-1 in float64, then sqrt (numpy fuses nothing: every pair advances a k at a time)"""
    u, v = u.astype(np.float64), v.astype(np.float64)
    s = np.zeros((len(u), len(v)))
    for k in range(u.shape[1]):
        d = u[:, k, None] - v[None, :, k]
        s += d * d
    return np.maximum(0.0, np.sqrt(s))


@pytest.mark.parametrize("n,dim", [(500, 512), (200, 100), (70, 32)])
def test_appearance_kernel_equals_sequential_chain(n, dim):
    """k_ss_appearance alone: n tracks born from the first frame (their vectors are the raw features) against the n detections of the second frame ->
    the frame's appearance matrix in the feature state, bit for bit the sequential float64 chain; dim 100 takes the kernel's plain form"""
    rng = np.random.default_rng(7 + dim)
    side = int(np.ceil(np.sqrt(n)))
    xy = np.array([(40.0 * (k % side) + 5, 50.0 * (k // side) + 5) for k in range(n)], np.float32)
    det = np.concatenate([xy, xy + np.array([20.0, 30.0], np.float32), np.full((n, 1), 0.9, np.float32), np.zeros((n, 1), np.float32)], 1)
    f1 = (rng.normal(0, 1, (n, dim)) * rng.uniform(0.5, 4.0, (n, 1))).astype(np.float32)      # raw network outputs: not normalised
    f2 = f1[rng.permutation(n)] + rng.normal(0, 0.3, (n, dim)).astype(np.float32)
    f2[3] = f1[5]                                                                             # an identical pair: distance 0
    feats = [f1, f2]
    frame = [0]
    t = new_tracker(lambda tlbrs: feats[frame[0]], max_tracks=512, max_dets=512)
    cur = t.update(det, None, warp=np.eye(2, 3))
    assert len(cur) == n
    slot_of_det = {}
    for v in cur:
        k = int(np.argmin(np.abs(xy - v.tlwh[:2]).sum(1)))
        slot_of_det[k] = v._slot
        assert np.array_equal(v.features[0], f1[k])                                            # born with the raw vector
    assert len(slot_of_det) == n
    frame[0] = 1
    t.update(det, None, warp=np.eye(2, 3))
    off = 64 + (512 * dim * 4 + 63) // 64 * 64                                                # header | vectors | appearance matrix (y7t_ss_layout)
    app = t._feat[off:off + 512 * 512 * 8].cpu().numpy().view(np.float64).reshape(512, 512)
    got = np.array([app[slot_of_det[k], :n] for k in range(n)])
    want = _sequential_cdist(f1, f2)
    assert np.array_equal(got, want), "%d of %d distances differ" % (int((got != want).sum()), got.size)
    assert got[5, 3] == 0.0


def test_plain_entry_points_refuse_a_strongsort_pool():
    """y7t_tracker_step with detections and y7t_tracker_step_frames return Y7T_E_STATE and set status bit 8; y7t_tracker_step_batch sets bit 8 on the
    StrongSORT pool of a batch, returns no rows for it and steps the ByteTrack pool beside it; the predict-only step is accepted"""
    from yolov7_tracker_amd import _lib
    cap = 256
    L, st, ids, out = tc.raw_pool("strongsort")
    d = torch.tensor([[10, 10, 60, 90, 0.9, 0]], dtype=torch.float32, device="cuda")
    cnt = ctypes.c_void_p(out.data_ptr() + cap * 64)
    assert L.y7t_tracker_step(_lib.ptr(st), None, -1, _lib.ptr(out), cap, cnt, 0, None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert tc.pool_status(L, st) == 0
    r = L.y7t_tracker_step(_lib.ptr(st), _lib.ptr(d), 1, _lib.ptr(out), cap, cnt, 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st) & 8 and b"StrongSORT" in L.y7t_last_error()
    L2, st2, _, out2 = tc.raw_pool("strongsort")
    tab = torch.tensor([d.data_ptr(), out2.data_ptr(), out2.data_ptr() + cap * 64], dtype=torch.int64, device="cuda")
    n1 = torch.ones(1, dtype=torch.int32, device="cuda")
    r = L.y7t_tracker_step_frames(_lib.ptr(st2), _lib.ptr(tab[0:1]), _lib.ptr(n1), _lib.ptr(tab[1:2]), _lib.ptr(tab[2:3]), cap, 1, 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st2) & 8
    # a batch of a StrongSORT and a ByteTrack pool
    _, st3, _, out3 = tc.raw_pool("strongsort")
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
    for s_ in (st, st2, st3, st4):
        L.y7t_tracker_release(_lib.ptr(s_))


def test_deepsort_step_refuses_a_strongsort_pool_and_strongsort_step_another_kind():
    from yolov7_tracker_amd import _lib
    cap = 256
    L, st, _, out = tc.raw_pool("strongsort")
    cnt = ctypes.c_void_p(out.data_ptr() + cap * 64)
    fb = int(L.y7t_deepsort_feature_bytes(cap, cap, 128, 8))
    feat = torch.zeros(fb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_deepsort_init(_lib.ptr(feat), fb, cap, cap, 128, 8, _lib.stream_ptr()))
    d = torch.tensor([[10, 10, 60, 90, 0.9, 0]], dtype=torch.float32, device="cuda")
    f = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
    r = L.y7t_tracker_step_deepsort(_lib.ptr(st), _lib.ptr(feat), cap, _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(out), cap, cnt, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st) & 8
    for kind in ("bytetrack", "deepsort", "uavmot"):
        L, st2, _, out2 = tc.raw_pool(kind)
        sb = int(L.y7t_strongsort_feature_bytes(cap, cap, 128))
        sfeat = torch.zeros(sb, dtype=torch.uint8, device="cuda")
        _lib.check(L.y7t_strongsort_init(_lib.ptr(sfeat), sb, cap, cap, 128, 0.1, _lib.stream_ptr()))
        r = L.y7t_tracker_step_strongsort(_lib.ptr(st2), _lib.ptr(sfeat), _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(out2), cap,
                                          ctypes.c_void_p(out2.data_ptr() + cap * 64), 0, None, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert r == -4 and tc.pool_status(L, st2) & 8, kind
        L.y7t_tracker_release(_lib.ptr(st2))
    L.y7t_tracker_release(_lib.ptr(st))


def test_strongsort_refuses_the_botsort_kalman_filter():
    from yolov7_tracker_amd import _lib
    with pytest.raises(NotImplementedError):
        new_tracker(kalman_format="botsort")
    L = _lib.load()
    nbytes = int(L.y7t_tracker_state_bytes(64, 64))
    st = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.y7t_tracker_init(_lib.ptr(st), nbytes, StrongSORT._KIND, 2, 64, 64, 0.2, 0.5, 30, 1, _lib.ptr(ids), _lib.stream_ptr()) == -1


def test_pool_and_feature_state_overflow_raise():
    from yolov7_tracker_amd import _lib, synth
    dets, fn = synth.make_identity_features(5, 60, 1280, seq_idx=3, dim=32)
    t = new_tracker(fn, max_tracks=24)
    with pytest.raises(_lib.Y7TError, match="overflow"):
        for d in dets:
            t.update(d, None, warp=np.eye(2, 3))
    # a feature state that is smaller than the pool it is stepped with: the step refuses, update raises on the feature state's status
    t = new_tracker(fn, max_tracks=128, max_dets=128)
    t._ensure_feature_state(32)
    nb = int(t._L.y7t_strongsort_feature_bytes(64, 128, 32))
    t._feat = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    _lib.check(t._L.y7t_strongsort_init(_lib.ptr(t._feat), nb, 64, 128, 32, 0.1, _lib.stream_ptr()))
    with pytest.raises(_lib.Y7TError, match="feature state"):
        t.update(dets[0], None, warp=np.eye(2, 3))


def test_pool_starts_clean_after_release_and_reinit():
    """the same blob (and the same feature state) released and initialised again: no track, no vector of the first life shows in the second"""
    from yolov7_tracker_amd import _lib
    g = load_golden("identity128")
    assert g["kalman_format"] == "strongsort"
    t = new_tracker(g["feature_fn"], g["conf"], 0, g["gamma"])
    for f in range(12):
        t.update(g["dets"][f], None, warp=g["warps"][f])
    assert len(t.tracked_stracks) > 10
    L = t._L
    L.y7t_tracker_release(_lib.ptr(t._state))
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack, _IdCounter
    BaseTrack._count = 0
    _lib.check(L.y7t_tracker_init(_lib.ptr(t._state), t._state.numel(), t._KIND, 3, t.cap_t, t.cap_d, g["conf"], 0.5, 30, t._flags, _lib.ptr(_IdCounter.tensor()),
                                  _lib.stream_ptr()))
    _lib.check(L.y7t_strongsort_init(_lib.ptr(t._feat), t._feat.numel(), t.cap_t, t.cap_d, t._feat_dim, g["gamma"], _lib.stream_ptr()))
    t.frame_id = 0
    t._snap_cache = t._vec_cache = None
    assert t.tracked_stracks == [] and t.lost_stracks == []
    run_golden(g, t)


def test_update_and_launch_agree_row_for_row():
    """same commit, injected features: update() (the get_feature seam, host staging) and _launch() (device tensors, the pipeline form) step two pools to the
    same rows, lists and vectors"""
    g = load_golden("identity512")
    a = new_tracker(g["feature_fn"], g["conf"], 0, g["gamma"], kalman_format=g["kalman_format"])
    b = StrongSORT(tc.opts(g["conf"], kalman_format=g["kalman_format"]), frame_rate=30, gamma=g["gamma"])
    out = torch.zeros((b.cap_t + 1, 8), dtype=torch.float64, device="cuda")
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    for f, d in enumerate(g["dets"]):
        c0 = BaseTrack._count                      # (the id counter is the process's: both pools draw this frame's ids from the same start)
        cur = a.update(d, None, warp=g["warps"][f])
        c1 = BaseTrack._count
        BaseTrack._count = c0
        feats = np.zeros((max(len(d), 1), g["dim"]), np.float32)
        keep = d[:, 4] > np.float32(g["conf"])
        if keep.any():
            feats[keep] = g["feature_fn"](d[keep, :4])
        w = torch.from_numpy(np.ascontiguousarray(g["warps"][f], np.float64).reshape(6)).cuda()
        b._launch(torch.from_numpy(d).cuda(), torch.from_numpy(feats).cuda(), warp=w, out=out)
        torch.cuda.synchronize()
        assert BaseTrack._count == c1
        h = out.cpu().numpy()
        rows = h[:int(h[b.cap_t].view(np.int32)[0])]
        assert rows[:, 0].astype(np.int64).tolist() == [x.track_id for x in cur], "frame %d" % f
        assert np.array_equal(rows[:, 1:5], np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4)), "frame %d" % f
        assert rows[:, 7].astype(np.int64).tolist() == [x._slot for x in cur]
    assert b._status() == 0 and b._feature_status() == 0 and tc.id_lists(a) == tc.id_lists(b)
    assert np.array_equal(a._vectors(), b._vectors())


def test_device_equals_host_build_where_the_sparse_solver_declines():
    """box-size features at 110 objects: more than 24 candidates per row -> the dense lapjv on the fused matrix, the row / column tie watch and the literal
    re-solve; the device (512 threads) against the CPU build of the same program, frame by frame"""
    from yolov7_tracker_amd import synth
    dets = synth.make_detections(14, 110, seq_idx=333, miss=0.05)
    fn = lambda b: synth.make_features(b, dim=128)      # noqa: E731
    host = hss.HostStrongSORT(fn, 128, kalman_format="strongsort")
    t = new_tracker(fn, threads=512)
    warp = np.eye(2, 3)
    for f, d in enumerate(dets):
        want = host.update(d, warp)
        cur = t.update(d, None, warp=warp)
        assert [x.track_id for x in cur] == [r[0] for r in want], "frame %d" % f
        assert np.array_equal(np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4), np.array([r[1] for r in want]).reshape(-1, 4)), "frame %d" % f


def test_update_with_the_device_reid_extractor():
    """the get_feature seam with ReIDExtractor(None, size=(256, 128)) -- OSNet x0.25 on 256 x 128 crops, the fp32 op list -- on synth.make_frames: it runs,
    and the tracks carry finite feat_dim-wide vectors"""
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker.reid import ReIDExtractor
    from yolov7_tracker_amd.tracker.strongsort import REID_SIZE
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    assert REID_SIZE == (256, 128)
    BaseTrack._count = 0
    ext = ReIDExtractor(None, size=(256, 128), max_crops=64)
    assert not ext.fused and (ext.in_w, ext.in_h) == (256, 128)
    t = StrongSORT(tc.opts(0.2, kalman_format="strongsort"), frame_rate=30, gamma=0.1, reid_model=ext)
    frames = synth.make_frames(4, 30, 640, seq_idx=2)
    dets = synth.make_detections(4, 30, 640, seq_idx=2, miss=0.0, fp=0.0)
    n_tracks = 0
    for fr, d in zip(frames, dets):
        cur = t.update(d, fr, warp=np.eye(2, 3))
        n_tracks = max(n_tracks, len(cur))
        for v in cur:
            assert len(v.features) == 1 and v.features[0].shape == (ext.feat_dim,) and np.isfinite(v.features[0]).all() and np.abs(v.features[0]).max() > 0
    assert n_tracks > 5 and t._feat_dim == ext.feat_dim


def test_use_ecc_without_a_warp_warns_once_and_the_ecc_object_is_called():
    g = load_golden("identity128")
    StrongSORT._warned = False
    t = new_tracker(g["feature_fn"], g["conf"], 0, g["gamma"])
    with pytest.warns(RuntimeWarning, match="use_ECC"):
        t.update(g["dets"][0], None)
    t2 = new_tracker(g["feature_fn"], g["conf"], 0, g["gamma"])
    calls = []

    class ECC:
        def apply(self, raw_frame, detections=None):
            calls.append(1)
            return g["warps"][len(calls) - 1]
    t2.ECC = ECC()
    for f in range(15):
        tc.check_tracks(t2.update(g["dets"][f], None), g, f, False)
    assert len(calls) == 15


def test_track_cli_strongsort_synthetic(tmp_path):
    """tracker/track.py --dataset synthetic --tracker strongsort --reid_model_path random:osnet --synthetic_dets writes results (kalman_format is set to
    strongsort like the reference's track.py:70-71)"""
    import warnings
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        folder = track.cli(["--dataset", "synthetic", "--tracker", "strongsort", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "1280",
                            "--reid_model_path", "random:osnet", "--synthetic_dets", "--synthetic_frames", "12", "--synthetic_objs", "30",
                            "--results_root", str(tmp_path)])
    assert os.path.basename(folder).startswith("strongsort_")
    lines = open(os.path.join(folder, "synthetic-000.txt")).read().splitlines()
    assert len(lines) > 50 and len({ln.split(",")[0] for ln in lines}) == 12 and all(len(ln.split(",")) == 10 for ln in lines)
