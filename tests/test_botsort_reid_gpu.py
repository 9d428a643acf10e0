"""BoT-SORT with its appearance branch on the MI355X: the three launches of a frame (k_br_prepare, k_tracker_step_botsort_reid<MAXT>, k_br_store) through the C ABI
and the Python class, against the reference's golden vectors (tests/golden/tracker_botsort_reid_*.npz) and the CPU build of the same program; the cosines the step
evaluated, read back from the feature state; the refusals, the status bits, the pipeline form and the tracker CLI with --botsort_reid; and the state path, untouched."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import botsort_reid_case as bc  # noqa: E402
from tests import tracker_case as tc  # noqa: E402
from tests._hostsim import botsort_reid as hbr  # noqa: E402
from yolov7_tracker_amd.tracker.botsort import BoTSORT, BoTSORTReID  # noqa: E402

NAMES = bc.names()


def new_tracker(feature_fn=None, conf=0.2, threads=0, **kw):
    """through BoTSORT's own constructor: the keyword selects the path"""
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    t = BoTSORT(tc.opts(conf, threads, "botsort", **kw), frame_rate=30, use_apperance_model=True)
    assert type(t) is BoTSORTReID and t.use_apperance_model and t._KIND == bc.KIND
    if feature_fn is not None:
        t.get_feature = lambda tlbrs, ori_img, _fn=feature_fn: _fn(tlbrs)
    return t


def step(t, g, f):
    d = g["dets"][f]
    return t.update_without_detection(None, None) if d is None else t.update(d, None, warp=None if g["warps"] is None else g["warps"][f])


@pytest.mark.parametrize("name,threads", [(n, th) for n in NAMES for th in ((512,) if n == "crowd300" else (256, 512, 1024))])
def test_tracker_matches_reference_golden(name, threads):
    """ids, classes and scores exactly, tlwh at util's tolerance, the tracked and lost lists exactly on every frame; the smoothed vectors of the tracked list after
    the last frame, read back through the track views, bit for bit.  (`cross` and `unconfirmed` differ from the state path's ids by construction.)"""
    g = bc.load_golden(name)
    t = new_tracker(g["feature_fn"], g["conf"], threads)
    for f in range(len(g["dets"])):
        tc.check_tracks(step(t, g, f), g, f, False, tc.id_lists(t))
    views = {v.track_id: v for v in t.tracked_stracks}
    assert len(g["final_ids"]) > 0
    for tid, want in zip(g["final_ids"], g["final_features"]):
        v = views[tid]
        assert len(v.features) == 1 and v.features[0].dtype == np.float32 and np.array_equal(v.smooth_feat, v.features[0]) and v.has_feature
        assert np.array_equal(v.features[0].view(np.uint32), want.view(np.uint32)), "track %d: smoothed vector" % tid


@pytest.mark.parametrize("name", ["default", "theta", "gmc"])
def test_device_equals_host_build_frame_by_frame(name):
    """rows bit for bit, both id lists, the count of cosines evaluated and of pairs theta_emb gated, both status words: the device (256 threads) against the CPU build"""
    g = bc.load_golden(name)
    host = bc.host_tracker(g)
    t = new_tracker(g["feature_fn"], g["conf"], 256)
    total = 0
    for f in range(len(g["dets"])):
        want = host.update(g["dets"][f], None if g["warps"] is None else g["warps"][f])
        cur = step(t, g, f)
        assert [x.track_id for x in cur] == [r[0] for r in want], "frame %d" % f
        assert np.array_equal(np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4), np.array([r[1] for r in want]).reshape(-1, 4)), "frame %d" % f
        assert tc.id_lists(t) == tc.id_lists(host), "frame %d" % f
        assert t.cosine_count() == (host.n_dots, host.n_emb), "frame %d" % f
        assert t._status() == 0 and t._feature_status() == 0 and host.feature_status == 0
        total += host.n_dots
    assert total == sum(g["evaluated"]) and total > 500      # (the reference's own count of pairs at or under theta_iou, recorded in the golden)


@pytest.mark.parametrize("dim", [128, 100])
def test_cosines_of_a_70_by_70_frame_equal_the_host_build(dim):
    """70 tracks born on the first frame against the 70 detections of the second (4900 pairs: the sparse solver's path): the pairs the step filed and their
    0.5 * (1 - cos), read back from the feature state's pair table, are the host build's, bit for bit; dim 100 takes the chain's plain loads"""
    rng = np.random.default_rng(11 + dim)
    n, cap = 70, 128
    xy = np.array([(16.0 * (k % 10) + 5, 52.0 * (k // 10) + 5) for k in range(n)], np.float32)      # 60-wide boxes 16 px apart: neighbours sit on both sides of theta_iou
    det1 = np.concatenate([xy, xy + np.array([60.0, 90.0], np.float32), np.full((n, 1), 0.9, np.float32), np.zeros((n, 1), np.float32)], 1)
    det2 = det1.copy()
    det2[:, [0, 2]] += rng.integers(-6, 7, (n, 1)).astype(np.float32)
    f1 = (rng.normal(0, 1, (n, dim)) * rng.uniform(0.5, 4.0, (n, 1))).astype(np.float32)
    f2 = (f1 + rng.normal(0, 0.4, (n, dim)) * rng.uniform(0.5, 4.0, (n, 1))).astype(np.float32)
    feats = {0: f1, 1: f2}
    frame = [0]
    fn = lambda tlbrs: feats[frame[0]]      # noqa: E731
    host = hbr.HostBoTSORTReID(fn, dim, cap_t=cap, cap_d=cap)
    t = new_tracker(fn, max_tracks=cap, max_dets=cap)
    for k, d in enumerate((det1, det2)):
        frame[0] = k
        want = host.update(d, np.eye(2, 3))
        cur = t.update(d, None, warp=np.eye(2, 3))
        assert [x.track_id for x in cur] == [r[0] for r in want] and (k == 1 or len(cur) == n)
    got = hbr.pair_table(t._feat.cpu().numpy(), cap, cap, dim)
    ref = host.pairs()
    assert len(ref) == host.n_dots == t.cosine_count()[0] and 70 <= len(ref) < 700
    assert sorted(got) == sorted(ref)
    bad = [k for k in ref if np.float64(got[k]).view(np.uint64) != np.float64(ref[k]).view(np.uint64)]
    assert not bad, "%d of %d cosines differ" % (len(bad), len(ref))
    # ... and they are the cosines of those vectors: numpy's own, to the recorded bound
    cos = bc.np_cosine(f1, f2)      # (a table row is a pool position = the tracked list's order = the order of birth = the first frame's detection order)
    assert max(abs(ref[(i, j)] - 0.5 * (1.0 - cos[i, j])) for (i, j) in ref) <= bc.maker().DOT_DIFF


def test_plain_entry_points_refuse_a_pool_of_the_new_kind():
    """y7t_tracker_step with detections and y7t_tracker_step_frames return Y7T_E_STATE and set status bit 8; y7t_tracker_step_batch sets bit 8 on such a pool of a
    batch, returns no rows for it and steps the ByteTrack pool beside it; the predict-only step is accepted"""
    from yolov7_tracker_amd import _lib
    cap = 256
    L, st, ids, out = bc.raw_pool()
    d = torch.tensor([[10, 10, 60, 90, 0.9, 0]], dtype=torch.float32, device="cuda")
    cnt = ctypes.c_void_p(out.data_ptr() + cap * 64)
    assert L.y7t_tracker_step(_lib.ptr(st), None, -1, _lib.ptr(out), cap, cnt, 0, None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert tc.pool_status(L, st) == 0
    r = L.y7t_tracker_step(_lib.ptr(st), _lib.ptr(d), 1, _lib.ptr(out), cap, cnt, 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st) & 8 and b"y7t_tracker_step_botsort_reid" in L.y7t_last_error()
    L2, st2, _, out2 = bc.raw_pool()
    tab = torch.tensor([d.data_ptr(), out2.data_ptr(), out2.data_ptr() + cap * 64], dtype=torch.int64, device="cuda")
    n1 = torch.ones(1, dtype=torch.int32, device="cuda")
    r = L.y7t_tracker_step_frames(_lib.ptr(st2), _lib.ptr(tab[0:1]), _lib.ptr(n1), _lib.ptr(tab[1:2]), _lib.ptr(tab[2:3]), cap, 1, 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st2) & 8
    _, st3, _, out3 = bc.raw_pool()
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


def test_the_appearance_steps_refuse_each_others_pools():
    """the DeepSORT and StrongSORT steps on a pool of the new kind, the new step on a pool of any other kind: Y7T_E_STATE and status bit 8"""
    from yolov7_tracker_amd import _lib
    cap = 256
    L, st, _, out = bc.raw_pool()
    cnt = ctypes.c_void_p(out.data_ptr() + cap * 64)
    d = torch.tensor([[10, 10, 60, 90, 0.9, 0]], dtype=torch.float32, device="cuda")
    f = torch.ones((1, 128), dtype=torch.float32, device="cuda")
    fb = int(L.y7t_deepsort_feature_bytes(cap, cap, 128, 8))
    feat = torch.zeros(fb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_deepsort_init(_lib.ptr(feat), fb, cap, cap, 128, 8, _lib.stream_ptr()))
    r = L.y7t_tracker_step_deepsort(_lib.ptr(st), _lib.ptr(feat), cap, _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(out), cap, cnt, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st) & 8
    L.y7t_tracker_release(_lib.ptr(st))
    L, st, _, out = bc.raw_pool()
    cnt = ctypes.c_void_p(out.data_ptr() + cap * 64)
    sb = int(L.y7t_strongsort_feature_bytes(cap, cap, 128))
    sfeat = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_strongsort_init(_lib.ptr(sfeat), sb, cap, cap, 128, 0.1, _lib.stream_ptr()))
    r = L.y7t_tracker_step_strongsort(_lib.ptr(st), _lib.ptr(sfeat), _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(out), cap, cnt, 0, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r == -4 and tc.pool_status(L, st) & 8
    L.y7t_tracker_release(_lib.ptr(st))
    bfeat = bc.raw_feature_state(L, cap, 128)
    for kind, kalman in (("bytetrack", 0), ("botsort", 2), ("deepsort", 0), ("strongsort", 3), ("uavmot", 0)):
        L, st2, _, out2 = tc.raw_pool(kind, kalman=kalman)
        r = L.y7t_tracker_step_botsort_reid(_lib.ptr(st2), _lib.ptr(bfeat), _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(out2), cap,
                                            ctypes.c_void_p(out2.data_ptr() + cap * 64), 0, None, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert r == -4 and tc.pool_status(L, st2) & 8, kind
        L.y7t_tracker_release(_lib.ptr(st2))


def test_the_new_kind_takes_the_botsort_kalman_filter_only():
    from yolov7_tracker_amd import _lib
    L = _lib.load()
    nbytes = int(L.y7t_tracker_state_bytes(64, 64))
    st = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")
    for kalman in (0, 3):
        assert L.y7t_tracker_init(_lib.ptr(st), nbytes, bc.KIND, kalman, 64, 64, 0.2, 0.5, 30, 1, _lib.ptr(ids), _lib.stream_ptr()) == -1
    assert L.y7t_tracker_init(_lib.ptr(st), nbytes, bc.KIND, bc.KALMAN_BOTSORT, 64, 64, 0.2, 0.5, 30, 1, _lib.ptr(ids), _lib.stream_ptr()) == 0
    L.y7t_tracker_release(_lib.ptr(st))
    o = tc.opts(kalman_format="default")
    t = BoTSORT(o, frame_rate=30, use_apperance_model=True)      # (the class sets kalman_format botsort itself, like BoTSORT)
    assert o.kalman_format == "botsort" and t.opts.kalman_format == "botsort"


def test_a_feature_state_smaller_than_the_pool_sets_status_bit_2():
    from yolov7_tracker_amd import _lib
    g = bc.load_golden("default")
    t = new_tracker(g["feature_fn"], max_tracks=128, max_dets=128)
    t._ensure_feature_state(g["dim"])
    nb = int(t._L.y7t_botsort_reid_feature_bytes(64, 128, g["dim"]))
    t._feat = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    _lib.check(t._L.y7t_botsort_reid_init(_lib.ptr(t._feat), nb, 64, 128, g["dim"], 0.5, 0.25, _lib.stream_ptr()))
    with pytest.raises(_lib.Y7TError, match="feature state"):
        t.update(g["dets"][0], None, warp=np.eye(2, 3))
    assert t._feature_status() == 2 and t._status() == 0 and t.tracked_stracks == []


def test_a_zero_norm_vector_stops_the_frame_and_leaves_the_pool():
    """the reference divides by the zero norm and hands NaN costs to lapjv; here the prepare launch sets status bit 4, the step leaves the pool and the vectors as
    they were, and update() raises"""
    from yolov7_tracker_amd import _lib
    g = bc.load_golden("default")
    fn, bad = g["feature_fn"], [False]

    def feature_fn(tlbrs):
        f = np.array(fn(tlbrs), np.float32)
        if bad[0]:
            f[2] = 0.0
        return f
    t = new_tracker(feature_fn, g["conf"])
    for f in range(5):
        t.update(g["dets"][f], None)
    lists, frame_id = tc.id_lists(t), t._snapshot()["hdr_frame_id"]
    blob, vecs = t._state.clone(), t._vectors().copy()
    bad[0] = True
    with pytest.raises(_lib.Y7TError, match="zero or non-finite norm"):
        t.update(g["dets"][5], None)
    assert t._feature_status() == 4 and t._status() == 0
    assert torch.equal(t._state, blob) and tc.id_lists(t) == lists and t._snapshot()["hdr_frame_id"] == frame_id == 5
    t._vec_cache = None
    assert np.array_equal(t._vectors(), vecs)


def test_update_and_launch_agree_and_launch_keeps_device_inputs_on_the_device():
    """update() (the get_feature seam, host staging) and _launch() (device tensors, the pipeline form) step two pools to the same rows, lists and vectors; _launch
    hands the caller's device tensors -- detections, features and the camera-motion matrix -- to the step as they are (no copy through the host)"""
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    g = bc.load_golden("gmc")
    a = new_tracker(g["feature_fn"], g["conf"])
    b = BoTSORT(tc.opts(g["conf"], kalman_format="botsort"), frame_rate=30, use_apperance_model=True)
    out = torch.zeros((b.cap_t + 1, 8), dtype=torch.float64, device="cuda")
    for f, d in enumerate(g["dets"][:30]):
        c0 = BaseTrack._count                      # (the id counter is the process's: both pools draw this frame's ids from the same start)
        cur = a.update(d, None, warp=g["warps"][f])
        c1 = BaseTrack._count
        BaseTrack._count = c0
        feats = np.zeros((max(len(d), 1), g["dim"]), np.float32)
        keep = d[:, 4] >= np.float32(g["conf"])
        if keep.any():
            feats[keep] = g["feature_fn"](d[keep, :4])
        w = torch.from_numpy(np.ascontiguousarray(g["warps"][f], np.float64).reshape(6)).cuda()
        dd, ff = torch.from_numpy(d).cuda(), torch.from_numpy(feats).cuda()
        b._launch(dd, ff, warp=w, out=out)
        kept = b._det_keep
        assert kept[0].data_ptr() == dd.data_ptr() and kept[1].data_ptr() == ff.data_ptr() and kept[2].data_ptr() == w.data_ptr()
        torch.cuda.synchronize()
        assert BaseTrack._count == c1
        h = out.cpu().numpy()
        rows = h[:int(h[b.cap_t].view(np.int32)[0])]
        assert rows[:, 0].astype(np.int64).tolist() == [x.track_id for x in cur], "frame %d" % f
        assert np.array_equal(rows[:, 1:5], np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4)), "frame %d" % f
    assert b._status() == 0 and b._feature_status() == 0 and tc.id_lists(a) == tc.id_lists(b)
    assert np.array_equal(a._vectors(), b._vectors())
    # the gmc callable of the class, with an estimator's device tensor
    c = new_tracker(g["feature_fn"], g["conf"])
    calls = []

    def gmc(raw_frame, detections):
        calls.append(torch.from_numpy(np.ascontiguousarray(g["warps"][len(calls)], np.float64).reshape(6)).cuda())
        return calls[-1]
    c.gmc = gmc
    for f in range(10):
        tc.check_tracks(c.update(g["dets"][f], None), g, f, False)
        assert c._det_keep[2].data_ptr() == calls[-1].data_ptr()
    assert len(calls) == 10


def test_botsort_without_the_flag_is_the_state_path():
    """BoTSORT(opts) -- and BoTSORT(opts, use_apperance_model=False) -- construct the state-path tracker and reproduce its golden: the untouched path"""
    from tests import util
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    _, fmt, dets, frames = util.load_tracker_case("botsort_gmc")
    warps = np.load(os.path.join(tc.GOLDEN, "tracker_botsort_gmc.npz"))["warps"]
    for kw in ({}, {"use_apperance_model": False}):
        BaseTrack._count = 0
        t = BoTSORT(tc.opts(kalman_format=fmt), frame_rate=30, **kw)
        assert type(t) is BoTSORT and t._KIND == 2 and t.use_apperance_model is False
        for f in range(40):
            cur = t.update_without_detection(None, None) if dets[f] is None else t.update(dets[f], None, warp=warps[f])
            assert [x.track_id for x in cur] == [r[0] for r in frames[f]], "frame %d" % f
            np.testing.assert_allclose(np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4), np.array([r[1] for r in frames[f]], np.float64).reshape(-1, 4),
                                       rtol=util.TLWH_RTOL, atol=util.TLWH_ATOL)


@pytest.mark.parametrize("gmc", ["none", "ecc"])
def test_track_cli_botsort_reid_synthetic(tmp_path, gmc):
    """tracker/track.py --dataset synthetic --tracker botsort --botsort_reid --reid_model_path random (the reference's Net on 128 x 64 crops, seeded weights)
    --synthetic_dets writes results, with and without --gmc ecc; the flag belongs to botsort"""
    import warnings
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    args = ["--dataset", "synthetic", "--tracker", "botsort", "--botsort_reid", "--reid_model_path", "random", "--model_path", "random:yolov7-tiny", "--nc", "10",
            "--img_size", "640", "--synthetic_dets", "--synthetic_frames", "8", "--synthetic_objs", "20", "--results_root", str(tmp_path)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        folder = track.cli(args + (["--gmc", "ecc"] if gmc == "ecc" else []))
    assert os.path.basename(folder).startswith("botsort_")
    lines = open(os.path.join(folder, "synthetic-000.txt")).read().splitlines()
    assert len(lines) > 30 and len({ln.split(",")[0] for ln in lines}) == 8 and all(len(ln.split(",")) == 10 for ln in lines)
    if gmc == "none":
        with pytest.raises(ValueError, match="botsort_reid"):
            track.cli([a if a != "botsort" else "bytetrack" for a in args])
