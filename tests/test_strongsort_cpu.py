"""StrongSORT without a GPU: the CPU build of its workgroup program (tests/_hostsim/strongsort.py: the plain forms of the frame's three launches at nt = 1)
against the reference's golden vectors (tests/golden/tracker_strongsort_*.npz, tests/golden/make_golden_strongsort.py) and, where the reference sources
exist, against the live reference on random scenes; the pinned arithmetic -- the float64 Euclidean chain, the float32 moving average, the fuse -- against
scipy / numpy; the port's matching.embedding_distance against the reference's."""
import functools
import os

import numpy as np
import pytest

from tests import _hostsim as hs
from tests import tracker_case as tc
from tests import util
from tests._hostsim import strongsort as hss

GOLDEN = tc.GOLDEN
NAMES = tc.NAMES["strongsort"]
SPARSE_NAMES = ["identity512", "crowd300", "crowd500"]      # identity features and frames of 64 x 64 pairs or more: the sparse component solver
load_golden = functools.partial(tc.load_golden, "strongsort")
maker = functools.partial(tc.maker, "strongsort")


def replay(want, n_frames=None, **kw):
    """run the host build over the scene and compare every frame with `want` (a golden / the live reference's frames) -> the tracker"""
    trk = hss.HostStrongSORT(want["feature_fn"], want["dim"], conf_thresh=want["conf"], gamma=want["gamma"], kalman_format=want["kalman_format"], **kw)
    tc.replay_host(trk, want, n_frames=n_frames)
    return trk


@pytest.mark.parametrize("name", NAMES)
def test_hostsim_strongsort_matches_reference_golden(name):
    """ids, classes and scores exactly, tlwh at util's tolerance, the tracked and lost lists exactly (entries in both lists and stale ones included)
    on every frame; the smoothed vectors at the end bit for bit"""
    g = load_golden(name)
    trk = replay(g)
    assert len(g["final_ids"]) > 0 and g["final_ids"] == g["tracked"][-1][:len(g["final_ids"])]
    for tid, want in zip(g["final_ids"], g["final_features"]):
        got = trk.vector(tc.slot_of(trk, tid))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), "track %d: smoothed vector" % tid


def test_goldens_contain_the_index_quirk():
    """on the golden files themselves: every scene has stale Tracked entries (tracks the second association's misapplied indices left Tracked without an
    update), at least one has a frame with a track in both lists -- visible in the recorded lists, too"""
    any_both = False
    for name in NAMES:
        g = load_golden(name)
        assert int(g["stale"].sum()) > 0, name
        both = [len(set(t) & set(lo)) for t, lo in zip(g["tracked"], g["lost"])]
        assert both == g["both"].tolist(), name
        any_both = any_both or max(both) > 0
    assert any_both


def test_goldens_state_their_environment_and_size():
    assert {str(np.load(os.path.join(GOLDEN, "tracker_strongsort_%s.npz" % n))["kalman_format"]) for n in NAMES} == {"default", "strongsort"}
    for name in NAMES:
        path = os.path.join(GOLDEN, "tracker_strongsort_%s.npz" % name)
        g = np.load(path)
        assert str(g["numpy_version"]) and str(g["scipy_version"]) and os.path.getsize(path) < 400 * 1000, name
        assert g["final_features"].dtype == np.float32 and g["final_features"].shape == (len(g["final_slots_ids"]), int(g["feat_dim"]))


def _stats():
    return [hs.lib().hs_ss_stat(k) for k in range(4)]


def test_boxfeat_takes_the_dense_path():
    """box-size features give a dense candidate graph: no fused association of the boxfeat golden goes through the sparse component solver"""
    before = _stats()
    replay(load_golden("boxfeat"))
    after = _stats()
    assert after[0] == before[0] and (after[1] - before[1]) + (after[3] - before[3]) > 50


def test_dense_candidate_graph_overflows_the_sparse_lists():
    """the same features at 110 objects: the problem is large enough for the sparse solver, whose 24 candidates per row overflow -> the dense lapjv on the
    fused matrix.  Checked against the host build with every assignment solved by the dense path alone (a scene of its own pool)"""
    from yolov7_tracker_amd import synth
    dets = synth.make_detections(14, 110, seq_idx=333, miss=0.05)
    fn = lambda b: synth.make_features(b, dim=128)      # noqa: E731
    before = _stats()
    a = hss.HostStrongSORT(fn, 128)
    rows_a = [a.update(d) for d in dets]
    after = _stats()
    assert after[1] > before[1], "no fused association declined by the sparse solver (%s -> %s)" % (before, after)
    assert max(len(r) for r in rows_a) > 64


@pytest.mark.parametrize("name", SPARSE_NAMES)
def test_identity_goldens_take_the_sparse_path_with_and_without_fast_scratch(name):
    g = load_golden(name)
    before = _stats()
    replay(g)
    assert _stats()[0] > before[0], "no fused association solved by the sparse component solver"
    hs.lib().hs_set_fast_bytes(0)      # every work array in the state blob (the placement branches a workgroup without enough LDS takes)
    try:
        before = _stats()
        replay(g, n_frames=8 if name == "crowd500" else None)
        assert _stats()[0] > before[0]
    finally:
        hs.reset_fast_bytes()


# ---- the pinned arithmetic ----
@pytest.mark.parametrize("dim", [32, 100, 128, 512])
def test_appearance_distance_equals_scipy_cdist(dim):
    """the plain form of k_ss_appearance == np.maximum(0, scipy cdist) of the float32 values cast to float64, bit for bit"""
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(40 + dim)
    u = rng.normal(0, 1, (70, dim)).astype(np.float32)
    v = rng.normal(0, 1, (90, dim)).astype(np.float32)
    u[:20] /= np.linalg.norm(u[:20], axis=1, keepdims=True)      # unit vectors, raw vectors, near-identical pairs, an identical pair
    v[:20] = u[:20] + np.float32(1e-3) * v[:20]
    v[20] = u[20]
    want = np.maximum(0.0, cdist(u.astype(np.float64), v.astype(np.float64)))
    got = hss.cdist(u, v)
    assert np.array_equal(got, want) and got[20, 20] == 0.0


def _ema_numpy(prev, raw):
    """basetrack.py:324-332 as numpy evaluates it on float32 arrays"""
    feature = raw / np.linalg.norm(raw)
    smooth_feat = 0.9 * prev + (1 - 0.9) * feature
    smooth_feat /= np.linalg.norm(smooth_feat)
    return smooth_feat


@pytest.mark.parametrize("dim", [7, 32, 37, 100, 128, 512, 1024])
def test_moving_average_equals_numpy(dim):
    rng = np.random.default_rng(50 + dim)
    for k in range(40):
        prev = rng.normal(0, 1, dim).astype(np.float32)
        if k % 2:
            prev /= np.linalg.norm(prev)      # a smoothed vector; even k: a raw birth vector
        raw = (rng.normal(0, 1, dim) * rng.uniform(0.1, 30)).astype(np.float32)
        want = _ema_numpy(prev, raw)
        got = hss.ema(prev, raw)
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dim, k)


@pytest.mark.parametrize("gamma", [0.1, 0.5])
def test_fuse_equals_python_expression(gamma):
    rng = np.random.default_rng(60)
    a, b = rng.uniform(0, 1, 5000), rng.uniform(0, 2, 5000)
    a[:100] = 1.0
    want = gamma * a + (1. - gamma) * b
    got = np.array([hs.lib().hs_ss_fuse(gamma, x, y) for x, y in zip(a, b)])
    assert np.array_equal(got, want)


def test_feature_vectors_follow_the_slot_not_its_previous_track():
    """a slot that is freed and reused starts with its new track's raw vector; re_activate and frames without a match leave a vector alone"""
    g = load_golden("identity128")
    trk = hss.HostStrongSORT(g["feature_fn"], g["dim"], conf_thresh=g["conf"], gamma=g["gamma"], kalman_format=g["kalman_format"], cap_t=96)      # a small pool: slots are reused
    lo = tc.layout(trk.cap_t, trk.cap_d)
    born = {}
    for f, d in enumerate(g["dets"]):
        rows = trk.update(d, g["warps"][f])
        tc.check_rows(rows, g, f, exact=False)
        tid = trk.blob[lo["tid"]:lo["tid"] + 4 * 96].view(np.int32)
        start = trk.blob[lo["start"]:lo["start"] + 4 * 96].view(np.int32)
        box = trk.blob[lo["box"]:lo["box"] + 16 * 96].view(np.float32).reshape(96, 4)
        for s in range(96):
            if tid[s] > 0 and start[s] == f + 1 and tid[s] not in born:      # born this frame: the raw feature of its detection
                born[int(tid[s])] = s
                tlbr = box[s].copy()
                tlbr[2:] += tlbr[:2]
                assert np.array_equal(trk.vector(s), g["feature_fn"](tlbr[None])[0]), (f, s)
    assert len(set(born.values())) < len(born), "no slot was reused"


def test_pool_and_feature_state_overflow_raise():
    from yolov7_tracker_amd import synth
    dets, fn = synth.make_identity_features(5, 40, 1280, seq_idx=3, dim=32)
    trk = hss.HostStrongSORT(fn, 32, cap_t=16)
    with pytest.raises(RuntimeError, match="capacity"):
        for d in dets:
            trk.update(d)
    trk = hss.HostStrongSORT(fn, 32, cap_t=64, cap_d=64, feat_cap_t=32)      # a feature state smaller than its pool: refused, nothing stepped
    with pytest.raises(RuntimeError, match="feature status 2"):
        trk.update(dets[0])


def test_vectors_follow_the_header():
    assert hs.lib().hs_ss_vec_offset(1024, 1024, 128) == 64      # (tracker/strongsort.py reads the vectors from there)


# ---- against the live reference ----
from oracle import ref_harness  # noqa: E402

needs_ref = pytest.mark.skipif(not ref_harness.available(), reason="reference sources not present")


def _want_from_reference(mg, dets, fn, dim, warps, conf, gamma, kalman_format="strongsort"):
    ref, _ = mg.run_reference(dets, fn, warps, conf, gamma, kalman_format)
    return tc.want_from_reference(ref, dets=dets, feature_fn=fn, warps=warps, dim=dim, conf=conf, gamma=gamma, kalman_format=kalman_format)


@needs_ref
@pytest.mark.parametrize("seed", range(40))
def test_hostsim_strongsort_matches_live_reference(seed):
    """random scenes in the manner of util.random_deepsort_scene (5..90 objects, box-size features on even seeds, identity features with noise on odd
    ones, dimensions 32 / 100 / 128 / 512, frames without detections), with warps on every third seed, gamma / conf_thresh varied and the plain xyah
    Kalman filter instead of the NSA one on every fifth; none is skipped"""
    from yolov7_tracker_amd import synth
    mg = maker()
    dets, fn, dim = util.random_deepsort_scene(seed)
    warps = synth.make_warps(len(dets), seq_idx=400 + seed) if seed % 3 == 0 else None
    conf, gamma = [0.2, 0.3, 0.4, 0.25][seed % 4], [0.1, 0.5, 0.02, 0.9][(seed // 2) % 4]
    replay(_want_from_reference(mg, dets, fn, dim, warps, conf, gamma, "default" if seed % 5 == 4 else "strongsort"))


@needs_ref
def test_hostsim_dense_overflow_scene_matches_live_reference():
    """test_dense_candidate_graph_overflows_the_sparse_lists' scene (the sparse solver declines, dense lapjv on the fused matrix) against the reference"""
    from yolov7_tracker_amd import synth
    dets = synth.make_detections(14, 110, seq_idx=333, miss=0.05)
    fn = lambda b: synth.make_features(b, dim=128)      # noqa: E731
    before = _stats()
    replay(_want_from_reference(maker(), dets, fn, 128, None, 0.2, 0.1))
    assert _stats()[1] > before[1]


@needs_ref
def test_port_embedding_distance_equals_reference():
    from yolov7_tracker_amd.tracker import matching as pm
    rm = ref_harness.load_tracker().matching

    class T:
        def __init__(self, f):
            self.features = [f]
    rng = np.random.default_rng(70)
    for n, m, dim in ((1, 1, 32), (7, 5, 100), (40, 60, 128), (30, 20, 512)):
        a = [T(rng.normal(0, 1, dim).astype(np.float32)) for _ in range(n)]
        b = [T((rng.normal(0, 1, dim) * 3).astype(np.float32)) for _ in range(m)]
        for metric in ("euclidean", "cosine"):
            want = rm.embedding_distance(a, b, metric)
            got = pm.embedding_distance(a, b, metric)
            assert got.dtype == np.float64 and np.array_equal(got, want), (n, m, dim, metric)
        assert np.array_equal(pm.embedding_distance(a, b, "euclidean"), hss.cdist(np.array([t.features[0] for t in a]), np.array([t.features[0] for t in b])))
    assert pm.embedding_distance([], b, "euclidean").shape == (0, len(b))
