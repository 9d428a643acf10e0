"""BoT-SORT with its appearance branch on the CPU: the host build of csrc/y7t_track_botsort_reid.h (tests/_hostsim/botsort_reid.py) against the reference's golden
vectors (tests/golden/tracker_botsort_reid_*.npz) and, where the reference is present, against the reference itself; its pinned arithmetic -- the normalisation, the
cosine's FMA chain, the two gates -- against numpy; and the sparsity: a cosine is taken for the pairs at or under theta_iou and for no other."""
import numpy as np
import pytest

from oracle import ref_harness
from tests import botsort_reid_case as bc
from tests import tracker_case as tc
from tests._hostsim import botsort_reid as hbr

NAMES = bc.names()


def test_the_twelve_scenes_are_there():
    assert NAMES == ["default", "cross", "theta", "lowconf_gaps", "rawnorm", "unconfirmed", "gmc", "dim512", "dim100", "conf04", "empty", "crowd300"]


@pytest.mark.parametrize("name", NAMES)
def test_host_build_matches_reference_golden(name):
    """ids, classes, scores and both id lists exactly on every frame, tlwh at util's tolerance; the smoothed vectors of the tracked list after the last frame bit for bit"""
    g = bc.load_golden(name)
    t = bc.host_tracker(g)
    tc.replay_host(t, g)
    assert len(g["final_ids"]) > 0
    for tid, want in zip(g["final_ids"], g["final_features"]):
        assert np.array_equal(t.vector(tc.slot_of(t, tid)).view(np.uint32), want.view(np.uint32)), "track %d: smoothed vector" % tid


def test_goldens_keep_their_distance_from_both_thresholds_and_cover_the_gates():
    """what the generator asserted when the files were made, read back from them"""
    mg = bc.maker()
    for name in NAMES:
        g = bc.load_golden(name)
        assert g["margin_iou"] >= mg.MARGIN and g["margin_emb"] >= mg.MARGIN, name
    assert (bc.load_golden("theta")["gate_counts"] > 0).all()
    assert bc.load_golden("cross")["differs"] >= 1 and bc.load_golden("unconfirmed")["differs"] >= 1
    assert any(d is None for d in bc.load_golden("lowconf_gaps")["dets"])


def _rows(rng, n, dim, lo=0.5, hi=4.0):
    return (rng.standard_normal((n, dim)) * rng.uniform(lo, hi, (n, 1))).astype(np.float32)


@pytest.mark.parametrize("dim", [128, 512, 100, 7, 129, 1000])
def test_pinned_norm_is_numpys_pairwise_sum(dim):
    """np.linalg.norm(axis=1) of the float64 casts, bit for bit: blocks of 128, eight accumulators, the halving of longer rows"""
    x = _rows(np.random.default_rng(dim), 40, dim)
    want = bc.np_norm(x)[:, 0]
    got = np.array([hbr.norm(r) for r in x])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dim", [128, 512, 100])
def test_pinned_cosine_against_numpy(dim):
    """The program's cosine against numpy's cal_cosine_distance on random float32 rows.  numpy's np.dot is the BLAS's dgemm, whose order of summation depends on
    the shapes (measured here: one FMA chain in 256-deep k blocks for large operands, other orders for small ones and single rows), so no one chain is bit-equal to
    it: the program's chain stays within the recorded bound (make_golden_botsort_reid.DOT_DIFF; 1.6e-15 at most was measured) for every shape -- and it IS one
    sequential FMA chain, bit for bit (exact rational emulation)."""
    rng = np.random.default_rng(100 + dim)
    worst = 0.0
    for m, n in ((1, 1), (1, 7), (7, 1), (3, 7), (13, 17), (40, 40), (70, 64)):
        u, v = _rows(rng, m, dim), _rows(rng, n, dim)
        v[: min(m, n)] = u[: min(m, n)] + np.float32(0.1) * rng.standard_normal((min(m, n), dim)).astype(np.float32)      # cosines near 1 as well
        got, want = hbr.cosine(u, v), bc.np_cosine(u, v)
        worst = max(worst, float(np.abs(got - want).max()))
    print("dim %d: largest |chain - np.dot| = %.3g" % (dim, worst))
    assert worst <= bc.maker().DOT_DIFF
    u, v = _rows(rng, 4, dim), _rows(rng, 3, dim)
    assert np.array_equal(hbr.cosine(u, v), bc.np_chain_cosine(u, v))


def test_half_and_gates_against_numpy_on_a_grid_with_exact_equality():
    """0.5 * (1 - dot) and equations 12-13 on a grid that straddles both thresholds; `>` is strict, so a pair exactly at a threshold passes"""
    e = np.spacing(0.5)
    ious = np.array([0.0, 0.1, 0.25 - e / 2, 0.25, 0.25 + e / 2, 0.4, 0.5 - e, 0.5, 0.5 + e, 0.7, 0.9, 1.0])
    halves = np.array([-1e-17, 0.0, 1e-9, 0.1, 0.25 - e / 2, 0.25, 0.25 + e / 2, 0.3, 0.5, 0.5 + e, 0.99, 1.0])
    want = bc.np_gate(ious[:, None] + 0 * halves[None, :], halves[None, :] + 0 * ious[:, None])
    got = np.array([[hbr.gate(a, b) for b in halves] for a in ious])
    assert np.array_equal(got, want)
    assert hbr.gate(0.5, 0.25) == 0.25 and hbr.gate(0.5 + e, 0.1) == 0.5 + e and hbr.gate(0.4, 0.25 + e / 2) == 0.4 and hbr.gate(0.1, 0.25) == 0.1
    dots = np.array([1.0, 1.0 - 2.0 ** -53, 0.5, 0.5 + e, 0.0, -0.3, 1.0 + 2.0 ** -52])
    assert np.array_equal(np.array([hbr.half(d) for d in dots]), 0.5 * (1.0 - dots))


def _predicted_boxes(trk, det, warp=None):
    """independently of the program: the tlbr boxes of the pool (confirmed tracked + lost) and of the unconfirmed tracks after the Kalman prediction and the
    camera motion, out of the host pool's blob (xywh means), and the lists' slots"""
    lo, b = tc.layout(trk.cap_t, trk.cap_d), trk.blob
    i32 = lambda off, n: b[off:off + 4 * n].view(np.int32)      # noqa: E731
    nt, nl = int(i32(lo["hdr_n_tracked"], 1)[0]), int(i32(lo["hdr_n_lost"], 1)[0])
    tracked, lost = i32(lo["tracked"], nt).tolist(), i32(lo["lost"], nl).tolist()
    act, state = i32(lo["act"], trk.cap_t), i32(lo["state"], trk.cap_t)
    mean = b[lo["mean"]:lo["mean"] + 64 * trk.cap_t].view(np.float64).reshape(-1, 8)
    pool = [s for s in tracked if act[s]] + lost
    unconf = [s for s in tracked if not act[s]]

    def box(s, predicted):
        m = mean[s].copy()
        if predicted:
            if state[s] != 1:
                m[7] = 0.0
            m[:4] = m[:4] + m[4:]
        if warp is not None:
            R, t = np.asarray(warp, np.float64).reshape(2, 3)[:, :2], np.asarray(warp, np.float64).reshape(2, 3)[:, 2]
            m = (np.kron(np.eye(4), R) @ m)
            m[:2] += t
        x, y, w, h = m[:4]
        return np.array([x - w / 2, y - h / 2, x + w / 2, y + h / 2])
    return pool, np.array([box(s, True) for s in pool]).reshape(-1, 4), unconf, np.array([box(s, False) for s in unconf]).reshape(-1, 4)


def _iou_dist(a, b):
    from tests._hostsim import lib
    out = np.zeros((len(a), len(b)))
    if len(a) and len(b):
        a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
        lib().hs_iou_cost(a.ctypes.data, len(a), b.ctypes.data, len(b), out.ctypes.data)
    return out


def test_cosines_are_taken_for_the_pairs_at_or_under_theta_iou_only():
    """A 30-object scene: on every frame the program's count of cosines equals the number of pairs with IoU_dist <= 0.5, computed independently with numpy from the
    host pool's boxes (Kalman prediction and camera motion restated above): the pool x the high detections for the first association, plus the unconfirmed tracks x
    the high detections that numpy's own first association (np.minimum of the gated matrices, solved by the dense lapjv) leaves."""
    from tests import _hostsim as hs
    from yolov7_tracker_amd import synth
    dets, fn = synth.make_identity_features(25, 30, 480, seq_idx=71, dim=64, miss=0.1)
    warps = synth.make_warps(25, seq_idx=71)
    t = hbr.HostBoTSORTReID(fn, 64)
    total, dense, third = 0, 0, 0
    for f, d in enumerate(dets):
        pool, pbox, unconf, ubox = _predicted_boxes(t, d, warps[f])
        hi = d[d[:, 4] >= np.float32(0.2)]
        dbox = hi[:, :4].astype(np.float64)
        first = _iou_dist(pbox, dbox)
        want = int((first <= 0.5).sum())
        if len(unconf) and len(hi):
            left = list(range(len(hi)))
            if len(pool):
                half = 0.5 * (1.0 - bc.np_cosine(np.stack([t.vector(s) for s in pool]), fn(hi[:, :4])))
                _, y = hs.lapjv(bc.np_gate(first, half), 0.9, sap=True)
                left = [j for j in range(len(hi)) if y[j] < 0]
            n3 = int((_iou_dist(ubox, dbox[left]) <= 0.5).sum())
            want, third = want + n3, third + n3
        t.update(d, warps[f])
        assert t.n_dots == want, "frame %d: %d cosines for %d pairs at or under theta_iou" % (f, t.n_dots, want)
        total += want
        dense += (len(pool) + len(unconf)) * len(hi)
    assert total > 100 and third > 0 and dense > 10 * total      # (both associations had pairs to count, far fewer than tracks x detections)


@pytest.mark.skipif(not ref_harness.available(), reason="needs the reference sources")
@pytest.mark.parametrize("seed", [201, 202, 203])
def test_host_build_matches_the_reference_live(seed):
    """a random scene per seed (misses, false positives, warps, a noisy appearance): the reference itself, run now, against the host build"""
    from yolov7_tracker_amd import synth
    dets, fn = synth.make_identity_features(30, 35, 560, seq_idx=seed, dim=96, miss=0.15, noise=0.6)
    warps = synth.make_warps(30, seq_idx=seed)
    ref, _, watch = bc.maker().run_reference(dets, fn, warps, 0.3)
    assert min(watch.margin_iou, watch.margin_emb) >= bc.maker().MARGIN
    want = tc.want_from_reference(ref, dets=dets, warps=warps)
    t = hbr.HostBoTSORTReID(fn, 96, conf_thresh=0.3)
    tc.replay_host(t, want)
    assert sum(watch.evaluated) > 200
