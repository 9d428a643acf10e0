"""DeepSORT's appearance arithmetic without a GPU, as a chain: numpy's own bits (tests/golden/np_norms.npz) pin the two norms of the host build; numpy expressions
evaluated with those norms pin the stored ring row and the normalised detection rows; the host build and the oracle agree on whole scenes whose rings wrap (budgets
3, 35 and the product's 100); and the per-frame check that tests/test_deepsort_feat_gpu.py applies to the device's blobs holds on the host build's."""
import os

import numpy as np
import pytest

from oracle import tracker_np
from tests import _hostsim as hs
from tests import deepsort_feat_case as fc
from tests import tracker_case as tc
from tests import util

G = np.load(os.path.join(util.GOLDEN, "np_norms.npz"))
WIDTHS = [int(w) for w in G["widths"]]


def test_golden_covers_the_widths_of_the_recipe():
    mg = tc.maker("np_norms")
    assert tuple(WIDTHS) == mg.WIDTHS == (1, 2, 3, 7, 8, 31, 32, 33, 64, 96, 100, 128, 160, 200, 256, 384, 512, 1024)
    for w in WIDTHS:
        assert G["x_%d" % w].shape == (64, w) and G["x_%d" % w].dtype == np.float32 and np.array_equal(G["x_%d" % w], mg.vectors(w))


@pytest.mark.parametrize("width", WIDTHS)
def test_row_norm_equals_numpy_bits(width):
    """sqrtf(y7t_np_pairwise_sumsq) == np.linalg.norm(x[None], axis=1)[0] as recorded, every vector"""
    got = np.array([np.sqrt(hs.np_pairwise_sumsq(x)) for x in G["x_%d" % width]], np.float32)
    bad = got.view(np.uint32) != G["rows_%d" % width]
    assert not bad.any(), "%d of 64 vectors differ" % int(bad.sum())


@pytest.mark.parametrize("width", WIDTHS)
def test_vector_norm_equals_numpy_bits(width):
    """sqrtf(y7t_blas_sdot_self) == np.linalg.norm(x) as recorded, every vector (a tail summed in float32 fails here wherever n & 31 leaves two or more elements: widths 3, 7, 8, 31, 100 and 200)"""
    got = np.array([np.sqrt(hs.blas_sdot_self(x)) for x in G["x_%d" % width]], np.float32)
    bad = got.view(np.uint32) != G["vec_%d" % width]
    assert not bad.any(), "%d of 64 vectors differ" % int(bad.sum())


@pytest.mark.parametrize("width", WIDTHS)
def test_stored_row_and_normalised_rows_equal_the_numpy_expressions(width):
    """y7t_feat_store == basetrack.py:324-332 followed by matching.py:165-178's division, y7t_feat_normalize_dets == the latter alone, float32 throughout, with
    the norms numpy recorded (the norm of the intermediate vector f / norm(f), which the golden does not hold, is taken by the host build's sum: pinned above)"""
    x = G["x_%d" % width]
    rows = G["rows_%d" % width].view(np.float32)
    vec = G["vec_%d" % width].view(np.float32)
    assert fc.same_bits(hs.feat_normalize(x), x / rows[:, None])
    for v, nr, nv in zip(x, rows, vec):
        assert fc.same_bits(hs.feat_store(v, 0), v / nr)                       # a new track keeps the raw vector; the distance divides it by its row norm
        f = v / nv                                                             # STrack.update: feat / np.linalg.norm(feat)
        assert fc.same_bits(hs.feat_store(v, 1), f / np.sqrt(hs.np_pairwise_sumsq(f)))


def test_dot_seq_is_dot_sequential():
    rng = np.random.default_rng(3)
    a, b = rng.normal(0, 1, (37, 100)).astype(np.float32), rng.normal(0, 1, (29, 100)).astype(np.float32)
    assert fc.same_bits(fc.dot_seq(a, b.T), tracker_np.dot_sequential(a, b.T))


def test_layout_restatement_equals_the_header():
    for cap_t, cap_d, dim, budget in ((64, 64, 7, 3), (512, 512, 128, 35), (100, 70, 100, 100)):
        assert fc.feat_layout(cap_t, cap_d, dim, budget)["total"] == hs.lib().hs_feat_bytes(cap_t, cap_d, dim, budget)


# ---- the ring wraps: host build == oracle ----
def _host_vs_oracle(scene):
    trk = hs.HostSimTracker("deepsort", feature_fn=scene["feature_fn"], feat_dim=scene["dim"], feat_budget=scene["budget"], cap_t=256, cap_d=256)
    ora = tracker_np.TrackerNP("deepsort", ids=tracker_np.IdCounter())
    ora.feature_fn, ora.dot, ora.feature_budget = scene["feature_fn"], tracker_np.dot_sequential, scene["budget"]
    got, want, longest, relost = [], [], 0, 0
    was_lost = set()
    for f, d in enumerate(scene["dets"]):
        got.append(trk.update(d))
        cur = ora.update(d)
        want.append([(int(t.tid), np.asarray(t.tlwh, np.float64).copy(), float(t.cls), float(t.score)) for t in cur])
        assert tc.id_lists(trk) == ([t.tid for t in ora.tracked], [t.tid for t in ora.lost]), "frame %d: tracked / lost lists" % f
        longest = max([longest] + [len(t.features) for t in ora.tracked + ora.lost])
        relost += sum(1 for t in ora.tracked if t.tid in was_lost and len(t.features) >= scene["budget"])
        was_lost = {t.tid for t in ora.lost}
    util.assert_same_tracks(got, want, "budget %d" % scene["budget"])
    return longest, relost


@pytest.mark.parametrize("budget", [3, 35, 100])
def test_hostsim_deepsort_equals_oracle_across_a_wrap(budget):
    """ids, boxes and the tracked / lost lists on every frame; the scene must fill a ring and re-find a lost track whose ring is full"""
    longest, refound_full = _host_vs_oracle(fc.wrap_scene(budget))
    assert longest == budget and refound_full > 0


# ---- the frame check of the GPU tests, on the host build's blobs ----
@pytest.mark.parametrize("dim", fc.WIDTHS)
def test_frame_check_holds_on_the_host_build_widths(dim):
    """the serial forms against the same reference, and the scene's coverage: detections with candidates of two ages, of one age and with none; a distance above 1
    (a zero row that is not masked would win the minimum); every ring wraps, some twice"""
    sc = fc.widths_scene(dim)
    res = fc.run_case(fc.HostRun(sc["cap"], dim, sc["budget"]), sc["frames"])
    cov = fc.coverage(res)
    assert cov["mixed"] > 0 and cov["one_age"] > 0 and cov["none"] > 0 and cov["max_app"] > 1.0 and max(cov["wraps"]) >= 2 and sum(w > 0 for w in cov["wraps"]) >= 9, cov


def test_frame_check_holds_on_the_host_build_shape():
    """130 objects, budget 35, slots with different counts in one frame (the host build runs the serial forms at any width: 32 keeps it short)"""
    sc = fc.shape_scene(32)
    choose = fc.ShapeChooser(sc["budget"])
    res = fc.run_case(fc.HostRun(sc["cap"], 32, sc["budget"]), sc["frames"], choose)
    assert len(choose.frames) == 8 and choose.seen == {1, 2, 31, 32, 33, 35}, choose.frames
    assert max(r["n_live"] for r in res.values()) > 128 and max(fc.coverage(res)["wraps"]) > 0
