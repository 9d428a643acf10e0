"""DeepSORT's three appearance launches on the MI355X, alone: k_ds_normalize (detn), k_embed_dist (app, cmin / cmax) and k_ds_store (ring, nfeat, fpos), read out of
the feature blob before and after a frame driven through the DeepSORT class, against the host build's bits and a float64 reference of the device's own stored rows
(tests/deepsort_feat_case.py: the check, its derived bounds and the scenes; tests/test_deepsort_feat_cpu.py runs the same check on the host build and pins the host
build's norms to numpy's recorded bits).  The rings are 3 or 35 deep (STORE_FEATURES_BUDGET patched), so that they wrap within a few frames; ring, detn and app start
as NaN.  Every case prints one MARGIN line (worst error / bound per kernel): profiles/deepsort_feat_margins.txt keeps the listing of one run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import tracker_np  # noqa: E402
from tests import deepsort_feat_case as fc  # noqa: E402
from tests import tracker_case as tc  # noqa: E402
from tests import util  # noqa: E402
from yolov7_tracker_amd.tracker import deepsort as ds  # noqa: E402


class DeviceRun:
    """a DeepSORT tracker of the product with `budget`-deep rings, its two blobs readable (fc.run_case drives it)"""

    def __init__(self, monkeypatch, cap, dim, budget):
        monkeypatch.setattr(ds, "STORE_FEATURES_BUDGET", budget)      # read when the feature state is sized and initialised
        self.cap, self.dim, self.budget = cap, dim, budget
        self._feats = None
        self.t = tc.new_tracker(ds.DeepSORT, feature_fn=lambda tlbrs: self._feats, max_tracks=cap, max_dets=cap)
        self.t._ensure_feature_state(dim)
        self.lay = fc.feat_layout(cap, cap, dim, budget)
        assert self.lay["total"] == int(self.t._L.y7t_deepsort_feature_bytes(cap, cap, dim, budget)) == self.t._feat.numel()
        for off, cnt in fc.poison_ranges(self.lay):
            self.t._feat[off:off + 4 * cnt].view(torch.float32).fill_(float("nan"))

    def blobs(self):
        torch.cuda.synchronize()
        return fc.read_pool(self.t._state.cpu().numpy(), self.cap, self.cap), fc.read_feat(self.t._feat.cpu().numpy(), self.lay)

    def step(self, dets, feats):
        self._feats = feats
        return self.t.update(dets, None)


@pytest.mark.parametrize("dim", fc.WIDTHS)
def test_three_launches_at_every_width(dim, monkeypatch):
    """9 objects in three groups of look-alikes, pool 64 / 64, budget 3, 8 frames, every frame checked: the wave forms at 1 / 2 / 4 / 8 blocks of 128, the tiled
    distance with serial norms (32, 64, 96, 160) and the plain forms (100, 7).  The scene must hold detections whose candidates have two ages, one age and none, a
    distance above 1 (an unmasked zero row would win the minimum) and rings that wrap twice"""
    sc = fc.widths_scene(dim)
    run = DeviceRun(monkeypatch, sc["cap"], dim, sc["budget"])
    res = fc.run_case(run, sc["frames"])
    print("\n" + fc.margin_line("widths dim %d" % dim, res))
    cov = fc.coverage(res)
    assert len(res) == 8 and cov["mixed"] > 0 and cov["one_age"] > 0 and cov["none"] > 0 and cov["max_app"] > 1.0 and max(cov["wraps"]) >= 2 and sum(w > 0 for w in cov["wraps"]) >= 9, cov


@pytest.mark.parametrize("dim", [128, 100])
def test_three_launches_at_130_slots_and_rows(dim, monkeypatch):
    """pool 512 / 512 (two ballot rounds), 130 tracks born in the first frame + a frame's unconfirmed ones (more live slots than the 128 workers: workgroups own two
    slots), 130 rows per frame (three detection tiles, the last 2 wide), budget 35, counts that differ between the slots of a frame; checked where the fullest ring
    holds 1, 2, 31, 32, 33 and 35 rows, on the first frame after a wrap and the third after it.  dim 100: the plain form walks its owned slots too"""
    sc = fc.shape_scene(dim)
    run = DeviceRun(monkeypatch, sc["cap"], dim, sc["budget"])
    choose = fc.ShapeChooser(sc["budget"])
    res = fc.run_case(run, sc["frames"], choose)
    print("\n" + fc.margin_line("shape dim %d, frames %s" % (dim, choose.frames), res))
    assert len(choose.frames) == 8 and choose.seen == {1, 2, 31, 32, 33, 35}, choose.frames
    assert all(len(d) == 130 for d, _ in sc["frames"]) and max(r["n_live"] for r in res.values()) > 128 and max(fc.coverage(res)["wraps"]) > 0


@pytest.mark.parametrize("budget", [3, 35, 100])
def test_device_deepsort_equals_oracle_across_a_wrap(budget, monkeypatch):
    """the whole tracker with wrapped rings (lost tracks re-found against a full ring): ids and boxes of every frame equal to the oracle with the same budget;
    100 is the product's own, unpatched"""
    if budget != 100:
        monkeypatch.setattr(ds, "STORE_FEATURES_BUDGET", budget)
    assert ds.STORE_FEATURES_BUDGET == budget
    sc = fc.wrap_scene(budget)
    t = tc.new_tracker(ds.DeepSORT, feature_fn=sc["feature_fn"], max_tracks=256, max_dets=256)
    got = [[(v.track_id, np.asarray(v.tlwh, np.float64), float(v.cls), float(v.score)) for v in t.update(d, None)] for d in sc["dets"]]
    assert t._feat_dim == sc["dim"] and int(t._feat[8:12].view(torch.int32).item()) == budget      # Y7TFeatHdr.budget
    want = tracker_np.run("deepsort", sc["dets"], feature_fn=sc["feature_fn"], dot=tracker_np.dot_sequential, feature_budget=budget)
    util.assert_same_tracks(got, want, "budget %d" % budget)
