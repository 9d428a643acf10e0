"""The scenes of tests/post_scenes.py meet their stated conditions under the CPU oracle alone (oracle/cnative.nms, oracle/detector_torch), so that no case of
tests/test_postprocess_gpu.py can pass vacuously: the cut really binds, the chain really separates the greedy walk from the wrong rule, the IoU really sits on the
threshold, no score sits in the band around conf_thres, ..."""
import numpy as np
import pytest

from tests import post_scenes as ps


def _ranks(scene):
    order = np.lexsort((scene["rows"], -scene["score"].astype(np.float64)))
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank


def test_reference_walk_is_nms_rows():
    """the walk is oracle.detector_torch.nms_rows restated on arrays: same kept anchor rows, in order, with and without the cuts binding"""
    from oracle import detector_torch as dt
    for s, kw in ((ps.clustered(1000, seed=1000), {}), (ps.separated(), {}), (ps.clustered(600, seed=600), {"max_nms": 100}), (ps.separated(), {"max_det": 65}),
                  (ps.ties(), {}), (ps.class_offsets(), {"iou_thres": 0.65})):
        cands = {int(r): (b, float(sc), int(c)) for r, b, sc, c in zip(s["rows"], s["box"], s["score"], s["cls"])}
        np.testing.assert_array_equal(s["rows"][ps.reference_walk(s, **kw)], dt.nms_rows(cands, **kw))
    assert len(ps.reference_walk(ps.clustered(0, seed=0))) == 0


def test_layout_matches_the_detectors_view_of_it():
    """ws_layout restates Detector.candidate_arrays' offsets (yolov7_tracker_amd/detector/model.py) and packs what unpack reads"""
    for B, cap in ((1, 64), (3, 1000), (16, 1024)):
        lay = ps.ws_layout(B, cap)
        rup = lambda n: (n + 255) // 256 * 256
        o1 = rup(B * cap * 16); o2 = o1 + rup(B * cap * 4); o3 = o2 + rup(B * cap * 4); o4 = o3 + rup(B * cap * 4)
        assert [lay[k][0] for k in ("cbox", "cscore", "ccls", "cidx", "count")] == [0, o1, o2, o3, o4]
        assert all(lay[k][0] % 256 == 0 for k in lay if k != "total") and lay["total"] == lay["lb"][0] + rup(B * 20) + 256
    scenes = [ps.clustered(n, seed=n) for n in (5, 0, 64)]
    buf = ps.pack_candidates(scenes, 64)
    cbox, cscore, ccls, cidx, count = ps.unpack_candidates(buf, 3, 64)
    assert count.tolist() == [5, 0, 64]
    for b, s in enumerate(scenes):
        n = len(s["score"])
        assert np.array_equal(cbox[b, :n], s["box"]) and np.array_equal(cscore[b, :n], s["score"]) and np.array_equal(ccls[b, :n], s["cls"]) and np.array_equal(cidx[b, :n], s["rows"])
        assert (cidx[b, n:] < 0).all() and not (cscore[b, n:] > 0).any()          # the sentinel is nothing a kernel could take for a candidate


def test_slot_order_is_not_row_order_and_scores_are_distinct():
    for s in (ps.clustered(1000, seed=1000), ps.separated(), ps.chain(), ps.tight_cluster(), ps.duplicates(), ps.class_offsets(), ps.rescale_scene()):
        assert len(np.unique(s["score"])) == len(s["score"])
        assert (np.diff(s["rows"]) < 0).sum() > len(s["rows"]) // 4
        r = _ranks(s)
        assert (np.diff(r) < 0).sum() > len(r) // 4                                # ... nor score order


def test_boundary_scenes():
    """case 1: at every count the walk is non-trivial -- from n = 63 on it both keeps and suppresses inside the first wave; the large scenes keep boxes in the chunks behind the first"""
    for n in ps.BOUNDARY_COUNTS:
        s = ps.clustered(n, seed=n)
        assert len(s["score"]) == n
        k = ps.reference_walk(s)
        assert len(k) == min(n, 2) if n <= 2 else 20 <= len(k) < min(n, 300)
    s = ps.clustered(1000, seed=1000)
    rk = _ranks(s)[ps.reference_walk(s)]
    assert 40 <= len(rk) <= 70 and 20 <= (rk < 64).sum() < 64 and (rk >= 256).sum() >= 3
    for a, b in ((300, 301), (300, 302)):                                           # case 2's images differ from each other
        assert not np.array_equal(ps.clustered(300, seed=a)["box"], ps.clustered(300, seed=b)["box"])


def test_max_det_scene():
    """case 3: >= 400 survive with the cut lifted; the cuts at 63 / 64 / 65 and at 300 do not fall on the first max_det of the sorted list (something in front is suppressed)
    and the cut at 300 falls behind the first 256-chunk"""
    s = ps.separated()
    k = ps.reference_walk(s, max_det=10 ** 9)
    assert 400 <= len(k) < 1000
    rk = _ranks(s)[k]
    assert rk[62] > 62 and rk[299] > 320 and (np.diff(rk) > 0).all()
    for m in (1, 2, 63, 64, 65, 300):
        np.testing.assert_array_equal(ps.reference_walk(s, max_det=m), k[:m])


def test_max_nms_scene():
    """case 4: every cut changes the keep list, and the cut is by rank -- the kept boxes are among the max_nms best"""
    s = ps.clustered(600, seed=600)
    full = ps.reference_walk(s)
    lens = [len(ps.reference_walk(s, max_nms=m)) for m in (64, 100, 257)]
    assert lens[0] < lens[1] < lens[2] < len(full) < 300
    for m in (64, 100, 257):
        assert _ranks(s)[ps.reference_walk(s, max_nms=m)].max() < m
    assert 20 <= len(ps.reference_walk(ps.prefix(s, 64))) < 64                      # cap = 64: the first 64 SLOTS, another set than the 64 best


@pytest.mark.parametrize("order,kept", [("descending", 150), ("ascending", 150), ("permuted", None)])
def test_chain_scene(order, kept):
    """case 5: neighbours at IoU exactly 0.5; the greedy walk keeps every second box of a run, the wrong rule (any better box suppresses) far fewer"""
    s = ps.chain(order)
    k = ps.reference_walk(s)
    wrong = ps.suppressed_by_any_better_box(s)
    if kept is not None:
        assert len(k) == kept and wrong == 1
    else:
        assert 100 <= len(k) <= 150 and wrong <= len(k) - 20
    x = np.sort(s["box"][:, 0])
    assert np.array_equal(x, 10.0 * np.arange(300))
    assert ps.suppressed_by_any_better_box(ps.separated()) < len(ps.reference_walk(ps.separated(), max_det=10 ** 9))


def test_cluster_tie_and_duplicate_scenes():
    """case 6"""
    assert len(ps.tight_cluster()["score"]) == 512 and len(ps.reference_walk(ps.tight_cluster())) == 1
    s = ps.ties()
    u, cnt = np.unique(s["score"], return_counts=True)
    assert (cnt == 8).all() and len(u) == 40
    k = ps.reference_walk(s)
    assert len(k) == 300 and len(ps.reference_walk(s, max_det=10 ** 9)) == 320     # nothing is suppressed; the cut falls inside a group (300 = 37 x 8 + 4)
    sc, rows = s["score"][k], s["rows"][k]
    assert (np.diff(sc) <= 0).all() and all((np.diff(rows[sc == v]) > 0).all() for v in u)
    assert any((np.diff(k[sc == v]) < 0).any() for v in u)                          # ... which is not slot order
    d = ps.duplicates()
    assert len(ps.reference_walk(d)) == 8 and len(ps.reference_walk(d, 1.0)) == 64
    assert len(np.unique(d["box"], axis=0)) == 8


def test_threshold_scenes():
    """case 7"""
    s = ps.clustered(1000, seed=1000)
    n = [len(ps.reference_walk(s, t, max_det=10 ** 9)) for t in (0.0, 0.45, 0.65, 1.0)]
    assert n[0] < n[1] < n[2] < n[3] == 1000
    t = ps.touching()
    assert ps.reference_walk(t, 0.0).tolist() == [0, 1, 3] and ps.reference_walk(t, 0.45).tolist() == [0, 1, 2, 3]
    h = ps.exact_half()
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert below < np.float32(0.5)
    assert ps.reference_walk(h, 0.5).tolist() == [0, 1] and ps.reference_walk(h, below).tolist() == [0]


def test_class_offset_scene():
    """case 8"""
    s = ps.class_offsets()
    off = (s["box"] + s["cls"][:, None] * ps.MAX_WH).astype(np.float32)
    exact = s["box"].astype(np.float64) + s["cls"][:, None].astype(np.float64) * 4096.0
    assert (off.max(1) > 2 ** 18).sum() > 50 and (off != exact).sum() > 100          # the class-offset sum is rounded
    k = set(ps.reference_walk(s).tolist())
    same = np.nonzero((s["box"] == np.array([300.3, 200.7, 380.1, 290.9], np.float32)).all(1))[0]
    assert len(same) == 12 and len(set(s["cls"][same].tolist())) == 12 and set(same.tolist()) <= k
    area = (s["box"][:, 2] - s["box"][:, 0]) * (s["box"][:, 3] - s["box"][:, 1])
    assert (area == 0).sum() == 1 and (s["box"][:, 2] - s["box"][:, 0] > 4000).sum() == 1
    assert 50 < len(k) < 300 and len(k) < len(s["score"]) - 100                      # and the NMS has work to do
    assert s["cls"].max() == 79


def test_rescale_scene():
    """case 10: everything is kept (the rows of every special box are in the output); half-way coordinates exist under each exact letterbox"""
    s = ps.rescale_scene()
    k = ps.reference_walk(s)
    assert len(k) == len(s["score"]) < 300
    for lb in ((2.0, 0.0, 0.0, 128.0, 160.0), (1.0, 0.0, 28.0, 200.0, 320.0), (1.0, 0.0, 0.0, 1280.0, 1280.0)):
        gain, padw, padh, H0, W0 = (np.float32(v) for v in lb)
        x = (s["box"][:, 0] - padw) / gain
        y = (s["box"][:, 1] - padh) / gain
        inside = (x > 0) & (x < W0) & (y > 0) & (y < H0)
        half = (x[inside] % 1 == 0.5)
        assert half.sum() >= 4 and (np.floor(x[inside][half]) % 2 == 0).any() and (np.floor(x[inside][half]) % 2 == 1).any()      # ties towards both neighbours
        rows = ps.expected_rows(s, k, lb)
        assert rows[:, :4].min() == 0 and rows[:, 0].max() <= W0 and rows[:, 2].max() == W0 and rows[:, 3].max() == H0
    b = s["box"]
    assert (b[:, 0] < 0).any() and (b[:, 1] < 0).any() and (b[:, 2] > 1280).any() and (b[:, 3] > 1280).any()


def test_expected_rows_is_scale_coords_round():
    """the float32 expression of expected_rows equals oracle.detector_torch.scale_coords_round bit for bit where the letterbox parameters are exact in float32"""
    import torch
    from oracle import detector_torch as dt
    s = ps.rescale_scene()
    k = np.arange(len(s["score"]))
    for img1, img0, lb in (((256, 320), (128, 160), (2.0, 0.0, 0.0, 128.0, 160.0)), ((256, 320), (200, 320), (1.0, 0.0, 28.0, 200.0, 320.0))):
        want = dt.scale_coords_round(img1, torch.from_numpy(s["box"].copy()), img0).numpy()
        assert np.array_equal(ps.expected_rows(s, k, lb)[:, :4], want)


@pytest.mark.parametrize("gi", range(len(ps.GRIDS)))
@pytest.mark.parametrize("conf", [0.01, 0.25])
def test_decode_scenes(gi, conf):
    """no float64 objectness / confidence within BAND of conf_thres, so the oracle's float32 filter and the float64 one agree on EVERY row; about a third of the rows pass"""
    sc = ps.decode_scene(gi, conf)
    nl, na, no, shapes, B = ps.GRIDS[gi]
    assert [h.shape for h in sc["heads"]] == [(B, ny, nx, na * no) for ny, nx in shapes] and all(h.dtype == np.float32 for h in sc["heads"])
    assert (sc["strides"] > 0).all() and (sc["anchors"] > 0).all()
    ref = ps.decode_reference(sc, conf)
    passing = [set() for _ in range(B)]
    row0 = 0
    for (obj, cf), (ny, nx) in zip(ps.scores64(sc["heads"], na, no), shapes):
        assert np.abs(obj - conf).min() >= ps.BAND and np.abs(cf - conf).min() >= ps.BAND
        for b, y, x, a in zip(*np.nonzero((obj > conf) & (cf > conf))):
            passing[b].add(row0 + (a * ny + y) * nx + x)                          # the reference's row order: level, anchor, y, x
        row0 += na * ny * nx
    assert row0 == sc["A"]
    assert [set(r) for r in ref] == passing
    total = sum(len(r) for r in ref)
    if sc["A"] * B >= 30:
        assert 0.25 * sc["A"] * B <= total <= 0.45 * sc["A"] * B and all(0 < len(r) < sc["A"] for r in ref)
    else:
        assert total == (1 if conf == 0.01 else 0)                                 # the 1 x 1 grid: one candidate, and the image without any


def test_decode_overflow_scene():
    sc = ps.decode_scene(2, 0.01, obj_logit=6.0)
    assert sc["A"] == 324 and [len(r) for r in ps.decode_reference(sc, 0.01)] == [324, 324]
