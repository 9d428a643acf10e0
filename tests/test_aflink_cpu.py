"""CPU: AFLink without a GPU (DESIGN.md section 4 "AFLink").  The packed weight vector and the per-column affine against the reference module's recorded float64
scores; the NumPy restatement of the linking procedure (tests/aflink_np.py) against every recorded scene; the host build of the device's candidate stage
(tests/_hostsim/aflink.py: gate, row-major compaction, pair transform of csrc/y7t_aflink.h) ARRAY-EQUAL to the restatement; the state-dict loader."""
import numpy as np
import pytest

from tests import aflink_np, aflink_scenes as sc


def test_fixture_set_holds_the_required_cases():
    g = sc.pairs_golden()
    assert g["x1"].shape == g["x2"].shape == (256, 30, 3) and g["x1"].dtype == np.float32
    assert float(g["E"]) == float(g["e_ref"]) > 0 and np.abs(g["scores32"].astype(np.float64) - g["scores64"]).max() == float(g["e_ref"])
    assert (g["scores64"] > 0.95).sum() >= 10 and (g["scores64"] < 0.05).sum() >= 10      # the recipe spreads the score
    scenes = sc.link_goldens()
    flags = {k: any(bool(s["flag_" + k]) for s in scenes.values()) for k in ("chain", "dup", "nocand", "compressed", "accepted", "rejected", "dropped_rows")}
    assert all(flags.values()), flags
    assert all(int(s["n_tracklets"]) <= 40 and s["rows_in"][:, 0].max() <= 120 for s in scenes.values())


def test_packed_blob_in_float64_meets_the_reference_module():
    """pins the packing order (state_dict() order without num_batches_tracked) and the per-column BatchNorms: a NumPy float64 walk of the packed vector lies within
    4 E of the reference module's own float64 scores (it differs from them by rounding order only: 1e-14 when recorded)"""
    g = sc.pairs_golden()
    got = aflink_np.forward_packed(sc.packed(), g["x1"], g["x2"])
    err = np.abs(got - g["scores64"]).max()
    print("restatement vs the reference's float64: %.3g   e_ref %.3g   bound 4 E = %.3g" % (err, float(g["e_ref"]), 4 * float(g["E"])))
    assert err <= 4 * float(g["E"])


def test_synth_forward_agrees_with_the_packed_walk():
    from yolov7_tracker_amd import synth
    g = sc.pairs_golden()
    lg = synth.aflink_forward_np(sc.weights(), g["x1"][:32], g["x2"][:32])
    s = 1.0 / (1.0 + np.exp(lg[:, 0] - lg[:, 1]))
    assert np.abs(s - g["scores64"][:32]).max() <= 4 * float(g["E"])


@pytest.mark.parametrize("name", sorted(sc.link_goldens()) or ["<no aflink_link_*.npz fixture>"])
def test_restatement_reproduces_the_recorded_scene(name):
    s = sc.link_goldens()[name]
    trace = {}
    out = aflink_np.link(s["rows_in"], lambda pairs, x1, x2: s["scores32"], tuple(s["thrT"]), float(s["thrS"]), float(s["thrP"]), trace=trace)
    assert np.array_equal(trace["pairs"], s["pairs"]) and np.array_equal(trace["links"], s["links"])
    assert np.array_equal(out, s["rows_out"])


def test_product_link_steps_equal_the_restatement_on_the_recorded_scenes():
    """tracker/aflink.py's host side (tracklet building, decisions, relabelling) from the recorded pairs and scores, without the device"""
    from yolov7_tracker_amd.tracker import aflink
    for name, s in sc.link_goldens().items():
        rows = s["rows_in"][np.argsort(s["rows_in"][:, 0], kind="stable")]
        ids, table, offsets = aflink.build_tracklets(rows)
        ids2, table2, offsets2 = aflink_np.tracklets(rows)
        assert ids == ids2 and np.array_equal(table, table2) and np.array_equal(offsets, offsets2)
        links = aflink.link_decisions(len(ids), s["pairs"], s["scores32"], float(s["thrP"]))
        assert np.array_equal(np.array(links, np.int32).reshape(-1, 2), s["links"]), name
        assert np.array_equal(aflink.relabel(rows, ids, links), s["rows_out"]), name


def _host_equals_restatement(table, offsets, thrT=(0, 30), thrS=75):
    from tests._hostsim import aflink as hs
    want_pairs, want_x1, want_x2 = aflink_np.candidates(table, offsets, thrT, thrS)
    got = hs.candidates(table, offsets, thrT, thrS, max_pairs=max(1, len(want_pairs)))
    assert got["count"] == len(want_pairs) and got["status"] == 0
    assert np.array_equal(got["pairs"], want_pairs)
    assert np.array_equal(got["x1"].view(np.uint32), want_x1.view(np.uint32)) and np.array_equal(got["x2"].view(np.uint32), want_x2.view(np.uint32))
    return len(want_pairs)


def test_host_build_of_the_candidate_stage_on_the_recorded_scenes():
    for name, s in sc.link_goldens().items():
        rows = s["rows_in"][np.argsort(s["rows_in"][:, 0], kind="stable")]
        _, table, offsets = aflink_np.tracklets(rows)
        assert _host_equals_restatement(table, offsets, tuple(s["thrT"]), float(s["thrS"])) == len(s["pairs"]), name


def test_host_build_of_the_candidate_stage_on_the_edge_geometries():
    counts = {name: _host_equals_restatement(t, o) for name, (t, o) in sc.geometry_tables().items()}
    assert counts["n1"] == 0 and counts["n2"] == 1 and counts["single_rows"] == 1 and counts["constant_column"] == 1
    assert counts["distance_edge"] >= 1 and counts["lengths"] >= 5 and counts["n65"] > 64 and counts["dense"] > 2048
    # a distance of exactly thrS passes, one ulp-scale step beyond does not
    t, o = sc.geometry_tables()["distance_edge"]
    pairs = aflink_np.candidates(t, o)[0].tolist()
    assert [0, 1] in pairs and [0, 2] not in pairs and [0, 3] in pairs


def test_host_build_reports_overflow_and_never_truncates_silently():
    from tests._hostsim import aflink as hs
    t, o = sc.geometry_tables()["n65"]
    want = aflink_np.candidates(t, o)[0]
    got = hs.candidates(t, o, max_pairs=len(want) - 1)
    assert got["count"] == len(want) and got["status"] == 1 and np.array_equal(got["pairs"], want[:-1])
    assert hs.candidates(t, o, max_pairs=len(want))["status"] == 0


def test_state_dict_loader_rejects_wrong_keys_and_shapes(tmp_path):
    import torch
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker import aflink
    w = {k: torch.from_numpy(v) for k, v in sc.weights().items()}
    good = dict(w)
    good["TemporalModule_1.0.bnf.num_batches_tracked"] = torch.tensor(0)      # the entries a real state dict carries besides
    torch.save({"module." + k: v for k, v in good.items()}, tmp_path / "ok.pth")
    got = aflink.load_aflink_weights(str(tmp_path / "ok.pth"))
    assert list(got) == [n for n, _ in synth.aflink_tensor_shapes()] and all(np.array_equal(got[k], sc.weights()[k]) for k in got)
    assert aflink.pack_aflink_weights(got).shape == (aflink_np.N_WEIGHTS,) and np.array_equal(aflink.pack_aflink_weights(got), sc.packed())
    missing = {k: v for k, v in w.items() if k != "FusionBlock_2.bn.bias"}
    torch.save(missing, tmp_path / "missing.pth")
    extra = dict(w, **{"classifier.fc3.weight": torch.zeros(2, 2)})
    torch.save(extra, tmp_path / "extra.pth")
    shape = dict(w, **{"TemporalModule_2.1.conv.weight": torch.zeros(64, 32, 1, 7)})
    torch.save(shape, tmp_path / "shape.pth")
    torch.save([1, 2, 3], tmp_path / "list.pth")
    for bad in ("missing.pth", "extra.pth", "shape.pth", "list.pth"):
        with pytest.raises(ValueError):
            aflink.load_aflink_weights(str(tmp_path / bad))
    for bad in ("random:dhn", "random:aflink:1:2:3"):
        with pytest.raises(ValueError):
            aflink.load_aflink_weights(bad)
    assert np.array_equal(aflink.load_aflink_weights("random:aflink:3:1.5")["classifier.fc2.bias"], sc.weights()["classifier.fc2.bias"])
