"""CPU: the YOLOv7 family beyond w6 / tiny -- yolov7, yolov7x, yolov7-e6, -d6, -e6e (RepConv, DownC, Shortcut): the generators, the lowering of nested concats and
adds, the RepConv fold, and the walk of tests/family_ref.py against the live reference Model and against goldens recorded from it
(tests/golden/make_golden_family.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import family_ref as fr
from tests import util
from yolov7_tracker_amd.detector import arch, graph, model, weights

REF = "/root/reference"


def _lower(name, hw, nc=80, max_batch=2):
    return graph.lower(graph.parse(arch.ARCHS[name](nc))[0], hw[0], hw[1], max_batch)


# ------------------------------------------------------------------------------------------------ 1. specs
def test_generators_equal_reference_yaml(have_reference):
    if not have_reference:
        pytest.skip("/root/reference not present")
    import yaml
    norm = lambda L: [str(x).replace("'None'", "None") for x in L]
    for name in fr.FAMILY:
        y = yaml.safe_load(open("%s/cfg/deploy/%s.yaml" % (REF, name)))
        spec = arch.ARCHS[name](y["nc"])
        assert norm(y["backbone"] + y["head"]) == norm(spec["layers"]), name
        assert y["anchors"] == spec["anchors"] and spec["n_backbone"] == len(y["backbone"]), name


def test_training_yamls_lower(have_reference):
    """IDetect (yolov7, yolov7x) and IAuxDetect + aux convs (e6, d6, e6e): the dead aux branch is dropped, the plan is the deploy graph's"""
    if not have_reference:
        pytest.skip("/root/reference not present")
    for name in fr.FAMILY:
        spec = arch.load_yaml("%s/cfg/training/%s.yaml" % (REF, name), nc=2)
        hw = fr.small_hw(name)
        p = graph.lower(graph.parse(spec)[0], hw[0], hw[1], 2)
        q = _lower(name, hw, 2)
        assert p.det["kind"] == ("IAuxDetect" if name in fr.P6 else "IDetect")
        assert np.array_equal(p.ops, q.ops) and len(p.heads) == len(q.heads), name


# ------------------------------------------------------------------------------------------------ 2. census
def _census(p):
    t = p.ops["type"]
    return dict(conv=int((t == 0).sum()), up=int((t == 1).sum()), pool=int(((t == 2) & (p.ops["KH"] > 1)).sum()), copy=int(((t == 2) & (p.ops["KH"] == 1)).sum()),
                add=int((t == 3).sum()), rep=sum(1 for w in p.wlayout if w.get("rep")),
                downc=sum(1 for w in p.wlayout for k in (w["wkey"] if isinstance(w["wkey"], tuple) else (w["wkey"],)) if k.rsplit(".", 1)[-1] in ("cv1", "cv2", "cv3")
                          and not any(k.startswith(s7 + ".") for s7 in p.sppcspc)))


def plan_census(name, hw, max_batch=2, nc=80):
    nodes, _ = graph.parse(arch.ARCHS[name](nc))
    p = graph.lower(nodes, hw[0], hw[1], max_batch)
    p.sppcspc = {w["wkey"].rsplit(".", 1)[0] for w in p.wlayout if isinstance(w["wkey"], str) and w["wkey"].endswith(".cv7")}
    c = _census(p)
    c["downc_pool"] = int(((p.ops["type"] == 2) & (p.ops["KH"] == 2) & (p.ops["stride"] == 2)).sum()) if name in fr.P6 else 0
    return c


@pytest.mark.parametrize("name", fr.FAMILY)
def test_census(name):
    for hw in (fr.small_hw(name), fr.nominal_hw(name)):
        c = plan_census(name, hw, 8)
        assert c["add"] == (11 if name == "yolov7-e6e" else 0)
        assert c["rep"] == (3 if name == "yolov7" else 0)
        assert c["copy"] == 0                                         # no tensor of these graphs needs a second home
        if name in fr.P6:                                             # 8 DownC per graph: 8 pools (2, 2, 0) and 24 convs
            assert c["downc_pool"] == 8 and c["downc"] == 24
        else:
            assert c["downc"] == 0 and c["pool"] == 5 + 3             # MP x 5, the SPPCSPC cascade


def test_repconv_parses_to_a_marked_3x3():
    nodes, layer_out = graph.parse(arch.yolov7(2))
    for i in (102, 103, 104):
        n = nodes[layer_out[i]]
        assert (n.kind, n.k, n.s, n.p, n.act, n.wkey) == ("conv", 3, 1, 1, 1, "model.%d" % i) and n.extra["rep"]
    p = graph.lower(nodes, 96, 160, 1)
    assert [w["wkey"] for w in p.wlayout if w.get("rep")] == ["model.102", "model.103", "model.104"]


def test_parse_still_refuses_unknown_modules():
    spec = arch.yolov7_tiny(2)
    spec["layers"][3] = [-1, 1, "Foldcut", []]
    with pytest.raises(NotImplementedError):
        graph.parse(spec)


# ------------------------------------------------------------------------------------------------ 3. plan soundness
def _check_plan(name, hw):
    nodes, _ = graph.parse(arch.ARCHS[name](2))
    p = graph.lower(nodes, hw[0], hw[1], 2)
    npix = {}                                   # buffer -> pixels per image, from the buffer table
    writers = {}                                # buffer -> [(c0, c1)]
    for op in p.ops:
        o = {k: int(op[k]) for k in op.dtype.names}
        isz_out = 4 if o["out_f32"] else 2
        assert o["in_coff"] >= 0 and o["in_coff"] + o["Cin"] <= o["in_ld"], "input slice leaves its buffer"
        assert o["H"] * o["W"] * o["in_ld"] <= p.buf_elems[o["in_buf"]][0]
        assert o["out_coff"] >= 0 and o["out_coff"] + o["Cout"] <= o["out_ld"], "output slice leaves its buffer"
        assert o["Ho"] * o["Wo"] * o["out_ld"] <= p.buf_elems[o["out_buf"]][0] and p.buf_elems[o["out_buf"]][1] == isz_out
        if o["up_C"] > 0 or o["type"] == 3:
            hh, ww = (o["H"], o["W"]) if o["type"] == 3 else (o["H"] // 2, o["W"] // 2)
            cc = o["Cin"] if o["type"] == 3 else o["up_C"]
            assert o["up_coff"] >= 0 and o["up_coff"] + cc <= o["up_ld"] and hh * ww * o["up_ld"] <= p.buf_elems[o["up_buf"]][0]
        if o["type"] == 3:                       # both operands and the output of an add have one shape; the output overlaps neither
            assert (o["Ho"], o["Wo"], o["Cout"]) == (o["H"], o["W"], o["Cin"])
            assert o["H"] * o["W"] * o["in_ld"] == p.buf_elems[o["in_buf"]][0] and o["H"] * o["W"] * o["up_ld"] == p.buf_elems[o["up_buf"]][0]
            assert o["Ho"] * o["Wo"] * o["out_ld"] == p.buf_elems[o["out_buf"]][0]
            for buf, coff in ((o["in_buf"], o["in_coff"]), (o["up_buf"], o["up_coff"])):
                assert buf != o["out_buf"] or coff + o["Cin"] <= o["out_coff"] or o["out_coff"] + o["Cout"] <= coff
            assert o["Cin"] % 8 == 0 and all(o[k] % 8 == 0 for k in ("in_ld", "in_coff", "up_ld", "up_coff", "out_ld", "out_coff"))
        writers.setdefault(o["out_buf"], []).append((o["out_coff"], o["out_coff"] + o["Cout"]))
        npix[o["out_buf"]] = o["Ho"] * o["Wo"]
    # channels that exist only at half resolution (upsample-on-read) are written by nobody at this resolution: the readers fetch them from up_buf
    virtual = {}
    for op in p.ops:
        if int(op["type"]) == 0 and int(op["up_C"]) > 0:
            virtual.setdefault(int(op["in_buf"]), set()).add((int(op["in_coff"]) + int(op["up_c0"]), int(op["in_coff"]) + int(op["up_c0"]) + int(op["up_C"])))
    live = {n.home for n in p.nodes if n.kind == "concat" and n.home is not None and any(int(op["in_buf"]) == n.home or int(op["up_buf"]) == n.home for op in p.ops)}
    assert live
    for buf in live:
        ld = p.buf_elems[buf][0] // npix[buf]
        cover = np.zeros(ld, np.int64)
        for c0, c1 in writers.get(buf, []) + sorted(virtual.get(buf, ())):
            cover[c0:c1] += 1
        assert (cover == 1).all(), "%s %s: buffer %d channels written %s times" % (name, hw, buf, sorted(set(cover.tolist())))
    # every nested concat is a channel range of its outer buffer
    for n in p.nodes:
        if n.kind == "concat" and n.home is not None:
            off = n.coff
            for j in n.src:
                t = p.nodes[j]
                if t.virtual:
                    off += t.c
                    continue
                assert (t.home, t.coff, t.ld) == (n.home, off, n.ld), "%s: node %d is not at its place in concat %d" % (name, j, n.idx)
                off += t.c
    return p


@pytest.mark.parametrize("name", fr.FAMILY)
def test_plan_soundness(name):
    for hw in (fr.small_hw(name), fr.nominal_hw(name)):
        _check_plan(name, hw)


def test_nested_concat_is_a_slice_of_the_outer_buffer():
    """e6 layer 100 (DownC) + 101 (Concat with layer 85): DownC's two convs write channels [0, 160) and [160, 320) of the 640-channel buffer of layer 101"""
    nodes, layer_out = graph.parse(arch.yolov7_e6(2))
    p = graph.lower(nodes, 192, 320, 2)
    inner, outer = nodes[layer_out[100]], nodes[layer_out[101]]
    assert inner.kind == outer.kind == "concat" and (inner.home, inner.coff, inner.ld) == (outer.home, 0, 640)
    a, b = (nodes[j] for j in inner.src)
    assert (a.home, a.coff, a.ld, b.home, b.coff, b.ld) == (outer.home, 0, 640, outer.home, 160, 640)
    assert (nodes[layer_out[85]].home, nodes[layer_out[85]].coff) == (outer.home, 320)


def test_a_concat_in_two_outer_concats_is_copied_into_the_second():
    """synthetic: DownC's concat feeds two Concats -> one home (the first), one k = 1 copy into the second"""
    L = [[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "DownC", [32]], [-2, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [32, 1, 1]],
         [[-3, -1], 1, "Concat", [1]], [[-3, -4], 1, "Concat", [1]], [-2, 1, "Conv", [32, 3, 1]], [-2, 1, "Conv", [32, 3, 1]], [-1, 1, "Conv", [32, 3, 2]],
         [[6, 7, 8], 1, "Detect", ["nc", "anchors"]]]
    spec = {"nc": 2, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": arch.P5_ANCHORS, "layers": L}
    nodes, layer_out = graph.parse(spec)
    p = graph.lower(nodes, 64, 64, 1)
    inner, first, second = nodes[layer_out[1]], nodes[layer_out[4]], nodes[layer_out[5]]
    assert (inner.home, inner.coff, inner.ld) == (first.home, 0, 64)
    copies = [op for op in p.ops if int(op["type"]) == 2 and int(op["KH"]) == 1]
    assert len(copies) == 1
    c = copies[0]
    assert (int(c["in_buf"]), int(c["in_coff"]), int(c["Cin"]), int(c["out_buf"]), int(c["out_coff"]), int(c["out_ld"])) == (first.home, 0, 32, second.home, 16, 48)


def test_add_may_live_in_a_concat_and_read_slices():
    """e6e layers 189 / 212: the Concat reads a Shortcut (162 / 137) -> the add writes into the concat buffer"""
    nodes, layer_out = graph.parse(arch.yolov7_e6e(2))
    p = graph.lower(nodes, 192, 320, 2)
    for cat, sc in ((189, 162), (212, 137)):
        c, a = nodes[layer_out[cat]], nodes[layer_out[sc]]
        assert a.kind == "add" and a.home == c.home and a.ld == c.ld and a.coff == c.c - a.c


# ------------------------------------------------------------------------------------------------ 4. RepConv fold
def _repconv_sd(g, tag, key="model.7"):
    pre = tag + "_in."
    return {key + "." + k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


@pytest.mark.parametrize("tag,identity", [("a", False), ("b", True)])
def test_repconv_fold_equals_reference_fuse(tag, identity, have_reference):
    g = np.load(os.path.join(util.GOLDEN, "family_repconv.npz"))
    sd = _repconv_sd(g, tag)
    assert ("model.7.rbr_identity.weight" in sd) == identity
    W, b = weights.folded(dict(wkey="model.7", kind="conv", rep=True), sd)
    np.testing.assert_allclose(W, g[tag + "_fused_weight"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(b, g[tag + "_fused_bias"], rtol=1e-5, atol=1e-6)
    # the deploy form of the same layer folds to the same weights
    dep = {"model.7.rbr_reparam.weight": torch.from_numpy(g[tag + "_fused_weight"]), "model.7.rbr_reparam.bias": torch.from_numpy(g[tag + "_fused_bias"])}
    W2, b2 = weights.folded(dict(wkey="model.7", kind="conv", rep=True), dep)
    np.testing.assert_allclose(W, W2, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(b, b2, rtol=1e-5, atol=1e-6)
    if have_reference:      # ... and the golden is what the live reference makes of these tensors
        from oracle import ref_harness
        ns = ref_harness.load_detector()
        c2, c1 = g[tag + "_in.rbr_dense.0.weight"].shape[:2]
        m = ns.common.RepConv(c1, c2, 3, 1).eval()
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eps = 1e-3
        m.load_state_dict({k[len("model.7."):]: v for k, v in sd.items()}, strict=False)
        m.fuse_repvgg_block()
        assert np.array_equal(m.rbr_reparam.weight.detach().numpy(), g[tag + "_fused_weight"]) and np.array_equal(m.rbr_reparam.bias.detach().numpy(), g[tag + "_fused_bias"])


def test_seeded_repconv_training_and_deploy_forms_pack_alike():
    """random_state_dict draws the training form (dense, 1x1, identity where cin == cout); its `fused` form is the deploy form of the same layers"""
    wl = [dict(wkey="model.3", kind="conv", rep=True, cin=32, cout=32, k=3, act=1), dict(wkey="model.4", kind="conv", rep=True, cin=32, cout=48, k=3, act=1)]
    tr, dp = weights.random_state_dict(wl, 5, bn_bias_mean=2.0), weights.random_state_dict(wl, 5, fused=True, bn_bias_mean=2.0)
    assert "model.3.rbr_identity.weight" in tr and "model.4.rbr_identity.weight" not in tr and "model.4.rbr_1x1.1.running_var" in tr
    assert sorted(dp) == ["model.3.rbr_reparam.bias", "model.3.rbr_reparam.weight", "model.4.rbr_reparam.bias", "model.4.rbr_reparam.weight"]
    for w in wl:
        (W, b), (W2, b2) = weights.folded(w, tr), weights.folded(w, dp)
        np.testing.assert_allclose(W, W2, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(b, b2, rtol=1e-5, atol=1e-6)
    # the fold is the layer: act(conv(x, W', b')) == the reference's three-branch forward, float64
    x = torch.randn((1, 32, 5, 6), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for w in wl:
        W, b = weights.folded(w, tr)
        got = torch.nn.functional.silu(torch.nn.functional.conv2d(x, torch.from_numpy(W), torch.from_numpy(b), padding=1))
        assert float((got - fr.repconv(x, tr, w["wkey"], 1, 1, torch.float64)).abs().max()) < 1e-12


def test_load_checkpoint_takes_both_repconv_forms(tmp_path):
    spec, nodes, plan, sd = fr.seeded("yolov7")
    dep = dict(sd)
    for w in plan.wlayout:
        if w.get("rep"):
            W, b = weights.folded(w, sd)
            for k in [k for k in dep if k.startswith(w["wkey"] + ".rbr_")]:
                del dep[k]
            dep[w["wkey"] + ".rbr_reparam.weight"], dep[w["wkey"] + ".rbr_reparam.bias"] = torch.from_numpy(W).float(), torch.from_numpy(b).float()
    blobs = []
    for tag, d in (("training", sd), ("deploy", dep)):
        torch.save({"model": d}, str(tmp_path / (tag + ".pt")))
        spec2, sd2, _ = model.load_checkpoint(str(tmp_path / (tag + ".pt")), cfg="yolov7", nc=2)
        assert spec2["layers"] == spec["layers"]
        blobs.append(weights.pack(plan.wlayout, sd2, plan.w_elems, plan.b_elems))
    assert np.abs(blobs[0][0].astype(np.float32) - blobs[1][0].astype(np.float32)).max() <= 2.0 ** -10 * np.abs(blobs[0][0].astype(np.float32)).max()      # (the deploy form went through fp32: an fp16 ulp)
    np.testing.assert_allclose(blobs[0][1], blobs[1][1], rtol=1e-5, atol=1e-6)
    assert model.load_checkpoint("random:yolov7-e6e:3", nc=2)[0]["layers"] == arch.yolov7_e6e(2)["layers"]


# ------------------------------------------------------------------------------------------------ 5. / 6. the walk against the reference
def _bar(name, dec, want, fuse_dev):
    """x / e6 / d6 / e6e: the standard of test_oracle_equals_live_reference_model (torch.equal).  yolov7: the reference after its own .fuse() re-parameterises the
    RepConvs, the walk evaluates three branches -- two fp32 roundings of one algebra: allowed 4 x the largest absolute difference between the reference's OWN fused
    and unfused outputs on this input (`fuse_dev`)"""
    if name == "yolov7":
        d = float((dec - want).abs().max())
        print("FAMILY %s: walk vs fused reference max |d| %.6g, the reference's fused vs unfused %.6g (bar 4 x)" % (name, d, fuse_dev))
        assert d <= 4 * fuse_dev
    else:
        assert torch.equal(dec, want), "%s: max |d| %.3g" % (name, float((dec - want).abs().max()))


_walks = {}


def _walk(name):
    if name not in _walks:
        spec, nodes, plan, sd = fr.seeded(name)
        _walks[name] = fr.forward(nodes, sd, fr.golden_image(name), spec["anchors"])
    return _walks[name]


@pytest.mark.parametrize("name", fr.FAMILY)
def test_walk_equals_live_reference_model(name, have_reference):
    if not have_reference:
        pytest.skip("/root/reference not present (the goldens cover this)")
    from oracle import ref_harness
    spec, nodes, plan, sd = fr.seeded(name)
    m = ref_harness.build_reference_model("cfg/deploy/%s.yaml" % name, 2)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("anchor" in k for k in missing)          # a seeded state dict loads into the reference's Model
    img = fr.golden_image(name)
    with torch.no_grad():
        ref = m(img)[0]
        fuse_dev = 0.0
        if name == "yolov7":
            m.fuse()
            fused = m(img)[0]
            fuse_dev, ref = float((fused - ref).abs().max()), fused
    dec, raw = _walk(name)
    print("FAMILY %s: head-logit std per level %s" % (name, [round(float(r.std()), 3) for r in raw]))
    _bar(name, dec, ref, fuse_dev)


@pytest.mark.parametrize("name", fr.FAMILY)
def test_walk_equals_golden(name):
    g = np.load(os.path.join(util.GOLDEN, "family_%s.npz" % name))
    spec, nodes, plan, sd = fr.seeded(name)
    assert fr.state_digest(sd) == str(g["state_digest"]), "the seeded state dict of %s is not the one the golden was recorded with" % name
    dec, raw = _walk(name)
    stds = [float(r.std()) for r in raw]
    print("FAMILY %s: head-logit std per level %s" % (name, [round(s, 3) for s in stds]))
    assert all(0.2 < s < 20 for s in stds) and all(bool(torch.isfinite(r).all()) for r in raw)      # the calibrated seeded network keeps O(1) activations
    _bar(name, dec, torch.from_numpy(g["decoded"]), float(g["fuse_dev"]) if "fuse_dev" in g.files else 0.0)
    if name != "yolov7":
        for l, r in enumerate(raw):
            assert np.array_equal(r.numpy(), g["raw%d" % l])


# ------------------------------------------------------------------------------------------------ 7. what already worked lowers as before
@pytest.mark.parametrize("tag", ["w6", "tiny"])
def test_w6_and_tiny_plans_are_unchanged(tag):
    g = np.load(os.path.join(util.GOLDEN, "family_parent_plans.npz"))
    cfg = json.loads(str(g[tag + "_cfg"]))
    p = graph.lower(graph.parse(arch.ARCHS[cfg["arch"]](cfg["nc"]))[0], cfg["hw"], cfg["hw"], cfg["max_batch"])
    assert p.ops.tobytes() == g[tag + "_ops"].tobytes()
    assert np.array_equal(p.buf_offsets, g[tag + "_buf_offsets"])
    assert [list(w["wkey"]) if isinstance(w["wkey"], tuple) else w["wkey"] for w in p.wlayout] == json.loads(str(g[tag + "_wkeys"]))
    assert not any("rep" in w for w in p.wlayout)

