"""Records the fixtures of tests/test_family_cpu.py / tests/test_family_gpu.py from the live reference (needs /root/reference; run from the repository root):

    python tests/golden/make_golden_family.py            # family_<graph>.npz for the five graphs + family_repconv.npz
    python tests/golden/make_golden_family.py --plans    # family_parent_plans.npz -- ONLY at the commit BEFORE a change of the lowering: it records what
                                                         # the lowering of that commit emits for yolov7-w6 and yolov7-tiny

family_<graph>.npz   the reference Model's raw head tensors and decoded output on one fixed image batch (P5 graphs 96 x 160, P6 graphs 192 x 320, B = 2) with the
                     seeded network of tests/family_ref.py::seeded(graph) (nc = 2, seed 0, bn_bias_mean = 2), the digest of that state dict and its BatchNorm running
                     statistics in fp16 (`bn_stats`: the calibration's reductions depend on the host's thread count) -- everything else is regenerated from the seed.  yolov7: the reference after its own .fuse() (RepConv re-parameterised, models/yolo.py:283-302) plus `fuse_dev`,
                     the largest absolute difference between its fused and unfused decoded outputs.
family_repconv.npz   RepConv(32, 48) and RepConv(32, 32) (the second has an identity branch) with randomised BN statistics: the training-form tensors and what the
                     reference's fuse_repvgg_block (models/common.py:584-640) makes of them.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))


def record_graphs():
    from oracle import ref_harness
    from tests import family_ref as fr
    for name in fr.FAMILY:
        spec, nodes, plan, sd = fr.seeded(name, calibrate=True)
        m = ref_harness.build_reference_model("cfg/deploy/%s.yaml" % name, 2)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all("anchor" in k for k in missing), (missing, unexpected)
        img = fr.golden_image(name)
        with torch.no_grad():
            dec, raw = m(img)
        out = {"state_digest": np.array(fr.state_digest(sd)), "hw": np.array(fr.small_hw(name)),
               "bn_stats": torch.cat([sd[k].reshape(-1) for k in fr.stat_keys(sd)]).numpy().astype(np.float16)}
        if name == "yolov7":
            m.fuse()
            with torch.no_grad():
                dec_f, raw_f = m(img)
            out["fuse_dev"] = np.array(float((dec_f - dec).abs().max()))
            dec, raw = dec_f, raw_f
        out["decoded"] = dec.numpy()
        for l, r in enumerate(raw):
            out["raw%d" % l] = r.numpy()
        np.savez_compressed(os.path.join(HERE, "family_%s.npz" % name), **out)
        print(name, "decoded", tuple(dec.shape), "fuse_dev", out.get("fuse_dev"), "head std", [round(float(r.std()), 3) for r in raw])


def record_repconv():
    from oracle import ref_harness
    ns = ref_harness.load_detector()
    g = torch.Generator().manual_seed(3)
    out = {}
    for tag, (c1, c2) in (("a", (32, 48)), ("b", (32, 32))):
        m = ns.common.RepConv(c1, c2, 3, 1).eval()
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eps = 1e-3                     # utils/torch_utils.py initialize_weights: what every BatchNorm of a Model has
                mod.weight.data = torch.rand(mod.num_features, generator=g) + 0.5
                mod.bias.data = torch.randn(mod.num_features, generator=g) * 0.5
                mod.running_mean.data = torch.randn(mod.num_features, generator=g) * 0.5
                mod.running_var.data = torch.rand(mod.num_features, generator=g) + 0.5
            elif isinstance(mod, torch.nn.Conv2d):
                mod.weight.data = torch.randn(mod.weight.shape, generator=g) * 0.1
        for k, v in m.state_dict().items():
            if "num_batches_tracked" not in k:
                out["%s_in.%s" % (tag, k)] = v.detach().numpy().copy()
        m.fuse_repvgg_block()
        out["%s_fused_weight" % tag] = m.rbr_reparam.weight.detach().numpy().copy()
        out["%s_fused_bias" % tag] = m.rbr_reparam.bias.detach().numpy().copy()
    np.savez_compressed(os.path.join(HERE, "family_repconv.npz"), **out)
    print("family_repconv.npz", sorted(out))


def record_parent_plans():
    from yolov7_tracker_amd.detector import arch, graph
    out = {}
    for tag, name, nc, hw, mb in (("w6", "yolov7-w6", 10, 1280, 80), ("tiny", "yolov7-tiny", 80, 640, 1)):
        p = graph.lower(graph.parse(arch.ARCHS[name](nc))[0], hw, hw, mb)
        out[tag + "_ops"] = np.frombuffer(p.ops.tobytes(), np.uint8)
        out[tag + "_buf_offsets"] = p.buf_offsets
        out[tag + "_wkeys"] = np.array(json.dumps([list(w["wkey"]) if isinstance(w["wkey"], tuple) else w["wkey"] for w in p.wlayout]))
        out[tag + "_cfg"] = np.array(json.dumps(dict(arch=name, nc=nc, hw=hw, max_batch=mb)))
    np.savez_compressed(os.path.join(HERE, "family_parent_plans.npz"), **out)


if __name__ == "__main__":
    if "--plans" in sys.argv:
        record_parent_plans()
    else:
        record_repconv()
        record_graphs()
