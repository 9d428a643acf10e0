"""GPU: yolov7-tiny -- the model of the README's own command lines -- op by op on identical inputs (tests/teacher_forced.py), where it had only the chaotic end-to-end
bound of tests/test_detector_gpu.py::test_whole_network_heads_match_oracle.  Tiny is LeakyReLU everywhere, 32-channel layers (Cin % 64 == 32), no ReOrg
(an 8-channel input layout), and the SP / MP pools of csrc/y7t_post.hip.

  * 448 x 576, three frames, all checked: the stride-32 map is 14 x 18, so the 5 / 9 / 13 windows are all smaller than the map.  Convolutions at the project's
    layer bound, unchanged (3e-4 + 6e-4 |ref| + 2 sqrt(K) 2^-24 sum|w x|); pools, upsamples and copies bit-exact; the input layout tensor bit-exact against numpy.
    Run with the default lowering (both nn.Upsample read through the 1x1 convs behind them, as the CLI runs it) and with upsample-on-read off (`upsample2x` launched).
  * 1280 x 1280: only the three SP pools and their producer, on a random input slice -- `maxpool<13,1>` (generic: 40 x 40 > 1024 pixels) on tiny's real map."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import op_refs, teacher_forced

pytestmark = pytest.mark.gpu


def _tiny(hw, B):
    from yolov7_tracker_amd.detector import arch, model
    return model.Detector(arch.yolov7_tiny(80), None, img_size=hw, max_batch=B, seed=0)


@pytest.mark.parametrize("on_read", ["1", "0"])
def test_every_op_of_tiny_matches_the_oracle_teacher_forced(monkeypatch, on_read):
    monkeypatch.setenv("Y7T_UPSAMPLE_ON_READ", on_read)
    H, W, B = 448, 576, 3
    det = _tiny((H, W), B)
    p = det.plan
    assert not p.reorg and p.in_ld == 8 and not p.stem_fused
    img = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(0))
    det(img)
    torch.cuda.synchronize()
    # the input layout tensor (k_input_layout<false>, ldout 8, no ReOrg): bit-exact against the numpy reference, pad channels zero
    want0 = op_refs.input_layout(img.numpy(), 0, 0, 8)
    got0 = det.buffer_view(0, B, 8).view(B, H, W, 8).cpu().numpy()
    assert np.array_equal(got0.view(np.uint16), want0.view(np.uint16)) and not got0[..., 3:].view(np.uint16).any()
    names = det.launch_list(B)
    det(img)                                                         # launch_list re-ran the ops in place: a clean forward again
    torch.cuda.synchronize()
    fr = list(range(B))
    r = teacher_forced.check_every_op(det, B, fr, img.half().float(), names)
    case = "yolov7-tiny 448x576x3, upsample-on-read %s" % on_read
    for k in sorted(set(names)):                                     # the launch list by kernel: worst err / tol of the convs, `exact` for pools / upsamples / copies
        print("MARGIN %-44s %-60s %s" % (k, "%s, %d ops" % (case, names.count(k)), "worst err/tol %.3f" % r["worst"][k] if k in r["worst"] else "exact"))
    assert r["visited"] == list(range(len(p.ops))) == list(range(len(names)))
    for k in ("maxpool<5,1> lds", "maxpool<9,1> lds", "maxpool<13,1> lds"):
        assert names.count(k) == 1, names
    assert names.count("maxpool<2,2>") == 3, names
    cin32 = [i for i, op in enumerate(p.ops) if int(op["type"]) == 0 and int(op["Cin"]) % 64 == 32]
    assert len(cin32) >= 1 and all(int(p.ops[i]["act"]) == 2 for i in range(len(p.ops)) if int(p.ops[i]["type"]) == 0 and int(p.ops[i]["detect_level"]) < 0)
    if on_read == "0":
        assert names.count("upsample2x") == 2 and r["n_up"] == 0, names
        assert r["n_conv"] == 50 and r["n_other"] == 8
    else:
        assert "upsample2x" not in names and sum("upsample-on-read" in n for n in names) == r["n_up"] == 2, names
        assert r["n_conv"] == 50 and r["n_other"] == 6


def test_tiny_sp_pools_on_the_1280_map():
    """the three SP ops of the plan at the project's own workload size and the conv that feeds them, through y7t_det_forward_ops on a random fp16 input slice"""
    from oracle import detector_torch as dt
    from yolov7_tracker_amd import _lib
    det = _tiny((1280, 1280), 1)
    p, L = det.plan, det._L
    sp = [i for i, op in enumerate(p.ops) if int(op["type"]) == 2 and int(op["stride"]) == 1 and int(op["KH"]) in (5, 9, 13)]
    assert [int(p.ops[i]["KH"]) for i in sp] == [5, 9, 13] and sp == list(range(sp[0], sp[0] + 3))
    o5 = p.ops[sp[0]]
    Hm, Wm, C = int(o5["H"]), int(o5["W"]), int(o5["Cin"])
    assert (Hm, Wm) == (40, 40) and all(int(p.ops[i][f]) == int(o5[f]) for i in sp for f in ("in_buf", "in_ld", "in_coff", "H", "W", "Cin"))
    prod = [i for i, op in enumerate(p.ops[:sp[0]]) if int(op["type"]) == 0 and int(op["out_buf"]) == int(o5["in_buf"]) and
            int(op["out_coff"]) <= int(o5["in_coff"]) and int(o5["in_coff"]) + C <= int(op["out_coff"]) + int(op["Cout"])]
    assert len(prod) == 1
    po = p.ops[prod[0]]
    ci = sum(1 for op in p.ops[:prod[0]] if int(op["type"]) == 0)       # the producer's entry in the weight layout (tiny has no two-layer ops)
    wl = p.wlayout[ci]
    assert not any(w.get("fused_next") for w in p.wlayout) and wl["cin"] == int(po["Cin"])
    Hi, Wi, Cin = int(po["H"]), int(po["W"]), int(po["Cin"])
    x = torch.from_numpy(np.random.default_rng(hash((Hi, Wi, Cin)) % 2 ** 32).normal(0, 1, (1, Hi, Wi, Cin)).astype(np.float16))
    det.buffer_view(int(po["in_buf"]), 1, int(po["in_ld"])).view(1, Hi, Wi, -1)[..., int(po["in_coff"]):int(po["in_coff"]) + Cin] = x.cuda()
    names = []
    for i in [prod[0]] + sp:
        _lib.check(L.y7t_det_forward_ops(p.handle, 1, i, i + 1, _lib.stream_ptr()))
        names.append(L.y7t_last_kernel().decode())
    torch.cuda.synchronize()
    assert names[1:] == ["maxpool<5,1>", "maxpool<9,1>", "maxpool<13,1>"], names       # 1600 pixels: over the LDS kernels' limit
    for k in names[1:]:
        print("MARGIN %-44s %-60s exact" % (k, "yolov7-tiny 1280x1280x1, 40x40 map, 256 channels of a 1024-wide buffer"))
    # the producer at the layer bound
    xs = x.float().permute(0, 3, 1, 2)
    keys = wl["wkey"] if isinstance(wl["wkey"], tuple) else (wl["wkey"],)
    k, s_, pd = int(po["KH"]), int(po["stride"]), int(po["pad"])
    ref = torch.cat([dt._conv_bn_act(xs, det._sd, key, k, s_, pd, wl["act"], fp16=True, round_out=False) for key in keys], 1).permute(0, 2, 3, 1)
    absum = torch.cat([dt.conv_abs_sum(xs, det._sd, key, s_, pd) for key in keys], 1).permute(0, 2, 3, 1)
    got = teacher_forced.arena_slice(det, 1, int(po["out_buf"]), int(po["out_ld"]), int(po["out_coff"]), int(po["Cout"]), Hm, Wm, [0]).float().cpu()
    tol = 3e-4 + 6e-4 * ref.abs() + 2 * float(Cin * k * k) ** 0.5 * 2.0 ** -24 * absum
    assert bool(((got - ref).abs() <= tol).all()), (names[0], float(((got - ref).abs() / tol).max()))
    # the pools, bit-exact on what the producer actually wrote
    src = teacher_forced.arena_slice(det, 1, int(o5["in_buf"]), int(o5["in_ld"]), int(o5["in_coff"]), C, Hm, Wm, [0]).float().cpu().permute(0, 3, 1, 2)
    assert float(src.std()) > 0.05 and float((src < 0).float().mean()) > 0.2          # LeakyReLU output: negative values are there
    for i in sp:
        op = p.ops[i]
        K = int(op["KH"])
        out = teacher_forced.arena_slice(det, 1, int(op["out_buf"]), int(op["out_ld"]), int(op["out_coff"]), C, Hm, Wm, [0]).float().cpu()
        assert torch.equal(out, F.max_pool2d(src, K, 1, K // 2).permute(0, 2, 3, 1)), "maxpool<%d,1>" % K
