"""Every op of a family detector's launch list judged on identical inputs: tests/teacher_forced.py::check_every_op for plans that hold adds and RepConv layers.

  convolutions   tests/teacher_forced.py::conv_tolerance, unchanged, against the oracle's layer (BN fold in float64, fp16 weights, fp32 accumulate);
  RepConv        against the reference's three-branch forward (tests/family_ref.py::repconv) in float64 on the op's fp16 input, unrounded -- the device stores the
                 re-parameterised kernel in fp16, so the bar's sum |w x| term carries 2^-11 more (each stored weight is within half an fp16 ulp, 2^-11 relative, of
                 the exact one: |sum (w~ - w) x| <= 2^-11 sum |w x|), with sum |w x| bounded from the branches (family_ref.repconv_abs_sum);
  pools, copies, upsamples, adds   bit-exact; an add against (a.float() + b.float()).half()."""
import collections

import torch
import torch.nn.functional as F

from tests import family_ref as fr
from tests.teacher_forced import arena_slice, conv_tolerance


def check_every_op(det, B, frames, x0, names):
    """arguments and result as tests/teacher_forced.py::check_every_op; the result also counts `n_add` and `n_rep`"""
    from oracle import detector_torch as dt
    p, sd, frs = det.plan, det._sd, frames
    ci = 0
    worst = collections.defaultdict(float)
    n = collections.Counter()
    visited = []

    def sl(buf, ld, coff, c, H, W):
        return arena_slice(det, B, buf, ld, coff, c, H, W, frs).float().cpu()
    for oi, op in enumerate(p.ops):
        o = {k: int(op[k]) for k in op.dtype.names}
        H, W, Cin = o["H"], o["W"], o["Cin"]
        x = x0.clone() if oi == 0 and o["in_buf"] == 0 else sl(o["in_buf"], o["in_ld"], o["in_coff"], Cin, H, W).permute(0, 3, 1, 2).contiguous()
        if o["type"] == 0 and o["up_C"] > 0:
            lo = sl(o["up_buf"], o["up_ld"], o["up_coff"], o["up_C"], H // 2, W // 2).permute(0, 3, 1, 2)
            x[:, o["up_c0"]:o["up_c0"] + o["up_C"]] = F.interpolate(lo, scale_factor=2, mode="nearest")
            n["up_on_read"] += 1
        if o["type"] == 0:
            wl = p.wlayout[ci]
            ci += 1
            assert not wl.get("fused_next"), "the family plans at these sizes hold no fused stride-2 + twin op"
            x = x[:, :wl["cin"]]
            k, s_, pd = o["KH"], o["stride"], o["pad"]
            extra_tol = 0.0
            if wl.get("rep"):
                ref = fr.repconv(x, sd, wl["wkey"], wl["act"], s_, torch.float64).float()
                absum = fr.repconv_abs_sum(x, sd, wl["wkey"], s_).float()
                extra_tol = 2.0 ** -11
                got = sl(o["out_buf"], o["out_ld"], o["out_coff"], o["Cout"], o["Ho"], o["Wo"])
                n["rep"] += 1
            elif wl["kind"] == "conv":
                keys = wl["wkey"] if isinstance(wl["wkey"], tuple) else (wl["wkey"],)
                ref = torch.cat([dt._conv_bn_act(x, sd, key, k, s_, pd, wl["act"], fp16=True, round_out=False) for key in keys], 1)
                absum = torch.cat([dt.conv_abs_sum(x, sd, key, s_, pd) for key in keys], 1)
                got = sl(o["out_buf"], o["out_ld"], o["out_coff"], o["Cout"], o["Ho"], o["Wo"])
            else:
                ref = F.conv2d(x, sd[wl["wkey"] + ".weight"].half().float(), sd[wl["wkey"] + ".bias"].float())
                absum = F.conv2d(x.abs(), sd[wl["wkey"] + ".weight"].half().float().abs(), sd[wl["wkey"] + ".bias"].float().abs())
                got = det.head_tensor(wl["level"], B)[frs].cpu()
            ref, absum = ref.permute(0, 2, 3, 1), absum.permute(0, 2, 3, 1)
            err = (got - ref).abs()
            tol = conv_tolerance(ref, absum, Cin * k * k, extra_tol)
            assert not bool((err > tol).any()), "op %d %s (%s, %dx%d %d->%d k%d s%d): %d values off, worst err/tol %.2f" % (
                oi, names[oi], wl["wkey"], H, W, Cin, o["Cout"], k, s_, int((err > tol).sum()), float((err / tol).max()))
            worst[names[oi]] = max(worst[names[oi]], float((err / tol).max()))
            n["conv"] += 1
        else:
            if o["type"] == 1:
                ref = F.interpolate(x, scale_factor=2, mode="nearest")
                n["up"] += 1
            elif o["type"] == 2:
                ref = F.max_pool2d(x, o["KH"], o["stride"], o["pad"])
                n["copy" if o["KH"] == 1 else "pool"] += 1
            else:
                assert o["type"] == 3 and names[oi] == "add"
                b2 = sl(o["up_buf"], o["up_ld"], o["up_coff"], Cin, H, W).permute(0, 3, 1, 2)
                ref = (x + b2).half().float()
                n["add"] += 1
            got = sl(o["out_buf"], o["out_ld"], o["out_coff"], Cin, ref.shape[2], ref.shape[3])
            assert torch.equal(got, ref.permute(0, 2, 3, 1)), "op %d %s" % (oi, names[oi])
        visited.append(oi)
    assert ci == len(p.wlayout) and visited == list(range(len(p.ops)))
    return dict(n_conv=n["conv"], n_rep=n["rep"], n_add=n["add"], n_pool=n["pool"], n_copy=n["copy"], n_up=n["up"], n_up_on_read=n["up_on_read"], visited=visited,
                worst=dict(worst))
