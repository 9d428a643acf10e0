"""Every op of a detector's launch list judged on IDENTICAL inputs (shared by tests/test_detector_pinned_gpu.py and tests/test_tiny_pinned_gpu.py).

After one forward of the whole list every tensor is still in the arena (one buffer per tensor), so for every op: read the op's actual fp16 input slice, evaluate
the oracle's layer on it (oracle/detector_torch.py: BN fold in float64, fp16 weights, fp32 accumulate) and compare with the op's actual output slice.
  convolutions  |got - ref| <= 3e-4 + 6e-4 |ref| + 2 sqrt(K) 2^-24 sum|w x|: half an fp16 ulp of the result plus the probabilistic forward error bound of an
                fp32 accumulation of K terms in another order (the worst-case one has K in place of 2 sqrt(K));
  pools, upsamples, concat copies: bit-exact."""
import collections

import torch
import torch.nn.functional as F

from yolov7_tracker_amd.detector.layout import WeightLayout


def conv_tolerance(ref, absum, K, extra_tol=0.0):
    """the convolution bar of the module docstring for a result `ref` of K-term sums with sum_k |w_k x_k| = absum (|act'| <= 1.1 (SiLU; LeakyReLU 1): the pre-activation
    bound carries over)"""
    return 3e-4 + 6e-4 * ref.abs() + (2 * float(K) ** 0.5 * 2.0 ** -24 + extra_tol) * absum


def arena_slice(det, B, buf, ld, coff, c, H, W, frames):
    v = det.buffer_view(buf, B, ld).view(B, H, W, ld)
    return v[frames][..., coff:coff + c]


def check_every_op(det, B, frames, x0, names):
    """det: a Detector whose arena holds one clean forward of B images; frames: the images whose every value is compared; x0: what op 0 reads for those images
    (NCHW float32 holding the fp16 values of the layout tensor, real channels only -- whether or not that tensor exists in memory); names: det.launch_list(B).
    Asserts per op; -> dict(n_conv, n_other, n_up, visited, worst) with `worst` the largest err / tol per kernel name."""
    from oracle import detector_torch as dt
    p, sd, fr = det.plan, det._sd, frames
    ci = 0
    worst = collections.defaultdict(float)
    n_conv = n_other = n_up = 0
    visited = []
    for oi, op in enumerate(p.ops):
        H, W, Cin = int(op["H"]), int(op["W"]), int(op["Cin"])
        if oi == 0 and int(op["in_buf"]) == 0:
            x = x0.clone()                                          # op 0 reads the frame through the layout kernel (or, fused stem, straight from the frame)
        else:
            x = arena_slice(det, B, int(op["in_buf"]), int(op["in_ld"]), int(op["in_coff"]), Cin, H, W, fr).float().cpu().permute(0, 3, 1, 2).contiguous()
        if int(op["up_C"]) > 0:      # upsample-on-read: these channels of the concat exist only at half resolution (nn.Upsample(None, 2, 'nearest'))
            c0, cu = int(op["up_c0"]), int(op["up_C"])
            lo = arena_slice(det, B, int(op["up_buf"]), int(op["up_ld"]), int(op["up_coff"]), cu, H // 2, W // 2, fr).float().cpu().permute(0, 3, 1, 2)
            x[:, c0:c0 + cu] = F.interpolate(lo, scale_factor=2, mode="nearest")
            n_up += 1
        if int(op["type"]) == 0:
            wl = p.wlayout[ci]
            ci += 1
            x = x[:, :wl["cin"]]                                   # the real channels of a padded layout (the stem's 12 of 16, tiny's 3 of 8)
            k, s_, pd = int(op["KH"]), int(op["stride"]), int(op["pad"])
            extra_tol = 0.0
            if wl["kind"] == "conv" and wl.get("fused_next"):      # WeightLayout.WS_S2_TWIN: the stride-2 layer + the twin 1x1 behind it in one launch; the tensor between them is never written
                w2 = p.wlayout[ci]
                ci += 1
                assert op["korder"] == WeightLayout.WS_S2_TWIN and w2.get("fused_prev") and isinstance(w2["wkey"], tuple)
                mid = dt._conv_bn_act(x, sd, wl["wkey"], k, s_, pd, wl["act"], fp16=True, round_out=True)        # (fp16 in LDS, as it would be in memory)
                ref = torch.cat([dt._conv_bn_act(mid, sd, key, 1, 1, 0, w2["act"], fp16=True, round_out=False) for key in w2["wkey"]], 1)
                absum = torch.cat([dt.conv_abs_sum(mid, sd, key, 1, 0) for key in w2["wkey"]], 1)
                extra_tol = 2.0 ** -11      # a 1-ulp difference of a middle value (other summation order) times its weight: bounded by 2^-11 sum |w x|
                got = arena_slice(det, B, int(op["out_buf"]), int(op["out_ld"]), int(op["out_coff"]), int(op["Cout"]), int(op["Ho"]), int(op["Wo"]), fr)
                got = got.float().cpu()
            elif wl["kind"] == "conv":
                keys = wl["wkey"] if isinstance(wl["wkey"], tuple) else (wl["wkey"],)
                ref = torch.cat([dt._conv_bn_act(x, sd, key, k, s_, pd, wl["act"], fp16=True, round_out=False) for key in keys], 1)
                absum = torch.cat([dt.conv_abs_sum(x, sd, key, s_, pd) for key in keys], 1)      # sum_k |w_k x_k| (+ |b|) per output
                got = arena_slice(det, B, int(op["out_buf"]), int(op["out_ld"]), int(op["out_coff"]), int(op["Cout"]), int(op["Ho"]), int(op["Wo"]), fr)
                got = got.float().cpu()
            else:                                                   # Detect 1x1 (models/yolo.py:46): fp16 weights, fp32 bias, fp32 output
                ref = F.conv2d(x, sd[wl["wkey"] + ".weight"].half().float(), sd[wl["wkey"] + ".bias"].float())
                absum = F.conv2d(x.abs(), sd[wl["wkey"] + ".weight"].half().float().abs(), sd[wl["wkey"] + ".bias"].float().abs())
                got = det.head_tensor(wl["level"], B)[fr].cpu()
            ref, absum = ref.permute(0, 2, 3, 1), absum.permute(0, 2, 3, 1)
            err = (got - ref).abs()
            tol = conv_tolerance(ref, absum, Cin * k * k, extra_tol)
            bad = err > tol
            if bool(bad.any()):
                w_ = int(torch.argmax((err / tol).flatten()))
                detail = "got %.6g ref %.6g sum|wx| %.4g tol %.3g" % (float(got.flatten()[w_]), float(ref.flatten()[w_]), float(absum.flatten()[w_]), float(tol.flatten()[w_]))
            assert not bool(bad.any()), "op %d %s (%s, %dx%d %d->%d k%d s%d): %d values off, worst err/tol %.2f [%s]" % (
                oi, names[oi], wl["wkey"], H, W, Cin, int(op["Cout"]), k, s_, int(bad.sum()), float((err / tol).max()), detail)
            worst[names[oi]] = max(worst[names[oi]], float((err / tol).max()))
            n_conv += 1
        else:
            if int(op["type"]) == 1:
                ref = F.interpolate(x, scale_factor=2, mode="nearest")                     # nn.Upsample(None, 2, 'nearest')
            else:
                ref = F.max_pool2d(x, int(op["KH"]), int(op["stride"]), int(op["pad"]))  # SPPCSPC pools (cascaded), SP / MP, concat copies (k = 1)
            got = arena_slice(det, B, int(op["out_buf"]), int(op["out_ld"]), int(op["out_coff"]), Cin, ref.shape[2], ref.shape[3], fr).float().cpu()
            assert torch.equal(got, ref.permute(0, 2, 3, 1)), "op %d %s" % (oi, names[oi])
            n_other += 1
        visited.append(oi)
    assert ci == len(p.wlayout)
    return dict(n_conv=n_conv, n_other=n_other, n_up=n_up, visited=visited, worst=dict(worst))
