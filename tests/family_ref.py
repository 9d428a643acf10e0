"""Test-side reference walk for the whole YOLOv7 family (tests/test_family_cpu.py, tests/test_family_gpu.py).

oracle.detector_torch.forward raises on node kinds it does not know, so this walk brings the two that the family adds and leaves the arithmetic of everything
else to the oracle's own functions (dt._conv_bn_act, dt.decode_level):
  add       Shortcut (models/common.py:80-86): x[0] + x[1]
  RepConv   the reference's own forward formula (models/common.py:507): act(bn(dense(x)) + bn(1x1(x)) [+ bn_id(x)]) on a training-form state dict, act(reparam(x))
            on a deploy-form one -- three branches, NOT the product's re-parameterised kernel: this module never calls weights.folded.
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detector_torch as dt

BN_EPS = dt.BN_EPS


def is_rep(n):
    return n.kind == "conv" and bool(n.extra and n.extra.get("rep"))


def _act(y, act):
    return F.silu(y) if act == 1 else (F.leaky_relu(y, 0.1) if act == 2 else y)


def repconv_branches(x, sd, key, stride=1, dtype=torch.float32):
    """the summands of RepConv.forward before the activation (models/common.py:500-507), each in `dtype`: [bn(dense(x)), bn(1x1(x)), bn_id(x) if present] --
    or [reparam(x)] for a deploy-form layer"""
    x = x.to(dtype)
    if key + ".rbr_reparam.weight" in sd:
        return [F.conv2d(x, sd[key + ".rbr_reparam.weight"].to(dtype), sd[key + ".rbr_reparam.bias"].to(dtype), stride=stride, padding=1)]

    def bn(z, pre):
        return F.batch_norm(z, sd[pre + ".running_mean"].to(dtype), sd[pre + ".running_var"].to(dtype), sd[pre + ".weight"].to(dtype), sd[pre + ".bias"].to(dtype),
                            False, 0.0, BN_EPS)
    out = [bn(F.conv2d(x, sd[key + ".rbr_dense.0.weight"].to(dtype), None, stride=stride, padding=1), key + ".rbr_dense.1"),
           bn(F.conv2d(x, sd[key + ".rbr_1x1.0.weight"].to(dtype), None, stride=stride, padding=0), key + ".rbr_1x1.1")]
    if key + ".rbr_identity.weight" in sd:
        out.append(bn(x, key + ".rbr_identity"))
    return out


def repconv(x, sd, key, act=1, stride=1, dtype=torch.float32):
    """RepConv.forward, summed in the reference's order (dense + 1x1 + identity)"""
    br = repconv_branches(x, sd, key, stride, dtype)
    y = br[0]
    for b in br[1:]:
        y = y + b
    return _act(y, act)


def repconv_abs_sum(x, sd, key, stride=1):
    """an upper bound of sum_k |w_k x_k| + |b| of the layer's equivalent 3x3 kernel, float64, from the branches (triangle inequality): the scale of the error bound
    of the convolution bar (tests/teacher_forced.py::conv_tolerance)"""
    x = x.double().abs()
    if key + ".rbr_reparam.weight" in sd:
        return F.conv2d(x, sd[key + ".rbr_reparam.weight"].double().abs(), sd[key + ".rbr_reparam.bias"].double().abs(), stride=stride, padding=1)

    def affine(pre):
        scale = sd[pre + ".weight"].double() / torch.sqrt(sd[pre + ".running_var"].double() + BN_EPS)
        return scale, sd[pre + ".bias"].double() - sd[pre + ".running_mean"].double() * scale
    s3, t3 = affine(key + ".rbr_dense.1")
    s1, t1 = affine(key + ".rbr_1x1.1")
    y = F.conv2d(x, (sd[key + ".rbr_dense.0.weight"].double() * s3[:, None, None, None]).abs(), t3.abs(), stride=stride, padding=1)
    y = y + F.conv2d(x, (sd[key + ".rbr_1x1.0.weight"].double() * s1[:, None, None, None]).abs(), t1.abs(), stride=stride, padding=0)
    if key + ".rbr_identity.weight" in sd:
        si, ti = affine(key + ".rbr_identity")
        y = y + x * si.abs()[None, :, None, None] + ti.abs()[None, :, None, None]
    return y


@torch.no_grad()
def forward(nodes, sd, img, anchors, keep=False, fp16=False):
    """oracle.detector_torch.forward's contract (same arguments, same results) for graphs with `add` nodes and RepConv layers.
    fp16=True emulates the storage precision of the HIP path as the oracle does: activations rounded to fp16 after every layer (a RepConv: the float64 three-branch
    sum, rounded once; an add: the exact sum, rounded once)."""
    vals = {0: img.float().half().float() if fp16 else img.float()}
    raw = []
    H = img.shape[2]
    for n in nodes[1:]:
        if n.kind == "detect":
            ex = n.extra
            a = torch.tensor(anchors, dtype=torch.float32).view(ex["nl"], -1, 2)
            base = "model.%d" % n.layer
            for l, j in enumerate(n.src):      # models/yolo.py:39-57 (Detect), :93-94 (IDetect), as oracle.detector_torch.forward states it
                x = vals[j]
                if ex["kind"] in ("IDetect", "IAuxDetect") and "%s.ia.%d.implicit" % (base, l) in sd:
                    x = x + sd["%s.ia.%d.implicit" % (base, l)].float()
                wd = sd["%s.m.%d.weight" % (base, l)].float()
                x = F.conv2d(x, wd.half().float() if fp16 else wd, sd["%s.m.%d.bias" % (base, l)].float())
                if ex["kind"] in ("IDetect", "IAuxDetect") and "%s.im.%d.implicit" % (base, l) in sd:
                    x = x * sd["%s.im.%d.implicit" % (base, l)].float()
                bs, _, ny, nx = x.shape
                raw.append(x.view(bs, ex["na"], ex["no"], ny, nx).permute(0, 1, 3, 4, 2).contiguous())
            continue
        if any(j not in vals for j in n.src):
            continue                                    # the dead aux branch of a training graph
        src = [vals[j] for j in n.src]
        if n.kind == "add":
            y = src[0] + src[1]
            y = y.half().float() if fp16 else y
        elif is_rep(n):
            if fp16:
                y = repconv(src[0], sd, n.wkey, n.act, n.s, torch.float64).float().half().float()
            else:
                y = repconv(src[0], sd, n.wkey, n.act, n.s)
        elif n.kind == "conv":
            if n.wkey + ".conv.weight" not in sd:
                continue
            y = dt._conv_bn_act(src[0], sd, n.wkey, n.k, n.s, n.p, n.act, fp16)
        elif n.kind == "reorg":
            x = src[0]
            y = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)
        elif n.kind == "concat":
            y = torch.cat(src, 1)
        elif n.kind == "up":
            y = F.interpolate(src[0], scale_factor=2, mode="nearest")
        elif n.kind == "pool":
            y = F.max_pool2d(src[0], n.k, n.s, n.p)
        else:
            raise NotImplementedError(n.kind)
        vals[n.idx] = y
    out = (dt.decode_heads(raw, anchors, H), raw)
    return out + (vals,) if keep else out


# ---- the five graphs, their test sizes and seeded networks (shared by the CPU and the GPU file) ----
FAMILY = ("yolov7", "yolov7x", "yolov7-e6", "yolov7-d6", "yolov7-e6e")
P6 = ("yolov7-e6", "yolov7-d6", "yolov7-e6e")


def small_hw(name):
    return (192, 320) if name in P6 else (96, 160)


def nominal_hw(name):
    return (1280, 1280) if name in P6 else (640, 640)


def state_digest(sd):
    """sha256 over the names, shapes and bytes of a state dict, in name order"""
    h = hashlib.sha256()
    for k in sorted(sd):
        a = np.ascontiguousarray(sd[k].detach().cpu().numpy())
        h.update(k.encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def golden_image(name, B=2):
    hw = small_hw(name)
    return torch.rand((B, 3) + hw, generator=torch.Generator().manual_seed(9))


_seeded = {}
STAT_KEYS = (".running_mean", ".running_var")


def stat_keys(sd):
    return [k for k in sorted(sd) if k.endswith(STAT_KEYS)]


def seeded(name, calibrate=False):
    """-> (spec, nodes, plan at the small size, state dict) of THE seeded network of graph `name` that the goldens were recorded with: nc = 2, seed 0, BatchNorm shifts
    around +2 (weights.random_state_dict(bn_bias_mean=2): the conditioning the pinned tests use), BatchNorm running statistics from tests/golden/family_<name>.npz.
    The statistics are the result of weights.calibrate_bn at the small size, rounded to fp16 and kept in the golden: the calibration's reductions depend on the host's
    thread count, everything else is regenerated from the seed.  calibrate=True (the golden maker) computes them instead.  Shared: callers must not modify it."""
    import os
    from tests import util
    from yolov7_tracker_amd.detector import arch, graph, weights
    if (name, calibrate) not in _seeded:
        spec = arch.ARCHS[name](2)
        nodes, _ = graph.parse(spec)
        plan = graph.lower(nodes, *small_hw(name), 2)
        sd = weights.random_state_dict(plan.wlayout, 0, bn_bias_mean=2.0)
        keys = stat_keys(sd)
        if calibrate:
            sd = weights.calibrate_bn(nodes, sd, hw=small_hw(name), seed=0)
            for k in keys:
                sd[k] = sd[k].half().float()
        else:
            g = np.load(os.path.join(util.GOLDEN, "family_%s.npz" % name))
            flat, o = torch.from_numpy(g["bn_stats"].astype(np.float32)), 0
            for k in keys:
                sd[k] = flat[o:o + sd[k].numel()].clone()
                o += sd[k].numel()
            assert o == flat.numel()
        _seeded[(name, calibrate)] = (spec, nodes, plan, sd)
    return _seeded[(name, calibrate)]
