"""Plain numpy float64 references of csrc/y7t_reid_fused.hip::k_osnet_x025, ONE STORED TENSOR AT A TIME, in the style of tests/op_refs.py (whose conv, dwconv3,
maxpool3s2, avgpool2, gap, fc and sum_bound they reuse), for the tensors the kernel's TAP instance copies out of LDS (tests/test_reid_fused_taps_gpu.py).

Every reference is TEACHER-FORCED: its inputs are the device's own taps of the tensors that op reads (fp16 values are exact in float64), so no error is carried
from op to op and every bar is that of a single op.  `staged()` walks the network and yields one comparison per tapped tensor; `chain()` runs the same functions
from a float32 crop without teacher forcing and without fp16 stores (== the oracle network up to the blob's fp16 weights, tests/test_reid_fused_ref_cpu.py);
`emulate()` is a host emulation of the kernel (fp32 accumulation in a shuffled order, fp16 stores at the kernel's storage points) that produces the same taps --
with, on request, one planted fault -- so that the bars are shown to pass a correct kernel and to catch a wrong one without a GPU.

The parameters come from the blob of tracker/reid.py::pack_fused, decoded in the kernel's consumption order by `decode_blob` (the one decoder, also behind
tests/test_reid_oracle.py::_interpret_fused_blob; the packing itself is pinned by test_fused_blob_encodes_the_network).

Layouts: activations NHWC (N, H, W, C) with N = crops; 1x1 weights (Co, Ci); depthwise weights (C, 3, 3).

Bars (derived, never tuned; u = 2^-24).  An fp32 quantity with forward bound b = sum_bound(K, sum|terms|, ref) that the kernel then stores as fp16:
    b + 2^-11 (|ref| + b) + 2^-25          (the conversion's half ulp of the value actually converted; 2^-25 = half the fp16 subnormal spacing)
and |ref| < 65504 is asserted.  K: stem 147 + 1, 1x1 convs CIN (+ 1 with a bias), depthwise 10, block output 4 MIDp + CIN (downsample) or + 1 (identity) + 1,
average pool 4, v 32, fc 129.  feats, v, S and gate are fp32: the fp32 bound alone.  Maxpool and zeros are exact."""
import numpy as np

from tests import op_refs as R

U32 = R.U32
U16 = 2.0 ** -11
f32, f16, f64 = np.float32, np.float16, np.float64

# name, H, W, CIN, COUT, MID (padded to a multiple of 16), R (hidden units of the gate), real MID
BLOCKS = [("conv2.0", 32, 16, 16, 64, 16, 1, 16), ("conv2.1", 32, 16, 64, 64, 16, 1, 16), ("conv3.0", 16, 8, 64, 96, 32, 1, 24), ("conv3.1", 16, 8, 96, 96, 32, 1, 24),
          ("conv4.0", 8, 4, 96, 128, 32, 2, 32), ("conv4.1", 8, 4, 128, 128, 32, 2, 32)]
TRANS = {"conv2.1": ("conv2.2", 64), "conv3.1": ("conv3.2", 96)}       # the transition behind a block
NW = 8
FAMILIES = ["crop", "stem", "maxpool", "x1", "U", "T", "S", "gate", "X", "transition", "tail", "zeros"]


GATE_FACTOR = 6


def gate_scaled_state_dict(factor, seed=3):
    """weights (B) of the tap tests: the suite's seeded weights with every gate.fc1 / gate.fc2 weight times `factor`, so that the gates leave the 0.35-0.61 band the
    plain scales keep them in (factor 1: weights (A), the suite's own)"""
    from yolov7_tracker_amd.tracker import reid
    sd = reid.random_state_dict(reid.osnet_spec(0.25), seed)
    return {k: (v * factor if k.endswith(("gate.fc1.weight", "gate.fc2.weight")) else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ the blob, in the kernel's consumption order
def decode_blob(blob):
    """-> {"stem": (W (16, 3, 7, 7), b), "blocks": [{c1w, c1b, g_w1 (R, MID), g_b1, g_w2 (R, MID), g_b2, c3w (fp16 values), c3b, dnw | None,
    lights: [(w (MID, MID), dw (MID, 3, 3), db)] * 10}], "conv2.2" / "conv3.2" / "conv5": (w, b), "fc": (w (512, 128), b)}, float32 arrays"""
    buf = memoryview(np.ascontiguousarray(blob).tobytes())
    pos = [0]

    def take(nbytes, dtype):
        a = np.frombuffer(buf[pos[0]:pos[0] + nbytes], dtype=dtype)
        pos[0] += nbytes
        return a

    def unfrag(ng, nk):
        fr = take(ng * nk * 512, f16).reshape(ng, nk, 64, 4).astype(f32)
        M = np.zeros((ng * 16, nk * 16), f32)
        lane = np.arange(64)
        for g in range(ng):
            for k in range(nk):
                for e in range(4):
                    M[g * 16 + lane % 16, k * 16 + 4 * (lane // 16) + e] = fr[g, k, :, e]
        return M

    def vec(n):
        return take(4 * n, f32).copy()

    P = {}
    # conv1 7x7: fragments [kh*2 + half][lane][e]: row lane % 16, input pixel kw = 4 * half + lane // 16, channel e (kw = 7 and e = 3 multiply the halo / the 4th channel)
    fr = take(14 * 512, f16).reshape(14, 64, 4).astype(f32)
    W1 = np.zeros((16, 3, 7, 7), f32)
    lane = np.arange(64)
    for kh in range(7):
        for h in range(2):
            kw = 4 * h + lane // 16
            ok = kw < 7
            assert not fr[kh * 2 + h, ~ok].any() and not fr[kh * 2 + h, :, 3].any()
            for c in range(3):
                W1[(lane % 16)[ok], c, kh, kw[ok]] = fr[kh * 2 + h, ok, c]
    P["stem"] = (W1, vec(16))
    P["blocks"] = []
    for name, H, W, cin, cout, mid, Rr, _ in BLOCKS:
        b = {"name": name}
        b["c1w"], b["c1b"] = unfrag(mid // 16, cin // 16), vec(mid)
        b["g_w1"], b["g_b1"], b["g_w2"], b["g_b2"] = vec(Rr * mid).reshape(Rr, mid), vec(4)[:Rr], vec(Rr * mid).reshape(Rr, mid), vec(mid)
        b["c3w"], b["c3b"] = unfrag(cout // 16, mid // 16), vec(cout)
        b["dnw"] = unfrag(cout // 16, cin // 16) if cin != cout else None
        b["lights"] = [(unfrag(mid // 16, mid // 16), vec(mid * 9).reshape(mid // 8, 9, 8).transpose(0, 2, 1).reshape(mid, 3, 3).copy(), vec(mid)) for _ in range(10)]
        P["blocks"].append(b)
        if name in TRANS:
            tn, c = TRANS[name]
            P[tn] = (unfrag(c // 16, c // 16), vec(c))
    P["conv5"] = (unfrag(8, 8), vec(128))
    wt = take(64 * 512 * 4, f16).reshape(64, 512, 2).astype(f32)          # [channel pair][output][2]
    P["fc"] = (np.ascontiguousarray(wt.transpose(1, 0, 2).reshape(512, 128)), vec(512))
    assert pos[0] == len(buf), "the kernel's walk and the blob's length disagree"
    return P


# ------------------------------------------------------------------------------------------------ the tap buffer
def decode_taps(raw, layout):
    """raw (N, stride) uint8, layout [(name, offset, dtype 0 fp16 / 1 fp32 / 2 int64, h, w, c, pitch)] (y7t_reid_fused_tap_layout) -> {name: (N, h, w, c) array}"""
    out = {}
    for name, off, dt, h, w, c, pitch in layout:
        dtype = (f16, f32, np.int64)[dt]
        n = h * w * pitch
        a = raw[:, off:off + n * np.dtype(dtype).itemsize].copy().view(dtype).reshape(raw.shape[0], h, w, pitch)
        out[name] = a[..., :c]
    return out


# ------------------------------------------------------------------------------------------------ the staged references: each -> (ref, bound)
def f16_bar(ref, b):
    """the bar of an fp32 quantity with forward bound b stored as fp16 (module docstring)"""
    assert np.all(np.abs(ref) < 65504)
    return b + U16 * (np.abs(ref) + b) + 2.0 ** -25


def ref_cr(frames, boxes, idx):
    """CR: crop (int() corners clipped like a numpy slice) + / 255 + bilinear resize to 128 x 64 + Normalize, in the frame's channel order, 4th channel and the
    3-pixel halo zero; an empty crop is all zero.  frames (B, H, W, 3) uint8 -> (N, 134, 72, 4).  The geometry (fy, fx and the weights) is float32 on both sides, operation
    for operation, so the weights are the kernel's own; the blend is float64.  Bound: a term (1 - wy) (1 - wx) p k255 passes the roundings of k255 itself, p * k255,
    1 - wx, the product, the inner sum, 1 - wy, the product and the outer sum -> 8 u relative, all terms >= 0, so e_v = 8 u v; (v - mean) * isd adds two roundings
    (mean and isd = 1.0f / std are the same float32 constants on both sides): b = e_v isd + 2 u |ref|; then the fp16 store."""
    n = len(boxes)
    Hf, Wf = frames.shape[1:3]
    ref, bar = np.zeros((n, 134, 72, 4)), np.zeros((n, 134, 72, 4))
    mean, isd = f32([0.485, 0.456, 0.406]).astype(f64), (f32(1) / f32([0.229, 0.224, 0.225])).astype(f64)
    for i, b in enumerate(boxes):
        x1, y1, x2, y2 = (int(v) for v in b)
        x1, x2, y1, y2 = min(max(x1, 0), Wf), min(max(x2, 0), Wf), min(max(y1, 0), Hf), min(max(y2, 0), Hf)
        cw, ch = x2 - x1, y2 - y1
        if cw <= 0 or ch <= 0:
            continue
        img = frames[int(idx[i])][y1:y2, x1:x2].astype(f64) / 255.0
        fy = (np.arange(128, dtype=f32) + f32(0.5)) * f32(f32(ch) / f32(128)) - f32(0.5)
        fx = (np.arange(64, dtype=f32) + f32(0.5)) * f32(f32(cw) / f32(64)) - f32(0.5)
        y0, x0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
        wy, wx = (fy - y0.astype(f32)).astype(f64)[:, None, None], (fx - x0.astype(f32)).astype(f64)[None, :, None]
        yb, xb = np.clip(y0 + 1, 0, ch - 1), np.clip(x0 + 1, 0, cw - 1)
        y0, x0 = np.clip(y0, 0, ch - 1), np.clip(x0, 0, cw - 1)
        v = (1 - wy) * ((1 - wx) * img[y0][:, x0] + wx * img[y0][:, xb]) + wy * ((1 - wx) * img[yb][:, x0] + wx * img[yb][:, xb])
        r = (v - mean) * isd
        ref[i, 3:131, 3:67, :3] = r
        bar[i, 3:131, 3:67, :3] = f16_bar(r, 8 * U32 * v * isd + 2 * U32 * np.abs(r))
    return ref, bar


def _conv_bar(x, w, bias, k, s, relu):
    ref, ab, K = R.conv(x, w, bias, k, s, 0, relu)
    return ref, R.sum_bound(K, ab, ref)


def _w11(w):
    return np.asarray(w)[:, None, None, :]


def ref_c1(P, cr):
    """C1: the 7x7 / stride 2 stem + folded BN + ReLU over the haloed crop (columns 70, 71 of CR meet only zero weights) -> (N, 64, 32, 16), K = 147 + 1"""
    W, b = P["stem"]
    return _conv_bar(np.asarray(cr, f64)[:, :, :70, :3], W.transpose(0, 2, 3, 1), b, 7, 2, True)


def ref_x0(c1):
    """X0: MaxPool2d(3, 2, 1) with -inf padding (the kernel skips the padding: its inputs are >= 0); exact"""
    return R.maxpool3s2(c1), None


def ref_conv1x1(x, w, bias, relu):
    """a 1x1 convolution (x1, transition Y, conv5): K = CIN (+ 1 with a bias)"""
    return _conv_bar(x, _w11(w), bias, 1, 1, relu)


def ref_u(x, w):
    """U: the linear 1x1 of a LightConv3x3 inside a one-pixel zero ring -> (N, H + 2, W + 2, MID), K = MID"""
    ref, b = _conv_bar(x, _w11(w), None, 1, 1, False)
    pad = ((0, 0), (1, 1), (1, 1), (0, 0))
    return np.pad(ref, pad), np.pad(b, pad)


def ref_t(u, dw, db):
    """T: depthwise 3x3 + folded BN + ReLU read from the HALOED U as the device holds it (ring included) -> (N, H, W, MID), K = 10"""
    ref, ab, K = R.dwconv3(u, dw, db, True)
    ref, ab = ref[:, 1:-1, 1:-1], ab[:, 1:-1, 1:-1]
    return ref, R.sum_bound(K, ab, ref)


def ref_s(t_ref, t_bound):
    """S: dwconv3<GAP> sums its fp32 accumulators after the ReLU, BEFORE the fp16 conversion: the sum over the map of the unrounded relu(ref), off by at most the sum of
    T's fp32 bounds plus the bound of a length-NPX sum.  Compared with the device's eight per-wave partials summed -> (N, MID)"""
    s = t_ref.sum((1, 2))
    return s, t_bound.sum((1, 2)) + R.sum_bound(t_ref.shape[1] * t_ref.shape[2], s, s)


LOG2E_ERR = abs(float(f32(np.log2(np.e))) - np.log2(np.e)) / np.log2(np.e)      # relative error of the float32 constant log2(e): 0.22 u


def ref_gate(blk, S, npx):
    """gate[MID] = sigmoid(fc2(relu(fc1(pooled)))) with pooled = sum of the eight per-wave partials / NPX.  S (N, NW, MID) -> (ref (N, MID), bound).

    The sums: the partials are >= 0, so their fp32 sum is relatively accurate to 7 u and the scale by 1 / NPX (a power of two) is exact: pooled_err = 7 u pooled;
    fc1 is a chain of MID products + the bias, fc2 of R + the bias (op_refs.sum_bound), the first layer's error carried through |w2|: e_a.
    The exponential: op_refs.gate's "+ 4 u for expf and the division" was written for expf; this kernel calls __expf = 2^(a * log2e) on the hardware exponential.  With
    a the argument (|a| its size): the float32 constant log2(e) is off by LOG2E_ERR (relative) and the product a * log2e is rounded once (u), so the exponent is off
    by at most |a| log2(e) (u + LOG2E_ERR) in absolute terms, the result E = e^-a by that times ln 2, i.e. |a| (u + LOG2E_ERR) relative; the hardware exponential adds
    1 ulp = 2 u relative.  (No accuracy table of v_exp_f32 ships with this repository or its toolchain; 1 ulp is the figure AMD's CDNA instruction-set documents
    state for V_EXP_F32 and is ASSUMED here.  A result below 2^-126 may be flushed: absolute 2^-126.)  So rho = |a| (u + LOG2E_ERR) + 2 u, and through
    g = 1 / (1 + E), |dg/dE| = g (1 - g) / E <= 1 / (4 E): |dg| <= rho / 4.  1 + E and the division round once each (correctly rounded division): + 2 u g <= 2 u.
    Together with the sigmoid's slope <= 1/4 on e_a:   bound = e_a / 4 + (|a| (u + LOG2E_ERR) + 2 u) / 4 + 2 u + 2^-126."""
    S = np.asarray(S, f64)
    w1, b1, w2, b2 = (np.asarray(blk[k], f64) for k in ("g_w1", "g_b1", "g_w2", "g_b2"))
    Rr, C = w1.shape
    p = S.sum(1) / npx
    a1 = p @ w1.T + b1
    e1 = (7 * U32 * p) @ np.abs(w1).T + R.sum_bound(C + 1, p @ np.abs(w1).T + np.abs(b1), a1)
    h = np.maximum(a1, 0.0)
    a2 = h @ w2 + b2
    e2 = e1 @ np.abs(w2) + R.sum_bound(Rr + 1, h @ np.abs(w2) + np.abs(b2), a2)
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(-a2))
    return g, 0.25 * e2 + 0.25 * (np.abs(a2) * (U32 + LOG2E_ERR) + 2 * U32) + 2 * U32 + 2.0 ** -126


def gated_w3(c3w, gate, emulate_f16=True):
    """the A operands of conv3 for one stream: fp16(float32(w16) * gate_f32) per crop, exactly as acc_add<GATED> forms them (a float32 multiply, then a conversion that
    rounds to nearest even like the device's).  c3w (Co, MID) fp16 values, gate (N, MID) -> (N, Co, MID) float64.  emulate_f16=False: the plain product (chain())"""
    if not emulate_f16:
        return np.asarray(c3w, f64)[None] * np.asarray(gate, f64)[:, None, :]
    return (np.asarray(c3w, f32)[None] * np.asarray(gate, f32)[:, None, :]).astype(f16).astype(f64)


def ref_x(blk, xin, ts, gates, emulate_f16=True):
    """X: relu(sum_s (W3 * g_s) . t_s + [Wd . xin | xin] + bias), the block's output.  xin (N, H, W, CIN), ts four (N, H, W, MID), gates four (N, MID).
    K = 4 MID + CIN (downsample) or + 1 (identity), + 1 for the bias"""
    xin = np.asarray(xin, f64)
    ref, ab, K = 0.0, 0.0, 1
    for t, g in zip(ts, gates):
        w = gated_w3(blk["c3w"], g, emulate_f16)
        t = np.asarray(t, f64)
        ref = ref + np.einsum("nhwm,ncm->nhwc", t, w)
        ab = ab + np.einsum("nhwm,ncm->nhwc", np.abs(t), np.abs(w))
        K += t.shape[-1]
    if blk["dnw"] is not None:
        wd = np.asarray(blk["dnw"], f64)
        ref, ab, K = ref + xin @ wd.T, ab + np.abs(xin) @ np.abs(wd).T, K + xin.shape[-1]
    else:
        ref, ab, K = ref + xin, ab + np.abs(xin), K + 1
    bias = np.asarray(blk["c3b"], f64)
    ref, ab = np.maximum(ref + bias, 0.0), ab + np.abs(bias)
    return ref, R.sum_bound(K, ab, ref)


def ref_pool(y):
    """the transition's AvgPool2d(2): K = 4"""
    ref, ab, K = R.avgpool2(y)
    return ref, R.sum_bound(K, ab, ref)


def ref_v(y5):
    """v: the global average pool of conv5's output, fp32: K = 32"""
    y5 = np.asarray(y5, f64)
    ref, ab, K = R.gap(y5.reshape(y5.shape[0], -1, y5.shape[-1]))
    return ref, R.sum_bound(K, ab, ref)


def ref_feats(P, v):
    """feats: fc + folded BatchNorm1d + ReLU, fp32: K = 128 + 1"""
    ref, ab, K = R.fc(v, P["fc"][0], P["fc"][1], True)
    return ref, R.sum_bound(K, ab, ref)


# ------------------------------------------------------------------------------------------------ the walk over the tapped tensors
def staged(P, frames, boxes, idx, taps):
    """-> one (family, name, got, ref, bar) per comparison; bar None: got and ref must be array_equal.  Every reference reads the DEVICE's taps of its inputs."""
    T = taps
    n = len(boxes)

    def stored(fam, name, ref_bound):
        ref, b = ref_bound
        return fam, name, np.asarray(T[name], f64), ref, f16_bar(ref, b)

    def zero(name, got):
        return "zeros", name, np.asarray(got), np.zeros_like(np.asarray(got)), None

    ref, bar = ref_cr(frames, boxes, idx)
    yield "crop", "CR", np.asarray(T["CR"], f64), ref, bar
    halo = np.ones((134, 72), bool)
    halo[3:131, 3:67] = False
    yield zero("CR halo", T["CR"][:, halo])
    yield zero("CR 4th channel", T["CR"][..., 3])
    yield stored("stem", "C1", ref_c1(P, T["CR"]))
    yield "maxpool", "X0", np.asarray(T["X0"], f64), ref_x0(T["C1"])[0], None
    x = T["X0"]
    for blk, (name, H, W, cin, cout, mid, Rr, mid_real) in zip(P["blocks"], BLOCKS):
        yield stored("x1", name + ".x1", ref_conv1x1(x, blk["c1w"], blk["c1b"], True))
        if mid_real < mid:
            yield zero(name + ".x1 padded channels", T[name + ".x1"][..., mid_real:])
        ts, gates, l = [], [], 0
        for s in range(4):
            for j in range(s + 1):
                w, dw, db = blk["lights"][l]
                un, tn = "%s.light%d.U" % (name, l), "%s.light%d.T" % (name, l)
                yield stored("U", un, ref_u(T[name + ".x1"] if j == 0 else T["%s.light%d.T" % (name, l - 1)], w))
                ring = np.ones((H + 2, W + 2), bool)
                ring[1:-1, 1:-1] = False
                yield zero(un + " halo ring", T[un][:, ring])
                t_ref, t_b = ref_t(T[un], dw, db)
                yield stored("T", tn, (t_ref, t_b))
                if mid_real < mid:
                    yield zero(un + " padded channels", T[un][..., mid_real:])
                    yield zero(tn + " padded channels", T[tn][..., mid_real:])
                l += 1
            sn, gn = "%s.stream%d.S" % (name, s), "%s.stream%d.gate" % (name, s)
            S = np.asarray(T[sn], f64).reshape(n, NW, mid)
            s_ref, s_b = ref_s(t_ref, t_b)
            yield "S", sn, S.sum(1), s_ref, s_b
            g_ref, g_b = ref_gate(blk, S, H * W)
            yield "gate", gn, np.asarray(T[gn], f64).reshape(n, mid), g_ref, g_b
            ts.append(T[tn])
            gates.append(np.asarray(T[gn]).reshape(n, mid))
        yield stored("X", name + ".X", ref_x(blk, x, ts, gates))
        x = T[name + ".X"]
        if name in TRANS:
            tn, c = TRANS[name]
            yield stored("transition", tn + ".Y", ref_conv1x1(x, P[tn][0], P[tn][1], True))
            yield stored("transition", tn + ".pool", ref_pool(T[tn + ".Y"]))
            x = T[tn + ".pool"]
    yield stored("tail", "Y5", ref_conv1x1(x, P["conv5"][0], P["conv5"][1], True))
    ref, b = ref_v(T["Y5"])
    yield "tail", "v", np.asarray(T["v"], f64).reshape(n, 128), ref, b
    ref, b = ref_feats(P, np.asarray(T["v"], f64).reshape(n, 128))
    yield "tail", "feats", np.asarray(T["feats"], f64).reshape(n, 512), ref, b


def worst(got, ref, bar):
    """-> (ok, worst err / bar) of one comparison of staged()"""
    if bar is None:
        ok = got.shape == ref.shape and np.array_equal(got, ref)
        return ok, (0.0 if ok else np.inf)
    err = np.abs(got - ref)
    return bool(np.all(err <= bar)), (float(np.max(err / np.maximum(bar, 1e-300))) if err.size else 0.0)


def chain(P, x, trace=None):
    """the staged references chained from a float32 crop x (N, 3, 128, 64) WITHOUT teacher forcing and without fp16 stores -> (N, 512) float64: the network the
    references describe (== the oracle's, up to the fp16 rounding of the blob's weights).  trace: a dict that receives, per block, the gates (4, N, MID real) and the
    gate's hidden pre-activations (4, N, R) of this float64 network"""
    cr = np.zeros((x.shape[0], 134, 72, 4))
    cr[:, 3:131, 3:67, :3] = np.asarray(x, f64).transpose(0, 2, 3, 1)
    t = ref_x0(ref_c1(P, cr)[0])[0]
    for blk, (name, H, W, cin, cout, mid, Rr, _) in zip(P["blocks"], BLOCKS):      # (_: the real MID)
        x1 = ref_conv1x1(t, blk["c1w"], blk["c1b"], True)[0]
        ts, gates, l = [], [], 0
        for s in range(4):
            u = x1
            for j in range(s + 1):
                w, dw, db = blk["lights"][l]
                u, ub = ref_t(ref_u(u, w)[0], dw, db)
                l += 1
            ts.append(u)
            gates.append(ref_gate(blk, ref_s(u, ub)[0][:, None, :], H * W)[0])
            if trace is not None:
                trace.setdefault(name, ([], []))[0].append(gates[-1][:, :_])
                trace[name][1].append(u.mean((1, 2)) @ np.asarray(blk["g_w1"], f64).T + blk["g_b1"])
        t = ref_x(blk, t, ts, gates, emulate_f16=False)[0]
        if name in TRANS:
            t = ref_pool(ref_conv1x1(t, *P[TRANS[name][0]], True)[0])[0]
    return ref_feats(P, ref_v(ref_conv1x1(t, *P["conv5"], True)[0])[0])[0]


# ------------------------------------------------------------------------------------------------ the host emulation of the kernel
FAULTS = {
    # name: (the tensor of staged() that must trip, what is planted)
    "conv2.0 conv2a: right halo column of U = last image column": "conv2.0.light0.U halo ring",
    "conv3.1 conv2d.3: right halo column of U = last image column": "conv3.1.light9.U halo ring",
    "conv2.1 gate: channels 0 and 1 swapped": "conv2.1.stream0.gate",
    "conv2.1: stream 4 gated with stream 3's gate": "conv2.1.X",
    "conv3.1: stream 4 gated with stream 3's gate": "conv3.1.X",
    "conv4.1: stream 4 gated with stream 3's gate": "conv4.1.X",
    "conv3.1 gate: channels 0 and 1 swapped": "conv3.1.stream0.gate",
    "conv4.1 gate: channels 0 and 1 swapped": "conv4.1.stream0.gate",
    "conv2.0 conv2b.1: bottom halo row of U = last image row": "conv2.0.light2.U halo ring",
    "maxpool reads one column too few at the right edge": "X0",
    "conv3.2 pool: the last output column reads column 6 twice": "conv3.2.pool",
    "conv2.1: identity add dropped": "conv2.1.X",
    "conv4.0 stream 0: S summed over 7 of the 8 waves": "conv4.0.stream0.gate",
    "conv3.0: padded channel 24 of x1 non-zero": "conv3.0.x1 padded channels",
}


def emulate(P, frames, boxes, idx, seed=0, fault=None):
    """the kernel on the host: float32 arithmetic, every sum accumulated in a shuffled order, fp16 stores where the kernel stores -> the taps dict of decode_taps.
    fault: a key of FAULTS, planted where the kernel would have it (the tensors behind it follow from the faulty one, as on a device)"""
    assert fault is None or fault in FAULTS
    rng = np.random.default_rng(seed)
    n = len(boxes)
    T = {}

    def acc(terms):
        order = rng.permutation(terms.shape[-1])
        s = terms[..., order[0]].astype(f32)
        for k in order[1:]:
            s = s + terms[..., k]
        assert s.dtype == f32
        return s

    def c11(x, w, bias, relu):
        t = np.asarray(x, f32)[..., None, :] * np.asarray(w, f32)
        if bias is not None:
            t = np.concatenate([t, np.broadcast_to(np.asarray(bias, f32)[:, None], t.shape[:-1] + (1,))], -1)
        s = acc(t)
        return np.maximum(s, f32(0)) if relu else s

    # crop: the kernel's float32 expression
    Hf, Wf = frames.shape[1:3]
    cr = np.zeros((n, 134, 72, 4), f16)
    mean, isd, k255 = f32([0.485, 0.456, 0.406]), f32(1) / f32([0.229, 0.224, 0.225]), f32(0.00392156862745098)
    for i, b in enumerate(boxes):
        x1, y1, x2, y2 = (int(v) for v in b)
        x1, x2, y1, y2 = min(max(x1, 0), Wf), min(max(x2, 0), Wf), min(max(y1, 0), Hf), min(max(y2, 0), Hf)
        cw, ch = x2 - x1, y2 - y1
        if cw <= 0 or ch <= 0:
            continue
        img = frames[int(idx[i])][y1:y2, x1:x2].astype(f32) * k255
        fy = (np.arange(128, dtype=f32) + f32(0.5)) * f32(f32(ch) / f32(128)) - f32(0.5)
        fx = (np.arange(64, dtype=f32) + f32(0.5)) * f32(f32(cw) / f32(64)) - f32(0.5)
        y0, x0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
        wy, wx = (fy - y0.astype(f32))[:, None, None], (fx - x0.astype(f32))[None, :, None]
        yb, xb = np.clip(y0 + 1, 0, ch - 1), np.clip(x0 + 1, 0, cw - 1)
        y0, x0 = np.clip(y0, 0, ch - 1), np.clip(x0, 0, cw - 1)
        v = (f32(1) - wy) * ((f32(1) - wx) * img[y0][:, x0] + wx * img[y0][:, xb]) + wy * ((f32(1) - wx) * img[yb][:, x0] + wx * img[yb][:, xb])
        assert v.dtype == f32
        cr[i, 3:131, 3:67, :3] = ((v - mean) * isd).astype(f16)
    T["CR"] = cr
    # stem: implicit GEMM over (kh, kw, c)
    W1, b1 = P["stem"]
    patches = np.stack([cr[:, kh:kh + 127:2, kw:kw + 63:2, :3] for kh in range(7) for kw in range(7)], 3).reshape(n, 64, 32, 147)
    T["C1"] = c11(patches, W1.transpose(0, 2, 3, 1).reshape(16, 147), b1, True).astype(f16)
    c1 = T["C1"].astype(f64)
    if fault == "maxpool reads one column too few at the right edge":
        c1 = c1.copy()
        c1[:, :, 31] = 0.0                                         # (inputs are >= 0 and the kernel's running maximum starts at 0)
    T["X0"] = R.maxpool3s2(c1).astype(f16)
    x = T["X0"]
    for blk, (name, H, W, cin, cout, mid, Rr, mid_real) in zip(P["blocks"], BLOCKS):
        x1 = c11(x, blk["c1w"], blk["c1b"], True).astype(f16)
        if fault == "conv3.0: padded channel 24 of x1 non-zero" and name == "conv3.0":
            x1[..., 24] = f16(2.0 ** -24)                          # the smallest fp16 there is
        T[name + ".x1"] = x1
        ts, gates, l = [], [], 0
        for s in range(4):
            t = x1
            for j in range(s + 1):
                w, dw, db = blk["lights"][l]
                u = np.pad(c11(t, w, None, False).astype(f16), ((0, 0), (1, 1), (1, 1), (0, 0)))
                if fault in ("conv2.0 conv2a: right halo column of U = last image column", "conv3.1 conv2d.3: right halo column of U = last image column") and \
                        (name, l) == ((fault[:7]), 0 if "conv2a" in fault else 9):
                    u[:, :, -1] = u[:, :, -2]
                if fault == "conv2.0 conv2b.1: bottom halo row of U = last image row" and (name, l) == ("conv2.0", 2):
                    u[:, -1] = u[:, -2]
                T["%s.light%d.U" % (name, l)] = u
                uf = u.astype(f32)
                terms = np.stack([uf[:, kh:kh + H, kw:kw + W] * dw[:, kh, kw] for kh in range(3) for kw in range(3)] + [np.broadcast_to(db, (n, H, W, mid))], -1)
                a = np.maximum(acc(terms), f32(0))
                t = a.astype(f16)
                T["%s.light%d.T" % (name, l)] = t
                l += 1
            # the pooled partials of the stream's last light: the pixels dealt to eight waves
            px = a.reshape(n, H * W, mid)[:, rng.permutation(H * W)].reshape(n, NW, H * W // NW, mid)
            S = acc(px.transpose(0, 1, 3, 2))                      # (n, NW, mid)
            T["%s.stream%d.S" % (name, s)] = S.reshape(n, NW, 1, mid)
            part = S.transpose(0, 2, 1)
            if fault == "conv4.0 stream 0: S summed over 7 of the 8 waves" and (name, s) == ("conv4.0", 0):
                part = part[..., :7]
            pooled = acc(part) * f32(1.0 / (H * W))
            h = np.maximum(acc(np.concatenate([pooled[:, None, :] * blk["g_w1"], np.broadcast_to(blk["g_b1"][:, None], (n, Rr, 1))], -1)), f32(0))
            a2 = acc(np.concatenate([h[:, None, :] * blk["g_w2"].T, np.broadcast_to(blk["g_b2"][:, None], (n, mid, 1))], -1))
            with np.errstate(over="ignore"):                     # (e^-a = inf -> gate 0, on the device as well)
                g = f32(1) / (f32(1) + np.exp(-a2))
            assert g.dtype == f32
            if fault in ("conv2.1 gate: channels 0 and 1 swapped", "conv3.1 gate: channels 0 and 1 swapped", "conv4.1 gate: channels 0 and 1 swapped") and name == fault[:7]:
                g[:, [0, 1]] = g[:, [1, 0]]
            T["%s.stream%d.gate" % (name, s)] = g.reshape(n, 1, 1, mid)
            ts.append(t)
            gates.append(g)
        used = list(gates)
        if fault is not None and fault.endswith("stream 4 gated with stream 3's gate") and name == fault[:7]:
            used[3] = gates[2]
        terms = [t.astype(f32)[..., None, :] * gated_w3(blk["c3w"], g).astype(f32)[:, None, None] for t, g in zip(ts, used)]
        xf = np.asarray(x, f32)
        if blk["dnw"] is not None:
            terms.append(xf[..., None, :] * blk["dnw"])
        elif not (fault == "conv2.1: identity add dropped" and name == "conv2.1"):
            terms.append(xf[..., None])
        terms.append(np.broadcast_to(blk["c3b"][:, None], (n, H, W, cout, 1)))
        x = np.maximum(acc(np.concatenate(terms, -1)), f32(0)).astype(f16)
        T[name + ".X"] = x
        if name in TRANS:
            tn, c = TRANS[name]
            y = c11(x, P[tn][0], P[tn][1], True).astype(f16)
            T[tn + ".Y"] = y
            yf = y.astype(f32)
            cols = np.arange(W)
            if fault == "conv3.2 pool: the last output column reads column 6 twice" and tn == "conv3.2":
                cols[7] = 6
            yf = yf[:, :, cols].reshape(n, H // 2, 2, W // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, H // 2, W // 2, c, 4)
            x = (acc(yf) * f32(0.25)).astype(f16)
            T[tn + ".pool"] = x
    y5 = c11(x, P["conv5"][0], P["conv5"][1], True).astype(f16)
    T["Y5"] = y5
    v = acc(y5.astype(f32).reshape(n, 32, 128).transpose(0, 2, 1)) * f32(1.0 / 32.0)
    T["v"] = v.reshape(n, 1, 1, 128)
    T["feats"] = c11(v, P["fc"][0], P["fc"][1], True).reshape(n, 1, 1, 512)
    return T
