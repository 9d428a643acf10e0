"""Plain numpy references of the general OSNet path (csrc/y7t_reid_osnet.hip; tracker/reid.py::lower_osnet_f16), ONE OP AT A TIME, in the style of
tests/reid_fused_ref.py: they reuse tests/op_refs.py (conv, dwconv3, avgpool2, gap, fc, gate, maxpool3s2, sum_bound) and add the instance norm and the gated sum.

Everything here is driven by an OP LIST (include/y7t.h: y7t_reid_op) and its weight blob, decoded back into matrices by `decode` -- so the references also check
the lowering and the fragment packing: what the device is given is what is interpreted.

  chain(ops, w, crops)       the op list in float64 without fp16 stores: == the reference module up to the fp16 rounding of the stored weights
  emulate(ops, w, crops)     float32 accumulation, fp16 stores at exactly the device's storage points -> (features, buffers); fault=... plants one defect
  staged(ops, w, bufs, n)    TEACHER-FORCED: every op's float64 reference from the buffers the op actually read (the device's, or emulate()'s), with its bar

Storage points (fp16 roundings) of the device: the crop pixel as the stem reads it; the stem's conv + bias; every pointwise output (after the residual / ReLU);
inside a LightConv3x3 the 1x1's output (LDS) and the depthwise output; the gated sum x2; every instance-norm output; the 2x2 average; the pooled vector of the
tail.  fp32: the per-strip channel sums, the gates, the features.

Bars (derived, never tuned; u = 2^-24).  An fp32 quantity with forward bound b = sum_bound(K, sum|terms|, ref) stored as fp16: reid_fused_ref.f16_bar,
    b + 2^-11 (|ref| + b) + 2^-25.
LightConv3x3 is two stored stages, of which only the second is visible: the 1x1's bar e_t (K = midp) is carried through the depthwise taps,
    b = sum_taps |w| e_t + sum_bound(10, sum|terms|, ref).
Instance norm (derivation in `instnorm`)."""
import numpy as np

from tests import op_refs as R
from tests.reid_fused_ref import f16_bar
from yolov7_tracker_amd.tracker import reid

U32 = R.U32
f16, f32, f64 = np.float16, np.float32, np.float64
IN_EPS = 1e-5
FAULTS = ["halo_wrong_side", "halo_clamped", "gate_shift", "unbiased_var", "no_relu_pool", "pad_nonzero"]


# ------------------------------------------------------------------------------------------------ the blob
def _unfrag(w, off, ng, nk):
    fr = w[off:off + ng * nk * 128].view(f16).reshape(ng, nk, 64, 4).astype(f64)
    M = np.zeros((ng * 16, nk * 16))
    lane = np.arange(64)
    for g in range(ng):
        for k in range(nk):
            for e in range(4):
                M[g * 16 + lane % 16, k * 16 + 4 * (lane // 16) + e] = fr[g, k, :, e]
    return M


def _unfrag_stem(w, off, ng):
    fr = w[off:off + ng * 14 * 128].view(f16).reshape(ng, 14, 64, 4).astype(f64)
    W1 = np.zeros((ng * 16, 7, 7, 3))                        # (Co, kh, kw, Ci): op_refs.conv's layout
    lane = np.arange(64)
    for g in range(ng):
        for kh in range(7):
            for h in range(2):
                kw = 4 * h + lane // 16
                ok = kw < 7
                assert not fr[g, kh * 2 + h, ~ok].any() and not fr[g, kh * 2 + h, :, 3].any()
                for c in range(3):
                    W1[g * 16 + (lane % 16)[ok], kh, kw[ok], c] = fr[g, kh * 2 + h, ok, c]
    return W1


def decode(op, w):
    """the parameters of one op, float64"""
    t, C, Co = int(op["type"]), int(op["C"]), int(op["Co"])
    wo, bo = int(op["w_off"]), int(op["b_off"])
    vec = lambda off, n: w[off:off + n].astype(f64)
    if t == reid.H_OS_STEM:
        return {"w": _unfrag_stem(w, wo, Co // 16), "b": vec(bo, Co)}
    if t in (reid.H_OS_PW, reid.H_OS_GAPFC):
        P = {"w": _unfrag(w, wo, Co // 16, C // 16), "b": vec(bo, Co)}
        if t == reid.H_OS_PW and int(op["k"]) == reid.RES_GEMM:
            P["w2"] = _unfrag(w, int(op["w2_off"]), Co // 16, int(op["s"]) // 16)
        return P
    if t == reid.H_OS_LIGHT:
        per = C * C // 2 + 10 * C
        return {"slots": [{"w": _unfrag(w, wo + s * per, C // 16, C // 16), "dw": vec(wo + s * per + C * C // 2, 9 * C).reshape(3, 3, C).transpose(2, 0, 1).copy(),
                           "b": vec(wo + s * per + C * C // 2 + 9 * C, C)} for s in range(int(op["s"]))]}
    if t == reid.H_OS_GATESUM:
        Rr = int(op["R"])
        return {"w1": vec(wo, Rr * C).reshape(Rr, C), "b1": vec(bo, Rr), "w2": vec(int(op["w2_off"]), C * Rr).reshape(C, Rr), "b2": vec(int(op["b2_off"]), C)}
    if t in (reid.H_OS_INSTNORM, reid.INSTNORM):
        return {"g": vec(wo, C), "b": vec(bo, C)}
    return {}


def real_channels(spec):
    """real (unpadded) output channels of every op of lower_osnet_f16, in op order"""
    ch, out = spec["channels"], []
    out += [ch[0]] + ([ch[0]] if spec.get("ibn") else []) + [ch[0]]
    for si, (cin, cout, nblk) in enumerate(zip(ch[:-1], ch[1:], spec["layers"])):
        for bi in range(nblk):
            out += [cout // 4] * 6 + [cout] + ([cout] if spec.get("ibn") and si == 0 else [])
        if si < 2:
            out += [cout, cout]
    return out + [ch[3], spec["feature_dim"]]


# ------------------------------------------------------------------------------------------------ buffers: raw float32 words per crop <-> typed views
def halves(raw, shape):
    return np.ascontiguousarray(raw).view(f16).reshape((raw.shape[0],) + tuple(shape))


def words(a):
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(f32)


def strips_of(op):
    S = reid.os_strip_rows(int(op["H"]), int(op["W"]), int(op["C"]), int(op["p"]))
    return S, (int(op["H"]) + S - 1) // S


# ------------------------------------------------------------------------------------------------ per-op float64 references: -> (ref, fp32 forward bound)
def stem(x32, P):
    """crop pixels rounded to fp16, 7x7 / 2 / 3 conv + bias"""
    ref, ab, K = R.conv(x32.astype(f16), P["w"], P["b"], 7, 2, 3, False)
    return ref, R.sum_bound(K, ab, ref)


def pw(x, P, relu, res=None, x2=None):
    x = np.asarray(x, f64)
    ref = x @ P["w"].T + P["b"]
    ab = np.abs(x) @ np.abs(P["w"]).T + np.abs(P["b"])
    K = x.shape[-1] + 1
    if x2 is not None:
        x2 = np.asarray(x2, f64)
        ref, ab, K = ref + x2 @ P["w2"].T, ab + np.abs(x2) @ np.abs(P["w2"]).T, K + x2.shape[-1]
    if res is not None:
        ref, ab, K = ref + np.asarray(res, f64), ab + np.abs(np.asarray(res, f64)), K + 1
    b = R.sum_bound(K, ab, ref)
    return (np.maximum(ref, 0.0) if relu else ref), b


def light(x, Ps):
    """LightConv3x3: 1x1 (stored fp16), depthwise 3x3 + bias + ReLU -> (ref, bound) (module docstring)"""
    x = np.asarray(x, f64)
    t = x @ Ps["w"].T
    e_t = f16_bar(t, R.sum_bound(x.shape[-1], np.abs(x) @ np.abs(Ps["w"]).T, t))
    ref, ab, K = R.dwconv3(t, Ps["dw"], Ps["b"], True)
    carried, _, _ = R.dwconv3(e_t, np.abs(Ps["dw"]), np.zeros_like(Ps["b"]), False)
    return ref, carried + R.sum_bound(K, ab, ref)


def strip_sums(y, S):
    """per-strip channel sums of the stored output.  y (N, H, W, C) -> (ref (N, strips, C), bound)"""
    y = np.asarray(y, f64)
    H = y.shape[1]
    ref = np.stack([y[:, r:r + S].sum((1, 2)) for r in range(0, H, S)], 1)
    ab = np.stack([np.abs(y[:, r:r + S]).sum((1, 2)) for r in range(0, H, S)], 1)
    return ref, R.sum_bound(S * y.shape[2], ab, ref)


def gatesum(xb, part, HW, P):
    """xb: the four finished branches [(N, H, W, C)] * 4, part (N, 4, strips, C) -> (ref, bound): pooled = sum of the strips / HW, the gate MLP (op_refs.gate with the
    pooled vector's own bound carried), x2 = sum_b gate_b x2_b with the gates' bounds carried (|x| e_gate) + the 4-term sum bound"""
    part = np.asarray(part, f64)
    pooled = part.sum(2) / HW
    e_p = R.sum_bound(part.shape[2], np.abs(part).sum(2) / HW, pooled)
    ref, ab, e = 0.0, 0.0, 0.0
    for b in range(4):
        g, e_g = R.gate(pooled[:, b], P["w1"], P["b1"], P["w2"], P["b2"], e_p[:, b])
        x = np.asarray(xb[b], f64)
        v = x * g[:, None, None, :]
        ref, ab, e = ref + v, ab + np.abs(v), e + np.abs(x) * e_g[:, None, None, :]
    return ref, e + R.sum_bound(4, ab, ref)


def instnorm(x, P, relu, unbiased=False):
    """InstanceNorm2d(affine, eps) over (N, H, W, C) in fp32, two-pass -> (ref, bound).  With u = 2^-24, HW = n, d = x - m, s = 1 / sqrt(v + eps):
      mean      m^ = fl(sum x / n):                          e_m = sum_bound(n, mean|x|, m)
      centred   d^ = fl(x - m^):                             |d^ - d| <= delta = e_m + u (|d| + e_m)
      variance  v^ = fl(sum d^2 / n), each square rounded:   e_v = mean(2 |d| delta + delta^2) + sum_bound(n + 1, mean(d^2 + 2 |d| delta + delta^2), v)
      scale     s^ = fl(1 / fl(sqrt(fl(v^ + eps)))):         e_s = e_v / 2 (max(v - e_v, 0) + eps)^(-3/2) + 3 u s     (|ds/dv| is largest at the low end)
      output    fl(fl(fl(d^ s^) gamma) + beta):              e_y = |gamma| (delta (s + e_s) + |d| e_s) + 3 u (|d s gamma| + |beta|) + u |y|
    ReLU is 1-Lipschitz.  A constant channel has d = 0, v = 0, s = eps^(-1/2): the bound stays finite."""
    x = np.asarray(x, f64)
    n = x.shape[1] * x.shape[2]
    m = x.mean((1, 2), keepdims=True)
    e_m = R.sum_bound(n, np.abs(x).mean((1, 2), keepdims=True), m)
    d = x - m
    v = (d * d).mean((1, 2), keepdims=True) * (n / (n - 1.0) if unbiased else 1.0)
    delta = e_m + U32 * (np.abs(d) + e_m)
    sq = 2 * np.abs(d) * delta + delta * delta
    e_v = sq.mean((1, 2), keepdims=True) + R.sum_bound(n + 1, (d * d + sq).mean((1, 2), keepdims=True), v)
    s = 1.0 / np.sqrt(v + IN_EPS)
    e_s = 0.5 * e_v * (np.maximum(v - e_v, 0.0) + IN_EPS) ** -1.5 + 3 * U32 * s
    y = d * s * P["g"] + P["b"]
    e_y = np.abs(P["g"]) * (delta * (s + e_s) + np.abs(d) * e_s) + 3 * U32 * (np.abs(d * s * P["g"]) + np.abs(P["b"])) + U32 * np.abs(y)
    return (np.maximum(y, 0.0) if relu else y), e_y


def gapfc(x, P, relu):
    """mean over the map, stored fp16, then the fc -> (pooled ref, pooled bar, features ref, features bound with the pooled bar carried)"""
    x = np.asarray(x, f64)
    v, ab, K = R.gap(x.reshape(x.shape[0], -1, x.shape[-1]))
    e_v = f16_bar(v, R.sum_bound(K, ab, v))
    return v, e_v, lambda vhat: _fc(vhat, P, relu)


def _fc(v, P, relu):
    ref, ab, K = R.fc(v, P["w"], P["b"], relu)
    return ref, R.sum_bound(K, ab, ref)


# ------------------------------------------------------------------------------------------------ walking an op list
def _dims(op):
    return tuple(int(op[k]) for k in ("H", "W", "C", "Ho", "Wo", "Co"))


def staged(ops, w, bufs, n):
    """teacher-forced comparisons: yields (op index, label, got, ref, bar) -- bar None: exact.  bufs: {buffer index: (n, floats per crop) float32 raw words}"""
    for i, op in enumerate(ops):
        t = int(op["type"])
        H, W, C, Ho, Wo, Co = _dims(op)
        P = decode(op, w)
        xin, out, aux = bufs[int(op["in_buf"])], bufs[int(op["out_buf"])], (bufs[int(op["aux_buf"])] if int(op["aux_buf"]) >= 0 else None)
        if t == reid.H_OS_STEM:
            ref, b = stem(xin[:, :H * W * 3].reshape(n, H, W, 3), P)
            yield i, "stem", halves(out, (Ho, Wo, Co)), ref, f16_bar(ref, b)
        elif t == reid.H_MAXPOOL_RELU:
            yield i, "maxpool", halves(out, (Ho, Wo, Co)), R.maxpool3s2(halves(xin, (H, W, C)), relu_first=True).astype(f16), None
        elif t == reid.H_OS_PW:
            mode = int(op["k"])
            x = halves(xin, (H, W, C))
            ref, b = pw(x, P, int(op["relu"]) & 1, res=halves(aux, (H, W, Co)) if mode == reid.RES_ADD else None,
                        x2=halves(aux, (H, W, int(op["s"]))) if mode == reid.RES_GEMM else None)
            yield i, "pw", halves(out, (H, W, Co)), ref, f16_bar(ref, b)
        elif t == reid.H_OS_LIGHT:
            lev, nb = int(op["k"]), int(op["s"])
            S, strips = strips_of(op)
            T = halves(out, (reid.OS_SLOTS, H, W, C))
            for s in range(nb):
                x = halves(xin, (H, W, C)) if lev == 0 else halves(xin, (reid.OS_SLOTS, H, W, C))[:, reid.os_level_slot(lev - 1) + s + 1]
                ref, b = light(x, P["slots"][s])
                got = T[:, reid.os_level_slot(lev) + s]
                yield i, "light L%d s%d" % (lev, s), got, ref, f16_bar(ref, b)
                if s == 0:
                    ref, b = strip_sums(got, S)
                    yield i, "sums L%d" % lev, aux.reshape(n, 4, strips, C)[:, lev], ref, b
        elif t == reid.H_OS_GATESUM:
            S, strips = strips_of(op)
            T = halves(xin, (reid.OS_SLOTS, H, W, C))
            ref, b = gatesum([T[:, reid.os_level_slot(k)] for k in range(4)], aux.reshape(n, 4, strips, C), H * W, P)
            yield i, "gatesum", halves(out, (H, W, C)), ref, f16_bar(ref, b)
        elif t == reid.H_OS_INSTNORM:
            ref, b = instnorm(halves(xin, (H, W, C)), P, int(op["relu"]))
            yield i, "instnorm", halves(out, (H, W, C)), ref, f16_bar(ref, b)
        elif t == reid.INSTNORM:
            x = xin.reshape(n, H, W, C) if aux is None else xin.reshape(n, H, W, C) + aux.reshape(n, H, W, C)       # float32: the kernel's one rounding
            ref, b = instnorm(x, P, int(op["relu"]))
            yield i, "instnorm32", out.reshape(n, H, W, C), ref, b
        elif t == reid.H_OS_AVGPOOL:
            ref, ab, K = R.avgpool2(halves(xin, (H, W, C)))
            yield i, "avgpool", halves(out, (Ho, Wo, C)), ref, f16_bar(ref, R.sum_bound(K, ab, ref))
        elif t == reid.H_OS_GAPFC:
            v, e_v, fc = gapfc(halves(xin, (H, W, C)), P, int(op["relu"]))
            vhat = halves(aux, (C,))
            yield i, "gap", vhat, v, e_v
            ref, b = fc(vhat)                                   # teacher-forced from the stored vector
            yield i, "fc", out[:, :Co], ref, b
        else:
            raise ValueError("op type %d has no reference here" % t)


def pads_nonzero(ops, bufs, n, real):
    """-> [(op index, count)] of non-zero values in the pad channels of every fp16 map an op wrote"""
    bad = []
    for i, (op, c) in enumerate(zip(ops, real)):
        t, H, W, Co = int(op["type"]), int(op["Ho"]) or int(op["H"]), int(op["Wo"]) or int(op["W"]), int(op["Co"])
        if t == reid.H_OS_GAPFC or c == Co:
            continue
        if t == reid.H_OS_LIGHT:
            a = halves(bufs[int(op["out_buf"])], (reid.OS_SLOTS, H, W, Co))[:, reid.os_level_slot(int(op["k"])):reid.os_level_slot(int(op["k"])) + int(op["s"])]
        else:
            a = halves(bufs[int(op["out_buf"])], (H, W, Co))
        k = int(np.count_nonzero(a[..., c:]))
        if k:
            bad.append((i, k))
    return bad


def _run(ops, w, crops, emu, fault=None):
    """chain (emu False: float64, no stores) or the emulation (float32 accumulation, fp16 stores).  -> (features (N, fd) float64, typed buffers)"""
    n = crops.shape[0]
    acc = f32 if emu else f64
    st = (lambda a: np.asarray(a, f32).astype(f16)) if emu else (lambda a: np.asarray(a, f64))
    mm = lambda x, Wm: np.asarray(x, acc) @ np.asarray(Wm, acc).T
    B = {int(ops[0]["in_buf"]): np.asarray(crops, f32)}
    feats = None
    n_pw = 0
    for op in ops:
        t = int(op["type"])
        H, W, C, Ho, Wo, Co = _dims(op)
        P = decode(op, w)
        x = B[int(op["in_buf"])]
        aux = B.get(int(op["aux_buf"]))
        if t == reid.H_OS_STEM:
            xi = st(x)
            y = np.zeros((n, Ho, Wo, Co), acc) + P["b"].astype(acc)
            xp = np.pad(np.asarray(xi, acc), ((0, 0), (3, 3), (3, 3), (0, 0)))
            for kh in range(7):
                for kw in range(7):
                    y = y + mm(xp[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2], P["w"][:, kh, kw])
            B[int(op["out_buf"])] = st(y)
        elif t == reid.H_MAXPOOL_RELU:
            y = R.maxpool3s2(np.asarray(x, f64), relu_first=fault != "no_relu_pool")
            B[int(op["out_buf"])] = st(y)
        elif t == reid.H_OS_PW:
            mode = int(op["k"])
            y = mm(x, P["w"]) + P["b"].astype(acc)
            if fault == "pad_nonzero" and n_pw == 0 and not P["w"][-1].any() and P["b"][-1] == 0:
                y[..., -1] += acc(0.25)                          # the first pointwise output that has a pad channel
                n_pw += 1
            if mode == reid.RES_GEMM:
                y = y + mm(aux, P["w2"])
            elif mode == reid.RES_ADD:
                y = y + np.asarray(aux, acc)
            B[int(op["out_buf"])] = st(np.maximum(y, 0) if int(op["relu"]) & 1 else y)
        elif t == reid.H_OS_LIGHT:
            lev, nb = int(op["k"]), int(op["s"])
            S, strips = strips_of(op)
            T = B.setdefault(int(op["out_buf"]), np.zeros((n, reid.OS_SLOTS, H, W, C), f16 if emu else f64))
            part = B.setdefault(int(op["aux_buf"]), np.zeros((n, 4, strips, C), acc))
            for s in range(nb):
                xs = x if lev == 0 else x[:, reid.os_level_slot(lev - 1) + s + 1]
                Ps = P["slots"][s]
                t_full = np.asarray(st(mm(xs, Ps["w"])), acc)                      # the 1x1 of every row (each strip recomputes its halo rows: same values)
                for k in range(strips):
                    r0 = k * S
                    rows = min(S, H - r0)
                    img = np.zeros((n, rows + 2, W + 2, C), acc)
                    for i in range(rows + 2):
                        y = r0 - 1 + i
                        if fault == "halo_wrong_side" and strips > 1 and i in (0, rows + 1):
                            y = r0 - S if i == 0 else r0 + rows + S - 1             # the neighbouring strip's far side
                        if fault == "halo_clamped":
                            y = min(max(y, 0), H - 1)
                        if 0 <= y < H:
                            img[:, i, 1:W + 1] = t_full[:, y]
                    if fault == "halo_clamped":
                        img[:, :, 0], img[:, :, W + 1] = img[:, :, 1], img[:, :, W]
                    a = np.zeros((n, rows, W, C), acc) + Ps["b"].astype(acc)
                    for kh in range(3):
                        for kw in range(3):
                            a = a + img[:, kh:kh + rows, kw:kw + W] * Ps["dw"][:, kh, kw].astype(acc)
                    o = st(np.maximum(a, 0))
                    T[:, reid.os_level_slot(lev) + s, r0:r0 + rows] = o
                    if s == 0:
                        part[:, lev, k] = np.asarray(o, acc).sum((1, 2), dtype=acc)
        elif t == reid.H_OS_GATESUM:
            part = np.asarray(aux, acc)
            pooled = part.sum(2) / acc(H * W)
            hid = np.maximum(pooled @ P["w1"].T.astype(acc) + P["b1"].astype(acc), 0)
            g = 1 / (1 + np.exp(-(hid @ P["w2"].T.astype(acc) + P["b2"].astype(acc))))          # (n, 4, C)
            g = np.asarray(g, acc)
            if fault == "gate_shift":
                g = np.roll(g, 1, axis=1)
            y = 0
            for b in range(4):
                y = y + np.asarray(x[:, reid.os_level_slot(b)], acc) * g[:, b, None, None, :]
            B[int(op["out_buf"])] = st(y)
        elif t in (reid.H_OS_INSTNORM, reid.INSTNORM):
            xa = np.asarray(x, acc).reshape(n, H, W, C)
            if aux is not None:
                xa = xa + np.asarray(aux, acc).reshape(n, H, W, C)
            hw = H * W
            m = xa.mean((1, 2), keepdims=True, dtype=acc)
            v = ((xa - m) ** 2).mean((1, 2), keepdims=True, dtype=acc)
            if fault == "unbiased_var" and hw > 1:
                v = v * acc(hw / (hw - 1.0))
            y = (xa - m) * (1 / np.sqrt(v + acc(IN_EPS))) * P["g"].astype(acc) + P["b"].astype(acc)
            y = np.maximum(y, 0) if int(op["relu"]) else y
            B[int(op["out_buf"])] = st(y) if t == reid.H_OS_INSTNORM else np.asarray(y, acc)
        elif t == reid.H_OS_AVGPOOL:
            xa = np.asarray(x, acc)
            B[int(op["out_buf"])] = st((xa[:, 0::2, 0::2] + xa[:, 0::2, 1::2] + xa[:, 1::2, 0::2] + xa[:, 1::2, 1::2]) * acc(0.25))
        elif t == reid.H_OS_GAPFC:
            v = st(np.asarray(x, acc).reshape(n, H * W, C).mean(1, dtype=acc))
            B[int(op["aux_buf"])] = v
            y = mm(v, P["w"]) + P["b"].astype(acc)
            feats = np.asarray(np.maximum(y, 0) if int(op["relu"]) else y, acc)
            B[int(op["out_buf"])] = feats
        else:
            raise ValueError("op type %d is not part of the fp16 OSNet list" % t)
    return np.asarray(feats, f64), B


def chain(ops, w, crops):
    return _run(ops, w, crops, False)[0]


def emulate(ops, w, crops, fault=None):
    """-> (features float64, {buffer index: raw float32 words per crop}) -- the form `staged` and `pads_nonzero` read"""
    feats, B = _run(ops, w, crops, True, fault)
    return feats, {k: words(v) for k, v in B.items()}


def rel_l2(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def worst(ops, w, bufs, n):
    """-> [(op index, label, worst err / bar or mismatches)] of staged(): ratio > 1 = over the bar"""
    out = []
    for i, label, got, ref, bar in staged(ops, w, bufs, n):
        if bar is None:
            out.append((i, label, float("inf") if not np.array_equal(np.asarray(got), np.asarray(ref)) else 0.0))
        else:
            err = np.abs(np.asarray(got, f64) - ref)
            out.append((i, label, float(np.max(err / np.maximum(bar, 1e-300)))))
    return out
