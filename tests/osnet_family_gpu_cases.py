"""GPU cases of tests/test_osnet_family_gpu.py, which runs this file in a process of its own (see there): the general OSNet path (csrc/y7t_reid_osnet.hip; DESIGN.md section 4 "OSNet family") -- one-op plans, whole networks, behaviour.

One-op plans are TEACHER-FORCED like tests/test_reid_ops_gpu.py: the op reads the fp16 tensors the test put into the arena, the float64 reference of
tests/osnet_f16_ref.py::staged reads the same tensors, the bar is that op's own derived bar (osnet_f16_ref's docstring; nothing tuned).  The arena is a sentinel
outside the buffers and between them, and must stay one.  After every op the pad channels of its output must be exactly zero.

Whole networks run on the fixture crops of tests/golden/osnet_family_<name>.npz (float64 embeddings of the reference module).  Every stored tensor of the
device is compared, at its own bar, with its reference computed from the device's own input buffers; end to end the device's relative L2 error against the
fixture must be at most 2 D_emu, D_emu being the error of the CPU emulation (it shares the rounding points, not the summation order).  MARGIN / NET lines are kept
in profiles/osnet_family_margins.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import op_refs as R
from tests import osnet_f16_ref as O
from yolov7_tracker_amd.tracker import reid

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 7.0
f16, f32, f64 = np.float16, np.float32, np.float64
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


class Plan:
    """an op list over an arena the test owns: 64 sentinel floats around every buffer"""

    def __init__(self, L, ops, per_crop, w, n, in_h, in_w, feat_dim, max_crops=None):
        from yolov7_tracker_amd import _lib
        self.L, self.n, self.per_crop = L, n, [int(b) for b in per_crop]
        self.max_crops = max_crops or n
        self.ops = np.ascontiguousarray(ops)
        offs, o = [], 64
        for b in self.per_crop:
            offs.append(o)
            o += (b * self.max_crops + 63) // 64 * 64 + 64
        self.offs = np.array(offs, dtype=np.int64)
        self.arena = torch.full((o,), SENTINEL, dtype=torch.float32, device="cuda")
        self.w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32).reshape(-1)).cuda()
        self.feat_dim, self.in_h, self.in_w = int(feat_dim), in_h, in_w
        self.h = ctypes.c_void_p()
        rc = L.y7t_reid_create(self.ops.ctypes.data_as(ctypes.c_void_p), len(self.ops), self.offs.ctypes.data_as(ctypes.c_void_p), len(offs), _lib.ptr(self.arena),
                               self.arena.numel() * 4, _lib.ptr(self.w), self.max_crops, in_h, in_w, self.feat_dim, ctypes.byref(self.h))
        assert rc == 0, (rc, L.y7t_last_error())

    def fill(self, buf, raw):
        """raw: (n, floats per crop) float32 words"""
        t = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).cuda().reshape(-1)
        assert t.numel() == self.n * self.per_crop[buf], (t.numel(), self.n, self.per_crop[buf])
        o = int(self.offs[buf])
        self.arena[o:o + t.numel()] = t

    def read(self, buf):
        o = int(self.offs[buf])
        return self.arena[o:o + self.n * self.per_crop[buf]].cpu().numpy().reshape(self.n, self.per_crop[buf])

    def run(self, crops=None):
        from yolov7_tracker_amd import _lib
        x = torch.zeros(self.n * self.in_h * self.in_w * 3, dtype=torch.float32, device="cuda") if crops is None else torch.from_numpy(np.ascontiguousarray(crops, dtype=np.float32)).cuda()
        feats = torch.full((self.n * self.feat_dim + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(self.L.y7t_reid_forward(self.h, None, 0, 0, None, self.n, _lib.ptr(x), _lib.ptr(feats), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((feats[self.n * self.feat_dim:] == SENTINEL).all())
        keep = torch.ones(self.arena.numel(), dtype=torch.bool, device="cuda")
        for b, o in zip(self.per_crop, self.offs):
            keep[int(o):int(o) + b * self.n] = False
        assert bool((self.arena[keep] == SENTINEL).all()), "an op wrote outside the buffers of its %d crops" % self.n
        return feats[:self.n * self.feat_dim].view(self.n, self.feat_dim).cpu().numpy()

    def bufs(self):
        return {b: self.read(b) for b in range(len(self.per_crop))}

    def close(self):
        if self.h:
            self.L.y7t_reid_destroy(self.h)
            self.h = None


def mk_ops(dicts):
    ops = np.zeros(len(dicts), reid.OP_DTYPE)
    for o, kw in zip(ops, dicts):
        o["aux_buf"], o["b_off"] = -1, -1
        for k, v in kw.items():
            o[k] = v
    return ops


class Blob:
    """weight pieces at 16-byte aligned float offsets"""

    def __init__(self):
        self.parts, self.n = [], 0

    def put(self, raw):
        a = np.frombuffer(raw, dtype=f32) if isinstance(raw, (bytes, bytearray)) else np.asarray(raw, f32).reshape(-1)
        if self.n % 4:
            pad = 4 - self.n % 4
            self.parts.append(np.zeros(pad, f32)); self.n += pad
        off = self.n
        self.parts.append(a); self.n += a.size
        return off

    def array(self):
        return np.concatenate(self.parts + [np.zeros(4, f32)])


def act(rng, shape, real, scale=1.0):
    """fp16 activations whose pad channels (>= real) are zero"""
    a = rng.normal(0, scale, shape).astype(f16)
    a[..., real:] = 0
    return a


def padded(M, rows, cols):
    out = np.zeros((rows, cols))
    out[:M.shape[0], :M.shape[1]] = M
    return out


def check(kernel, case, ops, w, bufs, n, real=None):
    """every staged comparison of the plan at its bar, MARGIN lines, pads zero"""
    worst = 0.0
    for i, label, got, ref, bar in O.staged(ops, w, bufs, n):
        if bar is None:
            assert np.array_equal(np.asarray(got), np.asarray(ref)), "%s %s %s: %d values differ" % (kernel, case, label, int((np.asarray(got) != np.asarray(ref)).sum()))
            continue
        err = np.abs(np.asarray(got, f64) - ref)
        ratio = float(np.max(err / np.maximum(bar, 1e-300)))
        worst = max(worst, ratio)
        assert np.all(err <= bar), "%s %s %s: %d values over the bar, worst err/bar %.2f" % (kernel, case, label, int((err > bar).sum()), ratio)
    print("MARGIN %-18s %-52s worst err/bar %.3f" % (kernel, case, worst))
    if real is not None:
        assert O.pads_nonzero(ops, bufs, n, real) == [], "%s %s: non-zero pad channels" % (kernel, case)
    return worst


# ------------------------------------------------------------------------------------------------ one-op plans
def light_params(rng, mid, midp):
    Wm = rng.normal(0, (1.0 / mid) ** 0.5, (mid, mid))
    dw = np.zeros((9, midp)); dw[:, :mid] = rng.normal(0, 1 / 3.0, (9, mid))
    b = np.zeros(midp); b[:mid] = rng.normal(0, 0.1, mid)
    return reid._frags(Wm, midp, midp) + reid._f32(dw) + reid._f32(b)


@pytest.mark.parametrize("mid", [16, 24, 72])
@pytest.mark.parametrize("H,W", [(7, 4), (4, 1), (5, 16)])
def test_light_level(L, H, W, mid):
    """levels 0 (four branches from one input) and 2 (two branches from the branch buffer), strip rows 1, 3, 5 and auto: every strip boundary of the tiny map, the
    zero halo, the per-strip sums of slot 0"""
    n, midp = 3, reid.pad16(mid)
    rng = R.rng_for("light", H, W, mid)
    for level, nb in ((0, 4), (2, 2)):
        for strip in (1, 3, 5, 0):
            S = reid.os_strip_rows(H, W, midp, strip)
            strips = (H + S - 1) // S
            blob = Blob()
            off = blob.put(b"".join(light_params(rng, mid, midp) for _ in range(nb)))
            per_crop = [3, H * W * midp // 2 if level == 0 else reid.OS_SLOTS * H * W * midp // 2, reid.OS_SLOTS * H * W * midp // 2, 4 * strips * midp]
            ops = mk_ops([dict(type=reid.H_OS_LIGHT, in_buf=1 if level == 0 else 2, out_buf=2, aux_buf=3, H=H, W=W, C=midp, Ho=H, Wo=W, Co=midp, k=level, s=nb, p=strip, w_off=off)])
            plan = Plan(L, ops, per_crop, blob.array(), n, 1, 1, 4 * strips * midp)
            try:
                T = act(rng, (n, reid.OS_SLOTS, H, W, midp), mid)
                plan.fill(1, O.words(act(rng, (n, H, W, midp), mid)) if level == 0 else O.words(T))
                before = T.copy()
                plan.fill(2, O.words(T))
                plan.run()
                bufs = plan.bufs()
                check("k_osnet_light", "%dx%d mid %d level %d strip %d (%d rows)" % (H, W, mid, level, strip, S), ops, blob.array(), bufs, n, real=[mid])
                after = O.halves(bufs[2], (reid.OS_SLOTS, H, W, midp))
                lo, hi = reid.os_level_slot(level), reid.os_level_slot(level) + nb
                assert np.array_equal(after[:, :lo].view(np.uint16), before[:, :lo].view(np.uint16)) and np.array_equal(after[:, hi:].view(np.uint16), before[:, hi:].view(np.uint16))
                part = bufs[3].reshape(n, 4, strips, midp)
                assert np.all(np.delete(part, level, axis=1) == SENTINEL), "sums of another level written"
            finally:
                plan.close()


@pytest.mark.parametrize("cin,cout", [(16, 64), (96, 24), (288, 72), (128, 128)])
def test_pointwise(L, cin, cout):
    """M = 3 x 5 x 7 = 105 pixels (not a multiple of the 16-pixel tile nor of the 64-pixel workgroup), every epilogue: none, ReLU, + identity then ReLU, the second
    GEMM (conv3 | downsample) then ReLU, and the IBN block's pre-norm sum (+ identity / second GEMM without ReLU)"""
    n, H, W = 3, 5, 7
    cinp, coutp, cin2 = reid.pad16(cin), reid.pad16(cout), 40
    rng = R.rng_for("pw", cin, cout)
    for relu, mode in ((0, reid.RES_NONE), (1, reid.RES_NONE), (1, reid.RES_ADD), (1, reid.RES_GEMM), (0, reid.RES_ADD), (0, reid.RES_GEMM)):
        blob = Blob()
        b = np.zeros(coutp); b[:cout] = rng.normal(0, 0.1, cout)
        kw = dict(w_off=blob.put(reid._frags(rng.normal(0, (1.0 / cin) ** 0.5, (cout, cin)), coutp, cinp)), b_off=blob.put(reid._f32(b)))
        aux_halves = 0
        if mode == reid.RES_GEMM:
            kw.update(s=reid.pad16(cin2), w2_off=blob.put(reid._frags(rng.normal(0, (1.0 / cin2) ** 0.5, (cout, cin2)), coutp, reid.pad16(cin2))))
            aux_halves = H * W * reid.pad16(cin2)
        elif mode == reid.RES_ADD:
            aux_halves = H * W * coutp
        per_crop = [3, H * W * cinp // 2, H * W * coutp // 2] + ([aux_halves // 2] if aux_halves else [])
        ops = mk_ops([dict(type=reid.H_OS_PW, in_buf=1, out_buf=2, aux_buf=3 if aux_halves else -1, H=H, W=W, C=cinp, Ho=H, Wo=W, Co=coutp, k=mode, relu=relu, **kw)])
        plan = Plan(L, ops, per_crop, blob.array(), n, 1, 1, H * W * coutp // 2)
        try:
            plan.fill(1, O.words(act(rng, (n, H, W, cinp), cin)))
            if mode == reid.RES_GEMM:
                plan.fill(3, O.words(act(rng, (n, H, W, reid.pad16(cin2)), cin2)))
            elif mode == reid.RES_ADD:
                plan.fill(3, O.words(act(rng, (n, H, W, coutp), cout)))
            plan.run()
            check("k_osnet_pw", "%d -> %d relu %d residual mode %d" % (cin, cout, relu, mode), ops, blob.array(), plan.bufs(), n, real=[cout])
        finally:
            plan.close()


@pytest.mark.parametrize("c0", [16, 48, 64])
@pytest.mark.parametrize("H,W", [(16, 16), (32, 16)])
def test_stem(L, H, W, c0):
    n = 3
    rng = R.rng_for("stem", H, W, c0)
    blob = Blob()
    off = blob.put(reid.stem_frags(rng.normal(0, (1.0 / 147) ** 0.5, (c0, 3, 7, 7))))
    boff = blob.put(rng.normal(0, 0.1, c0))
    ops = mk_ops([dict(type=reid.H_OS_STEM, in_buf=0, out_buf=1, H=H, W=W, C=3, Ho=H // 2, Wo=W // 2, Co=c0, k=7, s=2, p=3, w_off=off, b_off=boff)])
    plan = Plan(L, ops, [H * W * 3, (H // 2) * (W // 2) * c0 // 2], blob.array(), n, H, W, (H // 2) * (W // 2) * c0 // 2)
    try:
        plan.run(rng.normal(0, 1, (n, H, W, 3)).astype(f32))
        check("k_osnet_stem", "%dx%d crops -> %d" % (H, W, c0), ops, blob.array(), plan.bufs(), n)
    finally:
        plan.close()


@pytest.mark.parametrize("H,W", [(1, 1), (4, 4), (32, 16)])
def test_instance_norm(L, H, W):
    """fp16 (the general path) and fp32 (the exact op list; alone and as the norm of in + aux), channel 1 constant (variance 0) and the pad channels 24 .. 31 zero with
    zero gamma and beta"""
    n, C, real = 3, 32, 24
    rng = R.rng_for("instnorm", H, W)
    blob = Blob()
    g = np.zeros(C); g[:real] = rng.uniform(0.7, 1.3, real)
    b = np.zeros(C); b[:real] = rng.normal(0, 0.1, real)
    goff, boff = blob.put(g), blob.put(b)
    x = act(rng, (n, H, W, C), real)
    x[..., 1] = f16(0.75)
    for relu in (1, 0):
        ops = mk_ops([dict(type=reid.H_OS_INSTNORM, in_buf=1, out_buf=2, H=H, W=W, C=C, Ho=H, Wo=W, Co=C, relu=relu, w_off=goff, b_off=boff)])
        plan = Plan(L, ops, [3, H * W * C // 2, H * W * C // 2], blob.array(), n, 1, 1, H * W * C // 2)
        try:
            plan.fill(1, O.words(x))
            plan.run()
            bufs = plan.bufs()
            check("k_osnet_instnorm<h>", "%dx%d relu %d" % (H, W, relu), ops, blob.array(), bufs, n, real=[real])
            y = O.halves(bufs[2], (H, W, C)).astype(f64)
            want = b[1] if not relu else max(b[1], 0.0)
            assert np.all(np.abs(y[..., 1] - want) <= 2.0 ** -11 * abs(want) + 2.0 ** -25 + 4e-7), "a constant channel must come out as beta"
        finally:
            plan.close()
    for with_add in (False, True):
        ops = mk_ops([dict(type=reid.INSTNORM, in_buf=1, out_buf=2, aux_buf=3 if with_add else -1, H=H, W=W, C=C, Ho=H, Wo=W, Co=C, relu=1, w_off=goff, b_off=boff)])
        plan = Plan(L, ops, [3, H * W * C, H * W * C] + ([H * W * C] if with_add else []), blob.array(), n, 1, 1, H * W * C)
        try:
            plan.fill(1, x.astype(f32).reshape(n, -1) * f32(1.001))
            if with_add:
                plan.fill(3, act(rng, (n, H, W, C), real).astype(f32).reshape(n, -1))
            plan.run()
            check("k_osnet_instnorm<f>", "%dx%d add %d" % (H, W, with_add), ops, blob.array(), plan.bufs(), n)
        finally:
            plan.close()


@pytest.mark.parametrize("mid,Rr,H,W,strip", [(16, 1, 7, 4, 3), (128, 8, 5, 16, 0), (24, 1, 4, 1, 1), (72, 4, 40, 32, 0)])
def test_gate_sum(L, mid, Rr, H, W, strip):
    """R = 1 and R = 8, one strip and several, pads (24 -> 32, 72 -> 80), a map of more than one pixel chunk (40 x 32 = 1280 pixels)"""
    n, midp = 3, reid.pad16(mid)
    rng = R.rng_for("gatesum", mid, Rr, H, W)
    S = reid.os_strip_rows(H, W, midp, strip)
    strips = (H + S - 1) // S
    blob = Blob()
    w1 = padded(rng.normal(0, (1.0 / mid) ** 0.5, (Rr, mid)), Rr, midp)
    w2 = padded(rng.normal(0, 1.0, (mid, Rr)), midp, Rr)
    b2 = np.zeros(midp); b2[:mid] = rng.normal(0, 0.5, mid)
    kw = dict(w_off=blob.put(w1), b_off=blob.put(rng.normal(0, 0.1, Rr)), w2_off=blob.put(w2), b2_off=blob.put(b2))
    ops = mk_ops([dict(type=reid.H_OS_GATESUM, in_buf=1, out_buf=2, aux_buf=3, H=H, W=W, C=midp, Ho=H, Wo=W, Co=midp, R=Rr, p=strip, **kw)])
    plan = Plan(L, ops, [3, reid.OS_SLOTS * H * W * midp // 2, H * W * midp // 2, 4 * strips * midp], blob.array(), n, 1, 1, H * W * midp // 2)
    try:
        T = np.maximum(act(rng, (n, reid.OS_SLOTS, H, W, midp), mid), f16(0))
        part = np.zeros((n, 4, strips, midp), f32)
        for b in range(4):
            for k in range(strips):
                part[:, b, k] = T[:, reid.os_level_slot(b), k * S:(k + 1) * S].astype(f32).sum((1, 2), dtype=f32)
        plan.fill(1, O.words(T))
        plan.fill(3, part.reshape(n, -1))
        plan.run()
        check("k_osnet_gatesum", "mid %d R %d %dx%d strips %d" % (mid, Rr, H, W, strips), ops, blob.array(), plan.bufs(), n, real=[mid])
    finally:
        plan.close()


def test_avgpool_and_tail(L):
    n, H, W, C, fd = 3, 4, 6, 48, 32
    rng = R.rng_for("tail")
    blob = Blob()
    woff = blob.put(reid._frags(rng.normal(0, (1.0 / C) ** 0.5, (fd, C)), fd, C))
    boff = blob.put(rng.normal(0, 0.1, fd))
    ops = mk_ops([dict(type=reid.H_OS_AVGPOOL, in_buf=1, out_buf=2, H=H, W=W, C=C, Ho=H // 2, Wo=W // 2, Co=C),
                  dict(type=reid.H_OS_GAPFC, in_buf=2, out_buf=4, aux_buf=3, H=H // 2, W=W // 2, C=C, Ho=1, Wo=1, Co=fd, relu=1, w_off=woff, b_off=boff)])
    plan = Plan(L, ops, [3, H * W * C // 2, (H // 2) * (W // 2) * C // 2, C // 2, fd], blob.array(), n, 1, 1, fd)
    try:
        plan.fill(1, O.words(act(rng, (n, H, W, C), C)))
        feats = plan.run()
        bufs = plan.bufs()
        check("avgpool2 + gap + fc", "%dx%dx%d -> %d" % (H, W, C, fd), ops, blob.array(), bufs, n)
        assert np.array_equal(feats, bufs[4])
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ whole networks
def fixture(name):
    if name not in _CACHE:
        z = np.load(os.path.join(GOLD, "osnet_family_%s.npz" % name))
        width, ibn = reid.OSNET_NAMES[name]
        spec = reid.osnet_spec(width, ibn=ibn)
        _CACHE[name] = (z, spec, reid.random_state_dict(spec, int(z["seed"])))
    return _CACHE[name]


@pytest.mark.parametrize("key", ["a", "b", "c"])
@pytest.mark.parametrize("name", list(reid.OSNET_NAMES))
def test_network_on_fixture_crops(L, name, key):
    z, spec, sd = fixture(name)
    x, emb = z["crops_" + key], z["emb_" + key]
    n = x.shape[0]
    ops, per_crop, w = reid.lower_osnet_f16(sd, spec, x.shape[1], x.shape[2])
    plan = Plan(L, ops, per_crop, w, n, x.shape[1], x.shape[2], 512)
    try:
        feats = plan.run(x)
        bufs = plan.bufs()
    finally:
        plan.close()
    worst = check("network", "%s %dx%d" % (name, x.shape[1], x.shape[2]), ops, w, bufs, n, real=O.real_channels(spec))
    d_emu = O.rel_l2(O.emulate(ops, w, x)[0], emb)
    d_dev = O.rel_l2(feats, emb)
    print("NET %-16s %3dx%-3d crops %d  D_emu %.3e  device %.3e  (bar 2 D_emu = %.3e)  worst per-tensor err/bar %.3f" % (name, x.shape[1], x.shape[2], n, d_emu, d_dev, 2 * d_emu, worst))
    assert d_dev <= 2 * d_emu


def test_x1_0_at_strongsort_geometry(L):
    """two 128 x 256 (H x W) crops through osnet_x1_0: the auto strip rule at the real geometry (32 x 64 maps of 64 channels: 5-row strips, 7 strips) -- every stored
    tensor of the LightConv3x3 levels, the sums and the gated sums of the first block against the references from the device's own buffers, and the features against
    the emulation's at twice the emulation's own distance from the float64 chain"""
    spec = reid.osnet_spec(1.0)
    sd = reid.random_state_dict(spec, 4)
    x = R.rng_for("x1_0 128x256").normal(0, 1, (2, 128, 256, 3)).astype(f32)
    ops, per_crop, w = reid.lower_osnet_f16(sd, spec, 128, 256)
    assert O.strips_of(ops[3]) == (5, 7)
    plan = Plan(L, ops, per_crop, w, 2, 128, 256, 512)
    try:
        feats = plan.run(x)
        first = {int(o[k]) for o in ops[:9] for k in ("in_buf", "out_buf", "aux_buf") if int(o[k]) >= 0}
        bufs = {b: plan.read(b) for b in first}
    finally:
        plan.close()
    check("network", "osnet_x1_0 128x256, stem .. conv2.0", ops[:9], w, bufs, 2, real=O.real_channels(spec)[:9])
    emu = O.emulate(ops, w, x)[0]
    ref = O.chain(ops, w, x)
    d_emu, d_dev = O.rel_l2(emu, ref), O.rel_l2(feats, ref)
    print("NET %-16s 128x256 crops 2  D_emu %.3e  device %.3e  (against the float64 chain)" % ("osnet_x1_0", d_emu, d_dev))
    assert d_dev <= 2 * d_emu


# ------------------------------------------------------------------------------------------------ behaviour
def test_bits_repeat_and_do_not_depend_on_the_batch():
    from yolov7_tracker_amd.tracker.reid import ReIDExtractor
    x = torch.randn((5, 32, 16, 3), generator=torch.Generator().manual_seed(2))
    for width, ibn in ((0.75, False), (1.0, True)):
        e5 = ReIDExtractor(None, width=width, ibn=ibn, size=(16, 32), max_crops=5, seed=5, half=True)
        e128 = ReIDExtractor(None, width=width, ibn=ibn, size=(16, 32), max_crops=128, seed=5, half=True)
        assert e5.half and not e5.fused
        a = e5.forward_crops(x).cpu()
        assert torch.equal(a, e5.forward_crops(x).cpu()), "two calls differ"
        assert torch.equal(a, e128.forward_crops(x).cpu()), "max_crops changes the bits"
        for i in (0, 3):
            assert torch.equal(a[i:i + 1], e5.forward_crops(x[i:i + 1]).cpu()), "a crop alone differs from the crop in a batch of 5"
        assert float(a.abs().mean()) > 0.01 and bool(torch.isfinite(a).all())


def test_x0_25_half_and_the_default_paths():
    """x0_25 at 128 x 64 with half=True within 2 D_emu of the fixture; the defaults are untouched: without half the same configuration takes the fused kernel and
    meets the expectations of tests/test_reid_gpu.py::test_fused_osnet_kernel_matches_oracle, other widths take the fp32 op list; half with fused raises"""
    from oracle import reid_torch
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker.reid import ReIDExtractor
    z, spec, sd = fixture("osnet_x0_25")
    x, emb = z["crops_c"], z["emb_c"]
    e = ReIDExtractor(sd, max_crops=4, half=True)
    assert e.half and not e.fused
    ops, _, w = reid.lower_osnet_f16(sd, spec, 128, 64)
    d_emu, d_dev = O.rel_l2(O.emulate(ops, w, x)[0], emb), O.rel_l2(e.forward_crops(torch.from_numpy(x)).cpu().numpy(), emb)
    print("NET %-16s 128x64  crops 1  D_emu %.3e  device %.3e  (ReIDExtractor(half=True))" % ("osnet_x0_25", d_emu, d_dev))
    assert d_dev <= 2 * d_emu
    with pytest.raises(ValueError):
        ReIDExtractor(None, fused=True, half=True)
    assert not ReIDExtractor(None, width=0.5, max_crops=4).half and not ReIDExtractor(None, width=0.5, max_crops=4).fused
    fused = ReIDExtractor(None, seed=3, max_crops=64)
    assert fused.fused and not fused.half
    frame = synth.make_frames(1, 80, 640, seq_idx=3)[0]
    rng = np.random.default_rng(5)
    xy, wh = rng.uniform(0, 560, (60, 2)), rng.uniform(8, 200, (60, 2))
    boxes = np.concatenate([xy, np.minimum(xy + wh, 700)], 1).astype(np.float32)
    want = reid_torch.osnet_forward(fused.sd, reid_torch.preprocess(frame, boxes)).numpy()
    got = fused.features_for_boxes(frame, boxes).cpu().numpy()
    scale = float(np.abs(want).max())
    assert np.abs(got - want).max() <= 3e-3 * scale
    # the general path from the FRAME (k_reid_crop's pixels, rounded to fp16 by the stem): the same features at the fused kernel's tolerance
    half = ReIDExtractor(None, seed=3, max_crops=64, half=True).features_for_boxes(frame, boxes).cpu().numpy()
    assert np.abs(half - want).max() <= 3e-3 * scale


def test_checkpoint_detects_ibn_and_passes_half_through(tmp_path):
    from yolov7_tracker_amd.tracker.reid import ReIDExtractor
    z, spec, sd = fixture("osnet_ibn_x1_0")
    path = str(tmp_path / "osnet_ibn.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, path)
    e = ReIDExtractor.from_checkpoint(path, size=(16, 32), max_crops=4, half=True)
    assert e.half and e.spec.get("ibn") and e.spec["channels"][0] == 64
    ops, _, w = reid.lower_osnet_f16(sd, spec, 32, 16)
    d_emu, d_dev = O.rel_l2(O.emulate(ops, w, z["crops_a"])[0], z["emb_a"]), O.rel_l2(e.forward_crops(torch.from_numpy(z["crops_a"])).cpu().numpy(), z["emb_a"])
    assert d_dev <= 2 * d_emu
    assert not ReIDExtractor.from_checkpoint(path, size=(16, 32), max_crops=4).half


def test_ibn_exact_op_list():
    """osnet_ibn_x1_0 through the fp32 op list (the exact path) against the fixture: fp32 on ~60 layers, the existing op-list test's tolerance (2e-4)"""
    from yolov7_tracker_amd.tracker.reid import ReIDExtractor
    z, spec, sd = fixture("osnet_ibn_x1_0")
    e = ReIDExtractor(sd, width=1.0, size=(16, 32), max_crops=4)
    assert e.spec.get("ibn") and not e.half and not e.fused and int(reid.INSTNORM) in [int(o["type"]) for o in e.ops]
    got = e.forward_crops(torch.from_numpy(z["crops_a"])).cpu().numpy()
    np.testing.assert_allclose(got, z["emb_a"], rtol=2e-4, atol=2e-4 * float(np.abs(z["emb_a"]).max()))
