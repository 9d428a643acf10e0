"""GPU: the ReID op-list kernels of csrc/y7t_reid.hip ONE OP AT A TIME against the numpy float64 references of tests/op_refs.py (pinned against
torch.nn.functional by tests/test_op_refs_cpu.py).  As whole networks they run at one geometry only, and a wrong border tap moves a 512-dimensional feature by
far less than the whole-network bars.

Every case is a plan of one (or two) `y7t_reid_op`s built with y7t_reid_create over an arena the test owns: buffer 0 is a 3-float dummy (in_h = in_w = 1, the
entry copy of `crops_f32` lands there), the op reads buffer 1 (and its aux buffer) and writes buffer 2; feat_dim is the output's floats per crop, so
y7t_reid_forward hands back the op's whole output.  The arena starts as a sentinel and everything the op must not write has to keep it.

Bars (derived in tests/op_refs.py, never tuned): copy / max / ReLU / one rounding -> exact; fp32 sums of K products ->
(K + 2) 2^-24 sum|terms| + 2^-24 |ref|; the gate -> that bound carried through both layers, / 4, + 4 * 2^-24.  Every test prints its worst err / bound as a
`MARGIN` line (profiles/op_tests_margins.txt keeps the table of one run)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import op_refs as R

pytestmark = pytest.mark.gpu

N = 3
SENTINEL = 7.0
E_ARG = -1
KERNEL = {0: "k_reid_conv", 1: "k_reid_dwconv3", 2: "k_reid_pool<max>", 3: "k_reid_pool<avg>", 4: "k_reid_gap + k_reid_gate + k_reid_scale_acc", 5: "k_reid_add_relu",
          6: "k_reid_gap", 7: "k_reid_fc", 8: "k_reid_l2norm", 9: "k_h_pack", 11: "k_h_maxpool3s2_relu", 12: "k_h_add_relu (one operand)", 13: "k_h_add_relu",
          14: "k_h_gap_l2norm"}


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


def margin(kernel, case, err, bound):
    """assert err <= bound everywhere, print the worst ratio"""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print("MARGIN %-44s %-40s worst err/bound %.3f" % (kernel, case, ratio))
    assert np.all(err <= bound), "%s %s: %d values over the bound, worst err/bound %.2f" % (kernel, case, int((err > bound).sum()), ratio)
    return ratio


def exact(kernel, case, got, want):
    print("MARGIN %-44s %-40s exact" % (kernel, case))
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), "%s %s: %d values differ" % (kernel, case, int((got != want).sum()))


class OpPlan:
    """ops: list of dicts of y7t_reid_op fields; per_crop: floats per crop of every buffer (buffer 0: the 3-float dummy)"""

    def __init__(self, L, ops, per_crop, weights, n=N, max_crops=N, feat_dim=None, expect_rc=0):
        from yolov7_tracker_amd import _lib
        from yolov7_tracker_amd.tracker import reid
        assert per_crop[0] == 3
        self.L, self.n, self.max_crops, self.per_crop = L, n, max_crops, per_crop
        self.ops = np.zeros(len(ops), reid.OP_DTYPE)
        for o, kw in zip(self.ops, ops):
            o["aux_buf"], o["b_off"] = -1, -1
            for k, v in kw.items():
                o[k] = v
        offs, o = [], 64
        for b in per_crop:
            offs.append(o)
            o += (b * max_crops + 63) // 64 * 64 + 64                   # 64 sentinel floats between buffers
        self.offs = np.array(offs, dtype=np.int64)
        self.arena = torch.full((o,), SENTINEL, dtype=torch.float32, device="cuda")
        self.w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)).cuda()
        self.feat_dim = int(feat_dim if feat_dim is not None else per_crop[int(self.ops[-1]["out_buf"])])
        self.crops = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
        self.h = ctypes.c_void_p()
        self.rc = L.y7t_reid_create(self.ops.ctypes.data_as(ctypes.c_void_p), len(self.ops), self.offs.ctypes.data_as(ctypes.c_void_p), len(offs), _lib.ptr(self.arena),
                                    self.arena.numel() * 4, _lib.ptr(self.w), max_crops, 1, 1, self.feat_dim, ctypes.byref(self.h))
        assert self.rc == expect_rc, (self.rc, L.y7t_last_error())
        self.untouched = None

    def fill(self, buf, arr):
        """arr: (n, ...) float32 or float16 (two halves per float of the buffer)"""
        t = torch.from_numpy(np.ascontiguousarray(arr)).cuda().reshape(-1)
        o = int(self.offs[buf])
        if t.dtype == torch.float16:
            assert t.numel() == 2 * self.n * self.per_crop[buf]
            self.arena[o:o + t.numel() // 2].view(torch.float16)[:] = t
        else:
            assert t.dtype == torch.float32 and t.numel() == self.n * self.per_crop[buf]
            self.arena[o:o + t.numel()] = t

    def read(self, buf, floats=None, off=0):
        o = int(self.offs[buf]) + off
        return self.arena[o:o + (self.n * self.per_crop[buf] if floats is None else floats)].clone()

    def run(self, written):
        """forward -> (n, feat_dim) float32 numpy.  written: buffers the op may write; everything else of the arena (the dummy buffer aside) must stay as it was,
        and so must the rows of the written buffers behind crop n"""
        from yolov7_tracker_amd import _lib
        before = self.arena.clone()
        feats = torch.full((self.n * self.feat_dim + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(self.L.y7t_reid_forward(self.h, None, 0, 0, None, self.n, _lib.ptr(self.crops), _lib.ptr(feats), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((feats[self.n * self.feat_dim:] == SENTINEL).all())
        keep = torch.ones_like(before, dtype=torch.bool)
        keep[int(self.offs[0]):int(self.offs[0]) + 3 * self.n] = False
        for b, floats in written.items():
            keep[int(self.offs[b]):int(self.offs[b]) + floats] = False
        assert torch.equal(self.arena[keep].view(torch.int32), before[keep].view(torch.int32)), "the op wrote outside its output"
        return feats[:self.n * self.feat_dim].view(self.n, self.feat_dim).cpu().numpy()

    def close(self):
        if self.h:
            self.L.y7t_reid_destroy(self.h)


def one_op(L, op, x, out_floats, weights=(0.0,), aux=None, aux_floats=0, max_crops=N):
    """op reads buffer 1 (= x), aux buffer 3, writes buffer 2 -> (n, out_floats) float32 numpy (the raw words of an fp16 output)"""
    per_crop = [3, x[0].size // (2 if x.dtype == np.float16 else 1), out_floats] + ([aux_floats] if aux_floats else [])
    plan = OpPlan(L, [dict(op, in_buf=1, out_buf=2, aux_buf=3 if aux_floats else -1)], per_crop, weights, max_crops=max_crops)
    try:
        plan.fill(1, x)
        if aux is not None:
            plan.fill(3, aux)
        return plan.run({2: N * out_floats})
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ fp32 op list
@pytest.mark.parametrize("case", R.CONV_SHAPES)
def test_conv(L, case):
    from yolov7_tracker_amd.tracker import reid
    H, W, Ci, Co, k, s, p, has_bias, relu = case
    rng = R.rng_for("conv", case)
    x = rng.normal(0, 1, (N, H, W, Ci)).astype(np.float32)
    w = rng.normal(0, (Ci * k * k) ** -0.5, (Co, k, k, Ci)).astype(np.float32)
    b = rng.normal(0, 0.5, Co).astype(np.float32) if has_bias else None
    ref, ab, K = R.conv(x, w, b, k, s, p, relu)
    Ho, Wo = ref.shape[1:3]
    got = {}
    for kmajor in ((0, 1) if k == 1 and s == 1 else (0,)):
        wp = w.transpose(1, 2, 3, 0) if kmajor else w
        blob = np.concatenate([wp.reshape(-1), b if has_bias else np.zeros(0, np.float32)])
        op = dict(type=reid.CONV, H=H, W=W, C=Ci, Ho=Ho, Wo=Wo, Co=Co, k=k, s=s, p=p, relu=relu, w_kmajor=kmajor, w_off=0, b_off=w.size if has_bias else -1)
        got[kmajor] = one_op(L, op, x, Ho * Wo * Co, blob).reshape(ref.shape)
        margin(KERNEL[reid.CONV] + (" kmajor" if kmajor else ""), "%dx%d %d->%d k%d s%d p%d bias%d relu%d" % case, np.abs(got[kmajor] - ref), R.sum_bound(K, ab, ref))
    if 1 in got:                                                       # tracker/reid.py::_Lowering.conv: "same products in the same order either way"
        exact(KERNEL[reid.CONV] + " kmajor == cmajor", "%dx%d %d->%d" % case[:4], got[1], got[0])


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", R.DWCONV_SHAPES)
def test_dwconv3(L, shape, relu):
    from yolov7_tracker_amd.tracker import reid
    H, W, C = shape
    rng = R.rng_for("dw", shape, relu)
    x, w, b = (rng.normal(0, 1, s_).astype(np.float32) for s_ in ((N, H, W, C), (C, 3, 3), (C,)))
    ref, ab, K = R.dwconv3(x, w, b, relu)
    op = dict(type=reid.DWCONV3, H=H, W=W, C=C, Ho=H, Wo=W, Co=C, k=3, s=1, p=1, relu=relu, w_off=0, b_off=w.size)
    got = one_op(L, op, x, H * W * C, np.concatenate([w.reshape(-1), b])).reshape(ref.shape)
    margin(KERNEL[reid.DWCONV3], "%dx%d C%d relu%d" % (H, W, C, relu), np.abs(got - ref), R.sum_bound(K, ab, ref))


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_pools(L, shape):
    from yolov7_tracker_amd.tracker import reid
    H, W, C = shape
    x = R.rng_for("pool", shape).normal(-3, 1, (N, H, W, C)).astype(np.float32)
    x = -np.abs(x) - np.float32(0.125)                                 # ALL negative: a maximum that starts at zero cannot pass
    want = R.maxpool3s2(x).astype(np.float32)
    Ho, Wo = want.shape[1:3]
    got = one_op(L, dict(type=reid.MAXPOOL3S2, H=H, W=W, C=C, Ho=Ho, Wo=Wo, Co=C), x, Ho * Wo * C).reshape(want.shape)
    exact(KERNEL[reid.MAXPOOL3S2], "%dx%d C%d" % shape, got, want)
    if H >= 2 and W >= 2:
        ref, ab, K = R.avgpool2(x)
        got = one_op(L, dict(type=reid.AVGPOOL2, H=H, W=W, C=C, Ho=H // 2, Wo=W // 2, Co=C), x, (H // 2) * (W // 2) * C).reshape(ref.shape)
        margin(KERNEL[reid.AVGPOOL2], "%dx%d C%d" % shape, np.abs(got - ref), R.sum_bound(K, ab, ref))


@pytest.mark.parametrize("shape", R.GAP_SHAPES)
def test_gap(L, shape):
    from yolov7_tracker_amd.tracker import reid
    HW, C = shape
    x = R.rng_for("gap", shape).normal(0.5, 1, (N, HW, C)).astype(np.float32)
    ref, ab, K = R.gap(x)
    got = one_op(L, dict(type=reid.GAP, H=HW, W=1, C=C), x, C, max_crops=5)
    margin(KERNEL[reid.GAP], "HW%d C%d" % shape, np.abs(got - ref), R.sum_bound(K, ab, ref))


@pytest.mark.parametrize("shape", R.GATE_SHAPES)
def test_gate_acc(L, shape):
    """GATE_ACC = k_reid_gap + k_reid_gate + k_reid_scale_acc: first = 1 (overwrite the accumulator), then first = 0 of another branch onto the same accumulator;
    3 crops in an arena laid out for 8 (the gates sit behind max_crops pooled vectors in the scratch buffer)"""
    from yolov7_tracker_amd.tracker import reid
    C, Rr = shape
    H, W, MAXC = 4, 2, 8
    rng = R.rng_for("gate", shape)
    xa, xb = (rng.normal(0.3, 1, (N, H * W, C)).astype(np.float32) for _ in range(2))
    w1, b1 = rng.normal(0, C ** -0.5, (Rr, C)).astype(np.float32), rng.normal(0, 0.1, Rr).astype(np.float32)
    w2, b2 = rng.normal(0, Rr ** -0.5, (C, Rr)).astype(np.float32), rng.normal(0, 0.1, C).astype(np.float32)
    blob = np.concatenate([w1.reshape(-1), b1, w2.reshape(-1), b2])
    offs = dict(w_off=0, b_off=w1.size, w2_off=w1.size + Rr, b2_off=w1.size + Rr + w2.size)
    ops = [dict(type=reid.GATE_ACC, in_buf=1, out_buf=2, aux_buf=3, H=H, W=W, C=C, R=Rr, relu=1, **offs),
           dict(type=reid.GATE_ACC, in_buf=4, out_buf=2, aux_buf=3, H=H, W=W, C=C, R=Rr, relu=0, **offs)]
    per_crop = [3, H * W * C, H * W * C, 2 * C, H * W * C]
    written = {2: N * H * W * C, 3: 2 * MAXC * C}
    case = "C%d R%d" % shape
    refs = []
    for x in (xa, xb):
        pooled, pab, K = R.gap(x)
        g, gb = R.gate(pooled, w1, b1, w2, b2, R.sum_bound(K, pab, pooled))
        refs.append((pooled, R.sum_bound(K, pab, pooled), g, gb))
    # first branch alone
    plan = OpPlan(L, ops[:1], per_crop, blob, max_crops=MAXC)
    try:
        plan.fill(1, xa)
        got = plan.run(written).reshape(N, H * W, C)
        pooled, gate_ = plan.read(3, N * C).view(N, C).cpu().numpy(), plan.read(3, N * C, off=MAXC * C).view(N, C).cpu().numpy()
        assert bool((plan.read(3, (MAXC - N) * C, off=N * C) == SENTINEL).all()) and bool((plan.read(3, (MAXC - N) * C, off=(MAXC + N) * C) == SENTINEL).all())
    finally:
        plan.close()
    margin("k_reid_gap (GATE_ACC)", case, np.abs(pooled - refs[0][0]), refs[0][1])
    margin("k_reid_gate", case, np.abs(gate_ - refs[0][2]), refs[0][3])
    ref, ab, K = R.scale_acc(xa, refs[0][2])
    margin("k_reid_scale_acc first", case, np.abs(got - ref), np.abs(xa) * refs[0][3][:, None, :] + R.sum_bound(K, ab, ref))
    # both branches onto the same accumulator
    plan = OpPlan(L, ops, per_crop, blob, max_crops=MAXC)
    try:
        plan.fill(1, xa)
        plan.fill(4, xb)
        got = plan.run(written).reshape(N, H * W, C)
    finally:
        plan.close()
    ref, ab, K = R.scale_acc(xb, refs[1][2], ref)
    bound = np.abs(xa) * refs[0][3][:, None, :] + np.abs(xb) * refs[1][3][:, None, :] + R.sum_bound(K, ab, ref)
    margin("k_reid_scale_acc first, then accumulate", case, np.abs(got - ref), bound)


def test_gate_acc_refusals(L):
    from yolov7_tracker_amd.tracker import reid
    for C, Rr in ((257, 16), (256, 65), (64, 0)):
        op = dict(type=reid.GATE_ACC, in_buf=1, out_buf=2, aux_buf=3, H=2, W=2, C=C, R=Rr, relu=1, w_off=0, b_off=0, w2_off=0, b2_off=0)
        OpPlan(L, [op], [3, 4 * C, 4 * C, 2 * C], np.zeros(8, np.float32), expect_rc=E_ARG)


def test_add_relu_fc_l2norm(L):
    from yolov7_tracker_amd.tracker import reid
    rng = R.rng_for("misc")
    a, b = (rng.normal(0, 1, (N, 5, 3, 24)).astype(np.float32) for _ in range(2))
    ref, ab, K = R.add_relu(a, b)
    got = one_op(L, dict(type=reid.ADD_RELU, H=5, W=3, C=24), a, 5 * 3 * 24, aux=b, aux_floats=5 * 3 * 24).reshape(ref.shape)
    margin(KERNEL[reid.ADD_RELU], "5x3 C24", np.abs(got - ref), R.sum_bound(K, ab, ref))
    for (C, O) in R.FC_SHAPES:
        for relu in (0, 1):
            x, w, bias = (rng.normal(0, 1, s_).astype(np.float32) for s_ in ((N, C), (O, C), (O,)))
            ref, ab, K = R.fc(x, w, bias, relu)
            got = one_op(L, dict(type=reid.FC, H=1, W=1, C=C, Co=O, relu=relu, w_off=0, b_off=w.size), x, O, np.concatenate([w.reshape(-1), bias]))
            margin(KERNEL[reid.FC], "%d->%d relu%d" % (C, O, relu), np.abs(got - ref), R.sum_bound(K, ab, ref))
    for C in R.L2NORM_SHAPES:
        x = rng.normal(0, 1, (N, C)).astype(np.float32)
        ref, ab, K = R.l2norm(x)
        got = one_op(L, dict(type=reid.L2NORM, H=1, W=1, C=C), x, C)
        margin(KERNEL[reid.L2NORM], "C%d" % C, np.abs(got - ref), R.sum_bound(K, ab, ref))


# ------------------------------------------------------------------------------------------------ fp16 helpers of the MFMA op list
def _halves(feats, shape):
    return np.ascontiguousarray(feats).view(np.float16).reshape(shape)


def test_h_pack(L):
    from yolov7_tracker_amd.tracker import reid
    x = R.rng_for("pack").normal(0, 2, (N, 7, 5, 3)).astype(np.float32)
    x[0, 0, 0] = [65519.0, 2.0 ** -25, -1.0 - 2.0 ** -11]               # rounds to the largest fp16 / underflows to zero / a tie that rounds to even
    got = _halves(one_op(L, dict(type=reid.H_PACK, H=7, W=5, C=3), x, 7 * 5 * 8), (N, 7, 5, 16))
    exact(KERNEL[reid.H_PACK], "7x5", got.view(np.uint16), R.h_pack(x).view(np.uint16))


@pytest.mark.parametrize("n,H,W,C", [(1, 128, 64, 64), (N, 7, 5, 64), (N, 1, 1, 8)])
def test_h_maxpool_relu(L, n, H, W, C):
    from yolov7_tracker_amd.tracker import reid
    x = R.rng_for("hmp", H, W).normal(-0.5, 1, (n, H, W, C)).astype(np.float16)
    x[:, :3, :3] = -np.abs(x[:, :3, :3]) - np.float16(0.5)               # windows that are all negative: the ReLU floor, not a tap, is the answer
    want = R.maxpool3s2(x, relu_first=True).astype(np.float16)
    Ho, Wo = want.shape[1:3]
    per_crop = [3, H * W * C // 2, Ho * Wo * C // 2]
    plan = OpPlan(L, [dict(type=reid.H_MAXPOOL_RELU, in_buf=1, out_buf=2, H=H, W=W, C=C, Ho=Ho, Wo=Wo, Co=C)], per_crop, (0.0,), n=n, max_crops=n)
    try:
        plan.fill(1, x)
        got = _halves(plan.run({2: n * per_crop[2]}), want.shape)
    finally:
        plan.close()
    exact(KERNEL[reid.H_MAXPOOL_RELU], "%dx%d C%d n%d" % (H, W, C, n), got.view(np.uint16), want.view(np.uint16))


def test_h_relu_and_add_relu(L):
    from yolov7_tracker_amd.tracker import reid
    rng = R.rng_for("hadd")
    a, b = (rng.normal(0, 1, (N, 7, 5, 24)).astype(np.float16) for _ in range(2))
    b[0, 0, 0, :4] = -a[0, 0, 0, :4]                                   # exact cancellation
    a[0, 0, 1, :2], b[0, 0, 1, :2] = np.float16(2048.0), np.float16(1.0)      # a sum that is not an fp16 value: ONE rounding of the fp32 sum (to even)
    fl = 7 * 5 * 24 // 2
    got = _halves(one_op(L, dict(type=reid.H_RELU, H=7, W=5, C=24), a, fl), a.shape)
    exact(KERNEL[reid.H_RELU], "7x5 C24", got.view(np.uint16), R.h_add_relu(a).view(np.uint16))
    got = _halves(one_op(L, dict(type=reid.H_ADD_RELU, H=7, W=5, C=24), a, fl, aux=b, aux_floats=fl), a.shape)
    exact(KERNEL[reid.H_ADD_RELU], "7x5 C24", got.view(np.uint16), R.h_add_relu(a, b).view(np.uint16))


@pytest.mark.parametrize("shape", R.H_GAP_SHAPES)
def test_h_gap_l2norm(L, shape):
    from yolov7_tracker_amd.tracker import reid
    HW, C = shape
    x = R.rng_for("hgap", shape).normal(0.2, 1, (N, HW, C)).astype(np.float16)
    ref, bound = R.h_gap_l2norm(x)
    got = one_op(L, dict(type=reid.H_GAP_L2NORM, H=HW, W=1, C=C), x, C)
    margin(KERNEL[reid.H_GAP_L2NORM], "HW%d C%d" % shape, np.abs(got - ref), bound)


def test_h_op_refusals(L):
    from yolov7_tracker_amd.tracker import reid
    OpPlan(L, [dict(type=reid.H_GAP_L2NORM, in_buf=1, out_buf=2, H=32, W=1, C=1032)], [3, 16 * 1032, 1032], (0.0,), expect_rc=E_ARG)
    OpPlan(L, [dict(type=reid.H_RELU, in_buf=1, out_buf=2, H=2, W=2, C=12)], [3, 24, 24], (0.0,), expect_rc=E_ARG)
    OpPlan(L, [dict(type=reid.H_ADD_RELU, in_buf=1, out_buf=2, aux_buf=-1, H=2, W=2, C=16)], [3, 32, 32], (0.0,), expect_rc=E_ARG)


# ------------------------------------------------------------------------------------------------ a second width through the whole op list
def test_osnet_x0_5_through_the_op_list():
    """OSNet width 0.5 (32 / 128 / 192 / 256 channels: 32-wide OSBlock branches, R = 2 / 3 / 4 gates) on 128 x 64 crops, 5 crops in an arena for 8, against
    oracle/reid_torch.osnet_forward at the bar of the x0_25 test (tests/test_reid_gpu.py).  tests/test_op_refs_cpu.py checks that the oracle's own float32
    rounding error (float32 against float64 evaluation) is under a quarter of that bar."""
    from oracle import reid_torch
    from yolov7_tracker_amd.tracker.reid import ReIDExtractor
    e = ReIDExtractor(None, width=0.5, seed=3, max_crops=8)
    assert not e.fused and e.spec["channels"] == [32, 128, 192, 256]
    x = torch.randn((5, 3, 128, 64), generator=torch.Generator().manual_seed(1))
    got = e.forward_crops(x.permute(0, 2, 3, 1).contiguous()).cpu().numpy()
    want = reid_torch.osnet_forward(e.sd, x).numpy()
    assert got.shape == want.shape == (5, 512) and float(np.abs(want).mean()) > 0.05
    tol = 2e-4 * np.abs(want) + 2e-4 * float(np.abs(want).max())
    margin("OSNet x0_5 op list (all fp32 kernels)", "128x64, 5 crops of 8", np.abs(got - want), tol)
