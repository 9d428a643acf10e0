"""CPU: every numpy float64 reference of tests/op_refs.py against torch.nn.functional evaluated in float64 on the shapes the GPU tests use
(tests/test_reid_ops_gpu.py, tests/test_membound_gpu.py), so that a wrong reference can neither hide nor invent a failure there.  Two float64
evaluations of the same sum differ by rounding only: 1e-12 relative to sum|terms| is eight orders under the fp32 bars the references serve."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import op_refs as R

N = 3


_rng = R.rng_for


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).permute(0, 3, 1, 2)


def _close(ref, want, scale):
    want = want.numpy() if isinstance(want, torch.Tensor) else want
    assert ref.shape == want.shape, (ref.shape, want.shape)
    assert np.all(np.abs(ref - want) <= 1e-12 * (np.asarray(scale) + 1e-300) + 1e-300), float(np.abs(ref - want).max())


@pytest.mark.parametrize("case", R.CONV_SHAPES)
def test_conv(case):
    H, W, Ci, Co, k, s, p, has_bias, relu = case
    rng = _rng("conv", case)
    x, w = rng.normal(0, 1, (N, H, W, Ci)), rng.normal(0, 1, (Co, k, k, Ci))
    b = rng.normal(0, 1, Co) if has_bias else None
    ref, ab, K = R.conv(x, w, b, k, s, p, relu)
    wt = torch.from_numpy(w).permute(0, 3, 1, 2).contiguous()
    want = F.conv2d(_nchw(x), wt, None if b is None else torch.from_numpy(b), s, p)
    wab = F.conv2d(_nchw(np.abs(x)), wt.abs(), None if b is None else torch.from_numpy(np.abs(b)), s, p)
    _close(ref, (F.relu(want) if relu else want).permute(0, 2, 3, 1), ab)
    _close(ab, wab.permute(0, 2, 3, 1), ab)
    assert K == k * k * Ci + has_bias and float(ab.min()) >= 0.0


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", R.DWCONV_SHAPES)
def test_dwconv3(shape, relu):
    H, W, C = shape
    rng = _rng("dw", shape)
    x, w, b = rng.normal(0, 1, (N, H, W, C)), rng.normal(0, 1, (C, 3, 3)), rng.normal(0, 1, C)
    ref, ab, K = R.dwconv3(x, w, b, relu)
    want = F.conv2d(_nchw(x), torch.from_numpy(w)[:, None], torch.from_numpy(b), 1, 1, 1, C)
    wab = F.conv2d(_nchw(np.abs(x)), torch.from_numpy(np.abs(w))[:, None], torch.from_numpy(np.abs(b)), 1, 1, 1, C)
    _close(ref, (F.relu(want) if relu else want).permute(0, 2, 3, 1), ab)
    _close(ab, wab.permute(0, 2, 3, 1), ab)
    assert K == 10


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_pools(shape):
    H, W, C = shape
    x = _rng("pool", shape).normal(-3, 1, (N, H, W, C))                  # all-negative windows: a zero-initialised maximum would differ
    assert np.array_equal(R.maxpool3s2(x), F.max_pool2d(_nchw(x), 3, 2, 1).permute(0, 2, 3, 1).numpy())
    assert np.array_equal(R.maxpool3s2(x, relu_first=True), F.max_pool2d(F.relu(_nchw(x)), 3, 2, 1).permute(0, 2, 3, 1).numpy())
    if H >= 2 and W >= 2:
        ref, ab, K = R.avgpool2(x)
        _close(ref, F.avg_pool2d(_nchw(x), 2).permute(0, 2, 3, 1), ab)
        _close(ab, F.avg_pool2d(_nchw(np.abs(x)), 2).permute(0, 2, 3, 1), ab)
        assert K == 4


@pytest.mark.parametrize("shape", R.GAP_SHAPES)
def test_gap(shape):
    HW, C = shape
    x = _rng("gap", shape).normal(0, 1, (N, HW, C))
    ref, ab, K = R.gap(x)
    _close(ref, F.adaptive_avg_pool2d(torch.from_numpy(x).permute(0, 2, 1)[..., None], 1).flatten(1), ab)
    _close(ab, torch.from_numpy(np.abs(x)).mean(1), ab)
    assert K == HW


@pytest.mark.parametrize("shape", R.GATE_SHAPES)
def test_gate_and_scale_acc(shape):
    C, Rr = shape
    rng = _rng("gate", shape)
    x = rng.normal(0, 1, (N, 8, C))
    w1, b1, w2, b2 = rng.normal(0, C ** -0.5, (Rr, C)), rng.normal(0, 0.1, Rr), rng.normal(0, Rr ** -0.5, (C, Rr)), rng.normal(0, 0.1, C)
    pooled, pab, K = R.gap(x)
    g, bound = R.gate(pooled, w1, b1, w2, b2, R.sum_bound(K, pab, pooled))
    t = torch.from_numpy(x).permute(0, 2, 1)[..., None]                               # (N, C, HW, 1): ChannelGate.forward on a map
    p_t = F.adaptive_avg_pool2d(t, 1)
    g_t = torch.sigmoid(F.conv2d(F.relu(F.conv2d(p_t, torch.from_numpy(w1)[..., None, None], torch.from_numpy(b1))), torch.from_numpy(w2)[..., None, None], torch.from_numpy(b2)))
    _close(g, g_t.flatten(1), 1.0)
    assert bound.shape == g.shape and float(bound.min()) >= 4 * R.U32 and float(bound.max()) < 1e-4      # a few hundred roundings at most
    first, ab1, K1 = R.scale_acc(x, g)
    _close(first, (t * g_t)[..., 0].permute(0, 2, 1), ab1)
    second, ab2, K2 = R.scale_acc(x[:, ::-1], g, first)
    _close(second, (t * g_t + t.flip(2) * g_t)[..., 0].permute(0, 2, 1), ab2)
    assert (K1, K2) == (1, 2)


def test_add_relu_fc_l2norm():
    rng = _rng("misc")
    a, b = rng.normal(0, 1, (N, 4, 3, 24)), rng.normal(0, 1, (N, 4, 3, 24))
    ref, ab, K = R.add_relu(a, b)
    _close(ref, F.relu(torch.from_numpy(a) + torch.from_numpy(b)), ab)
    assert K == 2 and np.array_equal(ab, np.abs(a) + np.abs(b))
    for (C, O) in R.FC_SHAPES:
        for relu in (0, 1):
            x, w, bias = rng.normal(0, 1, (N, C)), rng.normal(0, 1, (O, C)), rng.normal(0, 1, O)
            ref, ab, K = R.fc(x, w, bias, relu)
            want = F.linear(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias))
            _close(ref, F.relu(want) if relu else want, ab)
            _close(ab, F.linear(torch.from_numpy(np.abs(x)), torch.from_numpy(np.abs(w)), torch.from_numpy(np.abs(bias))), ab)
            assert K == C + 1
    for C in R.L2NORM_SHAPES:
        x = rng.normal(0, 1, (N, C))
        ref, ab, K = R.l2norm(x)
        _close(ref, F.normalize(torch.from_numpy(x), dim=1, eps=0.0), 1.0)
        assert K == C and np.array_equal(ab, np.abs(ref))


def test_fp16_helpers():
    rng = _rng("h")
    x = rng.normal(0, 1, (N, 7, 5, 3)).astype(np.float32)
    p = R.h_pack(x)
    assert p.dtype == np.float16 and p.shape == (N, 7, 5, 16) and not p[..., 3:].any()
    assert torch.equal(torch.from_numpy(p[..., :3].copy()), torch.from_numpy(x).half())
    a, b = rng.normal(0, 1, (N, 64)).astype(np.float16), rng.normal(0, 1, (N, 64)).astype(np.float16)
    assert torch.equal(torch.from_numpy(R.h_add_relu(a)), F.relu(torch.from_numpy(a).float()).half())
    assert torch.equal(torch.from_numpy(R.h_add_relu(a, b)), F.relu(torch.from_numpy(a).float() + torch.from_numpy(b).float()).half())
    for HW, C in R.H_GAP_SHAPES:
        x = rng.normal(0, 1, (N, HW, C)).astype(np.float16)
        ref, bound = R.h_gap_l2norm(x)
        want = F.normalize(torch.from_numpy(x.astype(np.float64)).mean(1), dim=1, eps=0.0)
        _close(ref, want, 1.0)
        assert bound.shape == ref.shape and float(bound.min()) > 0.0 and float(bound.max()) < 1e-3


@pytest.mark.parametrize("is_u8,reorg,ldout,H,W", [(0, 0, 8, 6, 10), (0, 1, 16, 6, 10), (1, 0, 8, 5, 7), (1, 1, 16, 6, 26)])
def test_input_layout(is_u8, reorg, ldout, H, W):
    """against the torch expressions of tests/test_detector_pinned_gpu.py (tracker_dataloader.py:83-88, models/common.py:48-53)"""
    rng = _rng("layout", is_u8, reorg)
    if is_u8:
        img = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        t = torch.from_numpy(img[..., ::-1].copy()).permute(0, 3, 1, 2).float() / 255.0
    else:
        img = rng.random((2, 3, H, W), dtype=np.float32)
        t = torch.from_numpy(img)
    if reorg:
        t = torch.cat([t[..., ::2, ::2], t[..., 1::2, ::2], t[..., ::2, 1::2], t[..., 1::2, 1::2]], 1)
    got = torch.from_numpy(R.input_layout(img, is_u8, reorg, ldout))
    c = t.shape[1]
    assert got.shape == (2, t.shape[2], t.shape[3], ldout)
    assert torch.equal(got[..., :c], t.half().permute(0, 2, 3, 1)) and not got[..., c:].any()


def test_the_float32_osnet_oracle_is_accurate_enough_for_its_bar():
    """tests/test_reid_ops_gpu.py::test_osnet_x0_5_through_the_op_list judges the device against oracle/reid_torch.osnet_forward in float32 at rtol 2e-4 /
    atol 2e-4 max|want|.  That bar is only meaningful if the oracle's own rounding error is small against it: float32 against float64 evaluation of the same
    parameters on the same crops must differ by less than a quarter of it."""
    from oracle import reid_torch
    from yolov7_tracker_amd.tracker import reid
    sd = reid.random_state_dict(reid.osnet_spec(0.5), 3)
    x = torch.randn((5, 3, 128, 64), generator=torch.Generator().manual_seed(1))
    w32, w64 = reid_torch.osnet_forward(sd, x).double().numpy(), reid_torch.osnet_forward(sd, x, dtype=torch.float64).numpy()
    bar = 2e-4 * np.abs(w32) + 2e-4 * float(np.abs(w32).max())
    ratio = float((np.abs(w32 - w64) / bar).max())
    print("float32 vs float64 OSNet x0_5 oracle: worst |diff| / bar = %.3f" % ratio)
    assert ratio < 0.25
