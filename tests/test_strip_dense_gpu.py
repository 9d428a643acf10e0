"""GPU: the dense strip form of the LDS-patch kernel (csrc/y7t_conv_patch.hip, W = 20, 40) through y7t_conv2d_nhwc_f16, on the shapes of
tests/test_strip_dense_convsim.py: tiles that straddle rows and images, a ragged last tile, one to three chunk pairs, slices, every weight order -- against
torch fp32 at the layer bar of tests/test_detector_gpu.py -- and the poisoned-neighbour case: NaN in the pixels a wrapped tap would read must not spread."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_strip_dense_convsim import DENSE_CASES, poisoned_input
from tests.util import pack_w
from yolov7_tracker_amd.detector.layout import act_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


def run_layer(L, x, Wt, bias, act, korder, in_coff=0, out_ld=None, out_coff=0):
    from yolov7_tracker_amd import _lib
    B, H, W, in_ld = x.shape
    Cout, Cin = Wt.shape[:2]
    out_ld = out_ld or Cout
    cout_pad = (Cout + 63) // 64 * 64
    bp = np.zeros(cout_pad, np.float32)
    bp[:Cout] = bias
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(pack_w(Wt, Cin, cout_pad, korder)).cuda(), torch.from_numpy(bp).cuda()
    out = torch.full((B, H, W, out_ld), 7.0, dtype=torch.float16, device="cuda")
    zeros = torch.zeros(128, dtype=torch.float16, device="cuda")
    _lib.check(L.y7t_conv2d_nhwc_f16(_lib.ptr(xd), in_ld, in_coff, B, H, W, Cin, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out), out_ld, out_coff, 0, Cout, cout_pad,
                                     3, 3, 1, 1, act | act_bits(korder, force_patch=True), _lib.ptr(zeros), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.float().cpu().numpy(), L.y7t_last_kernel().decode()


def reference(x, Wt, bias, act):
    ref = F.conv2d(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), torch.from_numpy(Wt.astype(np.float16).astype(np.float32)), torch.from_numpy(bias), 1, 1)
    ref = F.silu(ref) if act == 1 else F.leaky_relu(ref, 0.1) if act == 2 else ref
    return ref.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: "%dx%dx%d_%d-%d_o%d" % (c[0], c[1], c[2], c[3], c[4], c[6]))
def test_dense_strip_layer_matches_torch_fp32(L, case):
    B, H, W, Cin, Cout, act, korder, kw = case
    in_ld, in_coff, out_ld, out_coff = kw.get("in_ld", Cin), kw.get("in_coff", 0), kw.get("out_ld", Cout), kw.get("out_coff", 0)
    rng = np.random.default_rng(B * 1000 + H + W + Cin)
    x = rng.normal(0, 1, (B, H, W, in_ld)).astype(np.float16)
    Wt = (rng.normal(0, 1, (Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    bias = rng.normal(0, 0.5, Cout).astype(np.float32)
    got, name = run_layer(L, x, Wt, bias, act, korder, in_coff, out_ld, out_coff)
    assert name.startswith("patch_strip<%d," % W), name
    # fp16 inputs are exact in both; fp32 accumulate; the only error is the final fp16 store (rel 2^-11) + sum order
    np.testing.assert_allclose(got[..., out_coff:out_coff + Cout], reference(x[..., in_coff:in_coff + Cin], Wt, bias, act), rtol=6e-4, atol=3e-4)
    other = np.ones(out_ld, bool)
    other[out_coff:out_coff + Cout] = False
    assert np.all(got[..., other] == 7.0)                              # nothing outside the output slice is written


def test_dense_strip_border_taps_are_selected_not_multiplied(L):
    """NaN in column W-1 and row H-1 of every image, no activation: isnan(out) == isnan(reference) exactly, the finite values at the layer bar"""
    B, H, W, Cin, Cout = 3, 20, 20, 64, 64
    x, want_nan = poisoned_input(B, H, W, Cin, 3)
    rng = np.random.default_rng(4)
    Wt = (rng.normal(0, 1, (Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    bias = rng.normal(0, 0.5, Cout).astype(np.float32)
    got, name = run_layer(L, x, Wt, bias, 0, 1)
    assert name.startswith("patch_strip<20,"), name
    ref = reference(x, Wt, bias, 0)
    assert np.array_equal(np.isnan(ref), np.broadcast_to(want_nan[..., None], ref.shape))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=6e-4, atol=3e-4)
