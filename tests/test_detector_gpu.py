"""GPU parity tests of the detector half of the hot path (through the C ABI): MFMA implicit-GEMM conv per layer, the
whole yolov7-tiny / yolov7-w6 forward, decode + NMS.  Oracle: oracle/detector_torch.py (plain torch fp32 on the CPU,
pinned against the reference's models.yolo.Model in tests/test_detector_oracle.py).
Stated tolerances (fp16 activations / fp32 accumulate vs the fp32 oracle): see each test."""
import ctypes

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import layer_cout_pad, pack_w
from yolov7_tracker_amd.detector.layout import FORCE_PATCH, WeightLayout as WL, act_bits, layout_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


CONV_CASES = [
    # B, H, W, Cin, Cout, k, s, act, in_ld, in_coff, out_ld, out_coff, out_f32, the kernel csrc/y7t_conv.hip::conv_dispatch sends the case to (written from the dispatch code)
    (1, 20, 20, 64, 64, 1, 1, 1, 64, 0, 64, 0, 0, "igemm<128,64,32,2> 1x1"),
    (2, 17, 23, 64, 128, 3, 1, 1, 64, 0, 128, 0, 0, "igemm<128,128,64,2> splitK"),
    (1, 40, 40, 128, 256, 3, 2, 1, 128, 0, 256, 0, 0, "igemm<128,128,64,2> splitK"),
    (2, 32, 32, 16, 64, 3, 1, 1, 16, 0, 64, 0, 0, "igemm<128,64,64,2> ragged-K"),          # stem-like (K = 144)
    (1, 24, 24, 96, 192, 1, 1, 2, 256, 64, 384, 192, 0, "igemm<128,64,32,2>"),    # slices of wider buffers, LeakyReLU
    (1, 16, 16, 256, 45, 1, 1, 0, 256, 0, 45, 0, 1, "igemm<128,64,32,2> 1x1 splitK"),        # Detect head: fp32 out, Cout not a multiple of 4
    (3, 9, 9, 512, 512, 3, 1, 1, 512, 0, 512, 0, 0, "igemm<128,128,64,2> splitK"),        # small map, deep K
    (1, 130, 130, 32, 64, 3, 2, 1, 32, 0, 64, 0, 0, "igemm<128,64,64,2> ragged-K"),        # M not a multiple of the tile
    (2, 24, 40, 128, 128, 3, 1, 1 | act_bits(WL.LINE_MAJOR), 128, 0, 128, 0, 0, "igemm<128,128,64,2> splitK"),  # weights in the (kh, chunk, kw) K order (act bit 8)
    (1, 33, 31, 192, 64, 3, 2, 1 | act_bits(WL.LINE_MAJOR), 256, 64, 64, 0, 0, "igemm<128,64,64,2> splitK"),  # same, stride 2, input slice of a wider buffer
    # LDS-patch kernel (3x3 / stride 1, Cin % 64 == 0): 16x16 tiles, 32x8 tiles, 64- and 128-channel panels, both K orders,
    # ragged image edges (act bit 9 forces the kernel when the tile efficiency is below its dispatch threshold or the batch leaves it fewer than 256 x 256 pixels per channel
    # tile: y7t_conv_patch_try declines those, and a forced 64-channel layer runs the multi-tile form), slices
    (2, 80, 80, 128, 128, 3, 1, 1 | act_bits(WL.LINE_MAJOR) | FORCE_PATCH, 128, 0, 128, 0, 0, "patch<16,16,128>"),
    (1, 64, 96, 64, 64, 3, 1, 1 | act_bits(WL.PATCH), 256, 128, 192, 64, 0, "patch<16,16,64>"),
    (1, 24, 64, 64, 128, 3, 1, 2 | FORCE_PATCH, 64, 0, 128, 0, 0, "patch<32,8,128>"),
    (4, 128, 128, 64, 64, 3, 1, 1 | act_bits(WL.LINE_MAJOR), 64, 0, 64, 0, 0, "patch<16,16,64>"),      # 65536 pixels x one channel tile: the smallest batch the dispatcher sends there unforced
    (2, 37, 53, 192, 256, 3, 1, 1 | act_bits(WL.LINE_MAJOR) | FORCE_PATCH, 256, 64, 320, 64, 0, "patch<32,8,128>"),
    (1, 37, 70, 128, 64, 3, 1, 1 | FORCE_PATCH, 128, 0, 64, 0, 0, "patch_mt<16,16,4>"),
    (3, 20, 20, 512, 512, 3, 1, 1 | act_bits(WL.LINE_MAJOR) | FORCE_PATCH, 512, 0, 512, 0, 0, "patch_strip<20,128>"),
    # the same kernel fed with panel-packed weights (act bit 10; what detector/graph.py chooses for eligible layers)
    (2, 80, 80, 128, 128, 3, 1, 1 | act_bits(WL.PATCH), 128, 0, 128, 0, 0, "patch<16,16,128>"),
    (1, 24, 64, 192, 64, 3, 1, 2 | act_bits(WL.PATCH), 256, 64, 64, 0, 0, "patch<32,8,64>"),
    (2, 37, 53, 64, 256, 3, 1, 1 | act_bits(WL.PATCH), 64, 0, 320, 64, 0, "patch<32,8,128>"),
    # strip tiling of the narrow maps (W = 40, 20): the batch as one dense strip, 256 consecutive positions per workgroup
    (3, 40, 40, 128, 128, 3, 1, 1 | act_bits(WL.PATCH), 128, 0, 128, 0, 0, "patch_strip<40,128>"),
    (2, 24, 40, 64, 64, 3, 1, 2 | act_bits(WL.LINE_MAJOR) | FORCE_PATCH, 128, 64, 192, 128, 0, "patch_strip<40,64>"),
    (5, 20, 20, 192, 256, 3, 1, 1 | act_bits(WL.PATCH), 192, 0, 256, 0, 0, "patch_strip<20,128>"),
    (1, 7, 20, 64, 64, 3, 1, 1 | FORCE_PATCH, 64, 0, 64, 0, 0, "patch_strip<20,64>"),
    # multi-tile workgroups of the 64-channel patch kernel (act bit 9 forces them on small problems): tile count not a multiple of 4,
    # ragged edges, 2 and 6 chunks per tile, all three weight orders, output slice
    (3, 48, 48, 64, 64, 3, 1, 1 | FORCE_PATCH | act_bits(WL.PATCH), 64, 0, 64, 0, 0, "patch_mt<16,16,4>"),
    (5, 20, 20, 256, 256, 3, 1, 1 | act_bits(WL.PATCH_N64), 256, 0, 256, 0, 0, "patch_strip<20,64>"),  # PATCH_N64: the patch kernel's 64-row panels on a layer whose Cout would allow 128 (strip tiling)
    (2, 32, 48, 64, 128, 3, 1, 2 | act_bits(WL.PATCH_N64), 64, 0, 256, 128, 0, "patch<16,16,64>"),  # ... 16x16 tiles, output slice
    (3, 20, 20, 256, 256, 1, 1, 1 | act_bits(WL.PANEL_1X1_N64), 256, 0, 256, 0, 0, "igemm<128,64,32,2> 1x1 splitK"),  # PANEL_1X1_N64: 64-row 1x1 panels on a layer whose Cout would allow 128
    (1, 24, 24, 96, 128, 1, 1, 2 | act_bits(WL.PANEL_1X1_N64), 256, 64, 384, 192, 0, "igemm<128,64,32,2>"),  # ... slices, LeakyReLU
    (1, 37, 70, 192, 64, 3, 1, 2 | FORCE_PATCH | act_bits(WL.LINE_MAJOR), 256, 64, 192, 64, 0, "patch_mt<16,16,4>"),
    (2, 24, 64, 64, 192, 3, 1, 1 | FORCE_PATCH, 64, 0, 192, 0, 0, "patch_mt<32,8,4>"),
    # 1x1 layers with panel-packed weights (act bit 11): 128- and 64-row panels, Cin % 64 == 32, split-K on a small map, fp32 head
    (2, 40, 40, 256, 256, 1, 1, 1 | act_bits(WL.PANEL_1X1), 256, 0, 256, 0, 0, "igemm<128,128,32,2> 1x1 splitK"),
    (1, 24, 24, 96, 192, 1, 1, 2 | act_bits(WL.PANEL_1X1), 256, 64, 384, 192, 0, "igemm<128,64,32,2>"),
    (1, 20, 20, 1024, 512, 1, 1, 1 | act_bits(WL.PANEL_1X1), 1024, 0, 512, 0, 0, "igemm<128,128,32,2> 1x1 splitK"),
    (1, 16, 16, 256, 45, 1, 1, 0 | act_bits(WL.PANEL_1X1), 256, 0, 45, 0, 1, "igemm<128,64,32,2> 1x1 splitK"),
    # the shapes six of the LDS-patch and strip cases above had while they fell through to the generic kernel (unforced, fewer than 256 x 256 pixels per channel tile:
    # y7t_conv_patch_try declines): 3x3 / stride 1 with split-K, both K orders, slices -- and the 32 x 8 tiles of the unforced 64-channel patch kernel
    (2, 80, 80, 128, 128, 3, 1, 1 | act_bits(WL.LINE_MAJOR), 128, 0, 128, 0, 0, "igemm<128,128,64,2> splitK"),
    (1, 64, 96, 64, 64, 3, 1, 1, 256, 128, 192, 64, 0, "igemm<128,64,64,2> splitK"),
    (1, 24, 64, 64, 128, 3, 1, 2, 64, 0, 128, 0, 0, "igemm<128,128,64,2> splitK"),
    (2, 24, 64, 192, 64, 3, 1, 1 | act_bits(WL.LINE_MAJOR), 192, 0, 64, 0, 0, "igemm<128,64,64,2> splitK"),
    (2, 24, 40, 64, 64, 3, 1, 2 | act_bits(WL.LINE_MAJOR), 128, 64, 192, 128, 0, "igemm<128,64,64,2> splitK"),
    (1, 7, 20, 64, 64, 3, 1, 1, 64, 0, 64, 0, 0, "igemm<128,64,64,2> splitK"),
    (5, 120, 128, 64, 64, 3, 1, 1 | act_bits(WL.LINE_MAJOR), 64, 0, 64, 0, 0, "patch<32,8,64>"),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_layer_matches_torch_fp32(L, case, kernel=None):
    """kernel: the name y7t_last_kernel() must report (the tests derived from this one pass their own; CONV_CASES carries it as its last column)"""
    from yolov7_tracker_amd import _lib
    case, kernel = case[:13], kernel or case[13]
    B, H, W, Cin, Cout, k, s, act, in_ld, in_coff, out_ld, out_coff, out_f32 = case
    rng = np.random.default_rng(hash(case) % 2**32)
    x = rng.normal(0, 1, (B, H, W, in_ld)).astype(np.float16)
    Wt = (rng.normal(0, 1, (Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    bias = rng.normal(0, 0.5, Cout).astype(np.float32)
    korder = layout_of(act)[0]
    cout_pad = layer_cout_pad(Cout, korder)
    act_code = act
    act = act & 255
    if k == 3 and s == 1 and Cin % 64 == 0:    # the dispatcher must send these to the patch kernel when tiles are >= 80 % useful
        assert os.environ.get("Y7T_CONV_PATCH", "1") != "0"
    wp = pack_w(Wt, Cin, cout_pad, korder)
    bp = np.zeros(cout_pad, np.float32); bp[:Cout] = bias
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(wp).cuda(), torch.from_numpy(bp).cuda()
    out = torch.full((B, Ho, Wo, out_ld), 7.0, dtype=torch.float32 if out_f32 else torch.float16, device="cuda")
    zeros = torch.zeros(128, dtype=torch.float16, device="cuda")
    _lib.check(L.y7t_conv2d_nhwc_f16(_lib.ptr(xd), in_ld, in_coff, B, H, W, Cin, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out), out_ld, out_coff,
                                     out_f32, Cout, cout_pad, k, k, s, pad, act_code, _lib.ptr(zeros), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert L.y7t_last_kernel().decode() == kernel, (L.y7t_last_kernel().decode(), kernel)
    got = out.float().cpu().numpy()
    xs = torch.from_numpy(x[..., in_coff:in_coff + Cin].astype(np.float32)).permute(0, 3, 1, 2)
    ref = F.conv2d(xs, torch.from_numpy(Wt.astype(np.float16).astype(np.float32)), torch.from_numpy(bias), stride=s, padding=pad)
    ref = F.silu(ref) if act == 1 else (F.leaky_relu(ref, 0.1) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1).numpy()
    g = got[..., out_coff:out_coff + Cout]
    # fp16 inputs are exact in both; fp32 accumulate; the only error is the final fp16 store (rel 2^-11) + sum order
    np.testing.assert_allclose(g, ref, rtol=6e-4, atol=3e-4)
    # nothing outside the output slice may be touched
    mask = np.ones(out_ld, bool); mask[out_coff:out_coff + Cout] = False
    assert np.all(got[..., mask] == 7.0)


# csrc/y7t_conv_ws.hip: the 64 -> 64 3x3 layers with the filter bank resident in registers, one persistent workgroup per compute unit walking a range of
# 16 x 16 tiles through a three-buffer patch ring (act bit 13: WS64).  Shapes: fewer tiles than compute units; thousands of tiles (every workgroup
# walks many, the ring wraps, uneven ranges); slices of concat buffers; both activations; the benchmarked layer itself (320 x 320, 8 frames).
WS_CASES = [
    # B, H, W, Cin, Cout, k, s, act (bit 13), in_ld, in_coff, out_ld, out_coff, out_f32
    (1, 16, 16, 64, 64, 3, 1, 1 | act_bits(WL.WS64), 64, 0, 64, 0, 0),
    (1, 48, 80, 64, 64, 3, 1, 1 | act_bits(WL.WS64), 64, 0, 64, 0, 0),
    (3, 160, 160, 64, 64, 3, 1, 2 | act_bits(WL.WS64), 128, 64, 256, 128, 0),
    (7, 96, 112, 64, 64, 3, 1, 0 | act_bits(WL.WS64), 64, 0, 64, 0, 0),
    (8, 320, 320, 64, 64, 3, 1, 1 | act_bits(WL.WS64), 128, 0, 256, 192, 0),
]


@pytest.mark.parametrize("case", WS_CASES)
def test_weights_stationary_kernel_matches_torch_fp32(L, case):
    from yolov7_tracker_amd import _lib
    test_conv_layer_matches_torch_fp32(L, case, "ws64<16,16>")


# csrc/y7t_conv_ws128.hip: the 128-channel sibling (act bit 14: WS128), here through the single-layer entry point = its statically partitioned form; the tile-counter
# form runs inside a plan (test_weights_stationary_kernels_on_the_tile_counter_inside_a_plan below, tests/test_detector_pinned_gpu.py with Y7T_CONV_WS128=1)
WS128_CASES = [
    # B, H, W, Cin, Cout, k, s, act (bit 14), in_ld, in_coff, out_ld, out_coff, out_f32
    (1, 4, 16, 128, 128, 3, 1, 1 | act_bits(WL.WS128), 128, 0, 128, 0, 0),
    (1, 48, 80, 128, 128, 3, 1, 1 | act_bits(WL.WS128), 128, 0, 128, 0, 0),
    (3, 160, 160, 128, 128, 3, 1, 2 | act_bits(WL.WS128), 256, 128, 512, 128, 0),
    (5, 80, 80, 128, 256, 3, 1, 0 | act_bits(WL.WS128), 128, 0, 256, 0, 0),
    (8, 160, 160, 128, 128, 3, 1, 1 | act_bits(WL.WS128), 512, 0, 128, 0, 0),
]


@pytest.mark.parametrize("case", WS128_CASES)
def test_weights_stationary_128_kernel_matches_torch_fp32(L, case):
    test_conv_layer_matches_torch_fp32(L, case, "ws128<4,16>")


# ... and its stride-2 form (S2: 2 x 16 output tiles, parity-split 5 x 33 patch): the two w6 layers (128 -> 256 at 320 x 320 and 160 x 160) and small / sliced / multi-image cases
WS128_S2_CASES = [
    (1, 4, 32, 128, 128, 3, 2, 1 | act_bits(WL.WS128), 128, 0, 128, 0, 0),
    (1, 48, 96, 128, 256, 3, 2, 1 | act_bits(WL.WS128), 128, 0, 256, 0, 0),
    (3, 160, 160, 128, 256, 3, 2, 2 | act_bits(WL.WS128), 256, 128, 512, 256, 0),
    (4, 320, 320, 128, 256, 3, 2, 1 | act_bits(WL.WS128), 128, 0, 512, 0, 0),
    (7, 20, 64, 128, 128, 3, 2, 0 | act_bits(WL.WS128), 128, 0, 128, 0, 0),
]


@pytest.mark.parametrize("case", WS128_S2_CASES)
def test_weights_stationary_128_stride2_kernel_matches_torch_fp32(L, case):
    test_conv_layer_matches_torch_fp32(L, case, "ws128_s2<2,16>")


def test_weights_stationary_kernels_on_the_tile_counter_inside_a_plan(monkeypatch):
    """round 5: inside a detector's plan the persistent kernels take their tiles from the op's tile counter (Y7TConvArgs::tile_ctr, csrc/y7t_conv_ws.hip DYN).  A w6 plan
    at 16 frames of 640 x 640 with the 128-channel kernel switched on: the launch list names the tile-counter forms; three forwards in a row (the counters must come back
    to zero by themselves) give bit-identical heads, and those equal the heads of the same network lowered WITHOUT the weights-stationary kernels to within the fp16
    rounding of the intermediate tensors (different kernels accumulate in another order); the counters read zero afterwards."""
    from yolov7_tracker_amd.detector import arch, model
    B, S = 16, 640
    rng = np.random.default_rng(3)
    img = torch.from_numpy(rng.random((B, 3, S, S), dtype=np.float32))
    monkeypatch.setenv("Y7T_CONV_WS128", "1")
    det = model.Detector(arch.ARCHS["yolov7-w6"](10), None, img_size=(S, S), max_batch=B, seed=0, bn_bias_mean=2.0, calib_image=img[:1])
    names = det.launch_list(B)
    assert sum(n == "ws64<16,16> dyn" for n in names) >= 3 and sum(n == "ws128<4,16> dyn" for n in names) >= 4, names
    heads = []
    for _ in range(3):
        out = det(img)[0]
        torch.cuda.synchronize()
        heads.append([r.clone() for r in out.raw()])
    for h in heads[1:]:
        for a, b in zip(heads[0], h):
            assert torch.equal(a, b)
    monkeypatch.setenv("Y7T_CONV_WS128", "0")
    monkeypatch.setenv("Y7T_CONV_WS", "0")
    ref = model.Detector(arch.ARCHS["yolov7-w6"](10), det._sd, img_size=(S, S), max_batch=B)
    assert not any(n.startswith(("ws64", "ws128")) for n in ref.launch_list(B))
    want = ref(img)[0].raw()
    torch.cuda.synchronize()
    for l, (a, b) in enumerate(zip(heads[0], want)):
        scale = b.float().std().item()
        err = (a.float() - b.float()).abs()
        assert err.mean().item() < 2e-3 * scale and err.max().item() < 4e-2 * scale, (l, err.mean().item(), err.max().item(), scale)


# csrc/y7t_conv_ws_s2.hip: the 64 -> 128 3x3 / stride 2 layer with the filter bank resident in registers, a persistent workgroup per compute unit walking 2 x 32 output
# tiles through a three-buffer patch ring (act bit 16: WS_S2).  Shapes: fewer tiles than compute units, thousands of tiles (uneven ranges, the ring wraps), slices of
# wider buffers, the activations, and the benchmarked layer itself (640 x 640 -> 320 x 320, 8 frames).
WS_S2_CASES = [
    # B, H, W, Cin, Cout, k, s, act (bit 16), in_ld, in_coff, out_ld, out_coff, out_f32
    (1, 4, 64, 64, 128, 3, 2, 1 | act_bits(WL.WS_S2), 64, 0, 128, 0, 0),
    (1, 96, 192, 64, 128, 3, 2, 1 | act_bits(WL.WS_S2), 64, 0, 128, 0, 0),
    (3, 160, 320, 64, 128, 3, 2, 2 | act_bits(WL.WS_S2), 128, 64, 256, 128, 0),
    (5, 100, 128, 64, 128, 3, 2, 0 | act_bits(WL.WS_S2), 64, 0, 128, 0, 0),
    (8, 640, 640, 64, 128, 3, 2, 1 | act_bits(WL.WS_S2), 64, 0, 128, 0, 0),
]


@pytest.mark.parametrize("case", WS_S2_CASES)
def test_stride2_weights_stationary_kernel_matches_torch_fp32(L, case):
    test_conv_layer_matches_torch_fp32(L, case, "ws_s2<2,32>")


# csrc/y7t_conv_p8.hip: the 1x1 layers with Cout % 256 == 0 on the 256 x 256 x 64 ping-pong pipeline (act bit 15: P8).  Shapes: one K-tile (prologue + tail only), odd and
# even K-tile counts, ragged pixel tiles, several channel tiles, thousands of tiles (every CU runs many workgroups back to back), slices of concat buffers, the activations,
# and two layers of the benchmarked list at 8 frames.
P8_CASES = [
    # B, H, W, Cin, Cout, k, s, act (bit 15), in_ld, in_coff, out_ld, out_coff, out_f32
    (1, 16, 16, 64, 256, 1, 1, 1 | act_bits(WL.P8), 64, 0, 256, 0, 0),
    (1, 15, 20, 192, 256, 1, 1, 0 | act_bits(WL.P8), 192, 0, 256, 0, 0),
    (2, 33, 47, 128, 512, 1, 1, 2 | act_bits(WL.P8), 256, 128, 1024, 256, 0),
    (3, 80, 80, 512, 256, 1, 1, 1 | act_bits(WL.P8), 512, 0, 512, 256, 0),
    (8, 80, 80, 1024, 512, 1, 1, 1 | act_bits(WL.P8), 1024, 0, 512, 0, 0),
    (8, 40, 40, 1536, 768, 1, 1, 1 | act_bits(WL.P8), 1536, 0, 768, 0, 0),
    # round 6, the persistent form (a workgroup walks a column of pixel tiles: more tiles than CUs, an even number of K-tiles): three channel tiles on 255 workgroups with a
    # ragged last pixel tile; one channel tile, slices of wider buffers, LeakyReLU; two K-tiles per tile (the shortest loop the cross-tile prefetch allows)
    (5, 79, 79, 512, 768, 1, 1, 1 | act_bits(WL.P8), 512, 0, 768, 0, 0),
    (12, 80, 80, 256, 256, 1, 1, 2 | act_bits(WL.P8), 512, 256, 768, 512, 0),
    (6, 120, 120, 128, 256, 1, 1, 1 | act_bits(WL.P8), 128, 0, 256, 0, 0),
]


@pytest.mark.parametrize("case", P8_CASES)
def test_pingpong_1x1_kernel_matches_torch_fp32(L, case):
    test_conv_layer_matches_torch_fp32(L, case, "p8<256,256,64> 1x1")


def test_pingpong_1x1_kernel_is_deterministic_under_load(L):
    """the schedule keeps four half-tiles of DMA in flight across its barriers: a race would show as run-to-run differences (rare wrong tiles that come and go with memory
    load, cdna_hip_programming.md section 5) -- the same launch 20 times on 6400 tiles while a copy kernel streams beside it on another stream: bit-identical outputs"""
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.detector import weights
    B, H, W, Cin, Cout = 8, 160, 160, 256, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((B, H, W, Cin), device="cuda", generator=g).half()
    wt = (torch.randn((Cout, Cin), device="cuda", generator=g) / Cin ** 0.5).half()
    wp = torch.from_numpy(weights.panel_pack_p8(wt.cpu().numpy())).cuda()
    b = torch.randn(Cout, device="cuda", generator=g)
    zeros = torch.zeros(128, dtype=torch.float16, device="cuda")
    big = torch.empty((2, 64 << 20), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    outs = []
    for it in range(20):
        out = torch.zeros((B, H, W, Cout), dtype=torch.float16, device="cuda")
        with torch.cuda.stream(side):
            big[1].copy_(big[0], non_blocking=True)
        _lib.check(L.y7t_conv2d_nhwc_f16(_lib.ptr(x), Cin, 0, B, H, W, Cin, _lib.ptr(wp), _lib.ptr(b), _lib.ptr(out), Cout, 0, 0, Cout, Cout, 1, 1, 1, 0, 1 | act_bits(WL.P8),
                                         _lib.ptr(zeros), _lib.stream_ptr()))
        outs.append(out)
    torch.cuda.synchronize()
    assert L.y7t_last_kernel().decode().startswith("p8<256,256,64> 1x1")
    ref = F.silu(x.float().view(-1, Cin) @ wt.float().t() + b).view(B, H, W, Cout)
    assert torch.allclose(outs[0].float(), ref, rtol=6e-4, atol=3e-4)
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def test_pingpong_1x1_upsample_on_read_equals_materialised_upsample(monkeypatch):
    """the DUAL instance inside a network: with the ping-pong kernel taking every eligible 1x1 layer of a small forward (Y7T_CONV_P8_MIN_TILES=1), the plan that reads the
    three upsampled tensors through the loader equals the plan that materialises them, bit for bit (same kernel, same K order on both sides)"""
    # (an EXPERIMENT switch: the lowering honours it only beside the measuring build -- named here; the p8 instances themselves are in the product library that is loaded)
    monkeypatch.setenv("Y7T_LIB", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yolov7-tracker_amd", "lib", "liby7t_ablate.so"))
    monkeypatch.setenv("Y7T_CONV_P8_MIN_TILES", "1")
    img = torch.rand((2, 3, 256, 320), generator=torch.Generator().manual_seed(9))
    det = build("yolov7-w6", 10, (256, 320), 2)
    names = det.launch_list(2)
    assert sum(n == "p8<256,256,64> 1x1 upsample-on-read" for n in names) == 3 and sum(n.startswith("p8<") for n in names) >= 14, names
    a = [t.clone() for t in det(img)[0].raw()]
    monkeypatch.setenv("Y7T_UPSAMPLE_ON_READ", "0")
    ref = build("yolov7-w6", 10, (256, 320), 2)
    assert sum(int(o["type"]) == 1 for o in ref.plan.ops) == 3
    b = ref(img)[0].raw()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# csrc/y7t_conv_patch_s2.hip: the stride-2 LDS-patch kernel (parity-split patch columns, 16-channel chunks; PATCH_S2 = act bit 12), 128- and 256-channel panels
S2_CASES = [
    # B, H, W, Cin, Cout, k, s, act (bit 12: PATCH_S2), in_ld, in_coff, out_ld, out_coff, out_f32
    (1, 16, 32, 64, 128, 3, 2, 1 | act_bits(WL.PATCH_S2), 64, 0, 128, 0, 0),
    (2, 46, 90, 128, 256, 3, 2, 1 | act_bits(WL.PATCH_S2), 192, 64, 320, 64, 0),
    (4, 80, 80, 256, 384, 3, 2, 1 | act_bits(WL.PATCH_S2), 256, 0, 384, 0, 0),
    (2, 41, 37, 192, 248, 3, 2, 2 | act_bits(WL.PATCH_S2), 192, 0, 256, 0, 0),
    (8, 160, 160, 64, 128, 3, 2, 1 | act_bits(WL.PATCH_S2), 64, 0, 128, 0, 0),
    (2, 40, 40, 768, 1024, 3, 2, 1 | act_bits(WL.PATCH_S2), 768, 0, 1024, 0, 0),
]


@pytest.mark.parametrize("case", S2_CASES)
def test_stride2_patch_kernel_matches_torch_fp32(L, case):
    test_conv_layer_matches_torch_fp32(L, case, "patch_s2<256>" if layer_cout_pad(case[4], WL.PATCH_S2) % 256 == 0 else "patch_s2<128>")      # (s2_bn of csrc/y7t_conv_patch_s2.hip)


def build(name, nc, hw, B, seed=0):
    from yolov7_tracker_amd.detector import arch, model
    return model.Detector(arch.ARCHS[name](nc), None, img_size=hw, max_batch=B, seed=seed)


@pytest.mark.parametrize("name,nc,hw,B", [("yolov7-tiny", 80, (128, 192), 2), ("yolov7-w6", 10, (256, 320), 2)])
def test_whole_network_heads_match_oracle(name, nc, hw, B):
    from oracle import detector_torch as dt
    det = build(name, nc, hw, B)
    img = torch.rand((B, 3) + hw, generator=torch.Generator().manual_seed(1))
    out = det(img)[0]
    raw = [r.cpu() for r in out.raw()]
    dec, raw_ref = dt.forward(det.nodes, det._sd, img, det.spec["anchors"])
    _, raw_q = dt.forward(det.nodes, det._sd, img, det.spec["anchors"], fp16=True)
    for l, (a, b, q) in enumerate(zip(raw, raw_ref, raw_q)):
        assert a.shape == b.shape
        scale = b.std().item()
        # (1) against the oracle run at the SAME storage precision (fp16 weights/activations, fp32 accumulate): only the
        #     summation order differs, i.e. rare one-ulp fp16 flips -- which a randomly initialised (chaotic) network
        #     amplifies ~1.1-1.3x per layer (scripts/debug_layers.py prints the per-layer growth from 1e-7 at layer 0)
        eq = (a - q).abs()
        assert eq.mean().item() < 3e-2 * scale, (l, eq.mean().item(), scale)
        assert eq.max().item() < 0.5 * scale, (l, eq.max().item(), scale)
        # (2) against the fp32 oracle: the stated fp16-vs-fp32 tolerance on RAW LOGITS of a random-weight net -- mean below 8 % of
        #     the logit spread (measured: 0.5 % tiny, 1.5-4 % w6); the layer-level test above is the tight one (6e-4)
        err = (a - b).abs()
        assert err.mean().item() < 0.08 * scale, (l, err.mean().item(), scale)
        assert err.max().item() < 1.2 * scale, (l, err.max().item(), scale)
        print("level", l, "vs fp16-oracle mean/max %.2e %.2e   vs fp32-oracle mean/max %.2e %.2e   (std %.2f)" % (
            eq.mean().item(), eq.max().item(), err.mean().item(), err.max().item(), scale))


def test_two_detectors_on_two_streams_do_not_share_scratch():
    """small-batch launches split K over several workgroups and sum fp32 slabs from a workspace: each detector owns one (y7t_det_create), so two
    detectors enqueued on different streams at the same time give the heads each gives alone"""
    d1, d2 = build("yolov7-w6", 10, (256, 320), 1, seed=0), build("yolov7-w6", 10, (256, 320), 1, seed=1)
    x1 = torch.rand((1, 3, 256, 320), generator=torch.Generator().manual_seed(3)).cuda()
    x2 = torch.rand((1, 3, 256, 320), generator=torch.Generator().manual_seed(4)).cuda()
    alone1 = [r.clone() for r in d1(x1)[0].raw()]
    alone2 = [r.clone() for r in d2(x2)[0].raw()]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(5):
        with torch.cuda.stream(s1):
            o1 = d1(x1)[0]
            r1 = [r.clone() for r in o1.raw()]
        with torch.cuda.stream(s2):
            o2 = d2(x2)[0]
            r2 = [r.clone() for r in o2.raw()]
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(r1, alone1)) and all(torch.equal(a, b) for a, b in zip(r2, alone2))


def test_u8_bgr_input_equals_float_input():
    det = build("yolov7-tiny", 80, (128, 128), 1)
    frame = torch.randint(0, 256, (1, 128, 128, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    a = [r.clone() for r in det(frame.cuda())[0].raw()]
    f = (frame[..., [2, 1, 0]].permute(0, 3, 1, 2).float() / 255.0).contiguous()   # tracker_dataloader.py:83-88
    b = det(f)[0].raw()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape", [(540, 960), (1280, 1280), (300, 500)])
def test_letterbox_layout_matches_oracle(shape):
    """raw uint8 BGR frame -> device letterbox (resize + pad 114) + BGR->RGB,/255,ReOrg,fp16 == oracle letterbox + layout"""
    from oracle import letterbox_np as lb
    det = build("yolov7-w6", 10, (256, 256), 1)
    rng = np.random.default_rng(4)
    # smooth-ish image so that bilinear taps are not pure noise
    small = rng.integers(0, 256, (shape[0] // 8 + 2, shape[1] // 8 + 2, 3)).astype(np.float32)
    frame = np.kron(small, np.ones((8, 8, 1), np.float32))[:shape[0], :shape[1]].astype(np.uint8)
    from yolov7_tracker_amd import _lib
    out, (H, W) = det.forward_frames(torch.from_numpy(frame), img_size=256)      # selects the plan of the letterboxed size
    _, _, new_h, new_w, top, left = det.letterbox_params(shape, 256, 64)
    fd = torch.from_numpy(frame).cuda()[None].contiguous()
    # the stand-alone kernel (plans whose stem is fused with it never write this tensor: test_fused_stem_equals_layout_plus_conv)
    _lib.check(_lib.load().y7t_letterbox_layout_u8(_lib.ptr(fd), 1, shape[0], shape[1], H, W, new_h, new_w, top, left, 1, _lib.ptr(det.plan.arena), 16,
                                                   _lib.stream_ptr()))
    torch.cuda.synchronize()
    ref = lb.letterbox(frame, new_shape=(256, 256), stride=64)
    assert ref.shape[:2] == (H, W)
    x = lb.to_model_input(ref)                                   # (3, H, W) RGB
    want = np.concatenate([x[:, ::2, ::2], x[:, 1::2, ::2], x[:, ::2, 1::2], x[:, 1::2, 1::2]], 0).transpose(1, 2, 0)   # ReOrg, HWC
    got = det.buffer_view(0, 1, 16).view(1, H // 2, W // 2, 16)[0, :, :, :12].float().cpu().numpy()
    # the kernel and the oracle are the same sequence of float32 operations (no FMA contraction in csrc/y7t_post.hip): equal, rounding ties included
    # (upscaled frames, left != 0, the plain 8-channel form: tests/test_preprocess_gpu.py)
    assert np.array_equal(got, want.astype(np.float16).astype(np.float32))


def test_staged_heads_give_identical_detections():
    """Detector.stage_heads: decode+NMS from a private copy of the head buffers (so that it can overlap the next forward)
    returns exactly what decode+NMS on the arena returns -- also after the arena has been overwritten"""
    det = build("yolov7-tiny", 80, (128, 192), 2)
    g = torch.Generator().manual_seed(5)
    out = det(torch.rand((2, 3, 128, 192), generator=g))[0]
    for l in range(len(det.plan.heads)):
        t = det.head_tensor(l, 2)
        t.copy_((torch.randn(t.shape, generator=g) * 1.5).cuda())
    d0, n0 = det.postprocess(out, 0.01, 0.45, None)
    d0, n0 = d0.clone(), n0.clone()
    staged = det.stage_heads(out)
    det(torch.rand((2, 3, 128, 192), generator=g))           # the next forward rewrites the arena
    d1, n1 = det.postprocess(staged, 0.01, 0.45, None)
    torch.cuda.synchronize()
    assert torch.equal(n0, n1) and int(n0.sum()) > 10
    for b in range(2):
        assert torch.equal(d0[b, :n0[b]], d1[b, :n1[b]])


def test_decode_nms_matches_oracle():
    """plant head logits, run the device decode+NMS chain, compare with the oracle's non_max_suppression +
    scale_coords + round on the decoded tensor of the SAME logits."""
    from oracle import cnative, detector_torch as dt
    det = build("yolov7-w6", 10, (256, 320), 2)
    g = torch.Generator().manual_seed(3)
    out = det(torch.rand((2, 3, 256, 320), generator=g))[0]
    p = det.plan
    for l in range(len(p.heads)):
        t = det.head_tensor(l, 2)
        v = torch.randn(t.shape, generator=g) * 1.5
        v.view(2, t.shape[1], t.shape[2], 3, 15)[..., 4] -= 3.0     # few objectness hits
        t.copy_(v.cuda())
    dets, nd = det.postprocess(out, 0.01, 0.45, ori_shapes=[(200, 300), (256, 320)])
    torch.cuda.synchronize()
    det.check_overflow()
    dec = dt.decode_heads([r.cpu() for r in out.raw()], det.spec["anchors"], 256)      # the ORACLE's Detect decode of the planted logits
    assert torch.allclose(out.decoded().cpu(), dec, rtol=1e-5, atol=1e-4)               # the product's convenience view agrees with it
    ref = dt.non_max_suppression(dec, 0.01, 0.45)
    nd = nd.cpu().numpy()
    for b, shp in enumerate([(200, 300), (256, 320)]):
        r = ref[b]
        assert nd[b] == len(r) and len(r) > 20
        d = dets[b, :nd[b]].cpu()
        rr = r.clone()
        rr[:, :4] = dt.scale_coords_round((256, 320), r[:, :4], shp)
        assert torch.equal(d[:, 5], rr[:, 5])
        np.testing.assert_allclose(d[:, 4].numpy(), rr[:, 4].numpy(), rtol=1e-5, atol=1e-6)
        assert (d[:, :4] - rr[:, :4]).abs().max().item() <= 1.0          # |dcoord| <= 1 px after round
        assert ((d[:, :4] - rr[:, :4]).abs() > 0).float().mean().item() < 0.02
    # exact greedy semantics on identical inputs: oracle NMS over the device's own candidates keeps the same set
    from tests import post_scenes
    cbox, cscore, ccls, cidx, _ = post_scenes.unpack_candidates(p.ws.cpu().numpy(), det.max_batch, det.max_cand)      # the workspace's documented head
    cnt = p.cand.cpu().numpy()
    keep = p.keep.cpu().numpy()
    for b in range(2):
        n = cnt[b]
        order = np.lexsort((cidx[b, :n], -cscore[b, :n].astype(np.float64)))
        boxes = (cbox[b, :n] + ccls[b, :n, None] * np.float32(4096)).astype(np.float32)[order]
        k = cnative.nms(boxes, cscore[b, :n][order], 0.45)[:300]
        np.testing.assert_array_equal(order[k], keep[b, :nd[b]])


def test_fused_detect_forward_equals_plain_forward():
    """y7t_det_forward_fused: the Detect 1x1 convs decode + filter in their epilogue (the head tensors are never written) and
    y7t_det_postprocess(head = NULL) starts at the rank sort -- candidate counts, detections and classes must equal the plain
    forward + decode pass; the raw heads can still be materialised afterwards and equal the plain forward's bit for bit."""
    det = build("yolov7-w6", 10, (256, 320), 2)
    g = torch.Generator().manual_seed(8)
    img = torch.rand((2, 3, 256, 320), generator=g)
    det.plant_objectness_bias(img.cuda(), target=800)
    out_a = det(img)[0]
    raw_a = [t.clone() for t in out_a.raw()]
    d_a, n_a = det.postprocess(out_a, 0.01, 0.45, ori_shapes=[(200, 300), (256, 320)])
    d_a, n_a, c_a = d_a.clone(), n_a.clone(), det.plan.post[0].cand.clone()
    for t in range(len(det.plan.heads)):
        det.head_tensor(t, 2).zero_()                                   # a fused forward must not need (or write) them
    out_b = det.forward(img, fuse_decode=0.01, pset=1)
    d_b, n_b = det.postprocess(out_b, 0.01, 0.45, ori_shapes=[(200, 300), (256, 320)])
    torch.cuda.synchronize()
    assert all(float(det.head_tensor(t, 2).abs().max()) == 0.0 for t in range(len(det.plan.heads)))
    assert torch.equal(n_a, n_b) and int(n_a.min()) > 20 and torch.equal(c_a, det.plan.post[1].cand) and int(c_a.min()) > 300
    for b in range(2):
        # (at this size the plain Detect convs run split-K, the fused ones do not: the fp32 logits may differ in the last bit)
        a, bb = d_a[b, :n_a[b]], d_b[b, :n_b[b]]
        assert torch.equal(a[:, 5], bb[:, 5]) and (a[:, :4] - bb[:, :4]).abs().max() <= 1.0 and (a[:, 4] - bb[:, 4]).abs().max() <= 1e-5
        assert ((a[:, :4] - bb[:, :4]).abs() > 0).float().mean() < 0.01
    assert all(torch.equal(x, y) for x, y in zip(raw_a, out_b.raw()))      # lazily re-run Detect convs
    with pytest.raises(ValueError):
        det.postprocess(out_b, 0.25, 0.45, None)                          # the threshold was fixed at forward time
    det(img)
    with pytest.raises(Exception):
        det._materialise_heads(out_b)                                     # the arena has moved on


@pytest.mark.parametrize("B,H,W,act,kw", [(1, 4, 64, 1, {}), (2, 8, 128, 2, {"in_ld": 128, "in_coff": 64, "out_ld": 256, "out_coff": 128}), (3, 64, 192, 1, {}), (1, 640, 640, 1, {})],
                         ids=["one-tile", "slices-leaky", "many-tiles", "640x640"])
def test_stride2_weights_stationary_with_the_twin_1x1_behind_it(L, B, H, W, act, kw):
    """WS_S2_TWIN through the C ABI (y7t_conv2d_nhwc_f16, act bit 19): 3x3 / stride 2 64 -> 128 + activation, then -- on the tile in LDS, the tensor between the layers never
    reaches memory -- the 128 -> 128 1x1 convolution + activation.  Reference: the two layers one after the other in fp32 on the fp16 weights, middle tensor rounded to fp16."""
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.detector import weights
    in_ld, in_coff = kw.get("in_ld", 64), kw.get("in_coff", 0)
    out_ld, out_coff = kw.get("out_ld", 128), kw.get("out_coff", 0)
    rng = np.random.default_rng(B * 1000 + H + W + 11)
    x = rng.normal(0, 1, (B, H, W, in_ld)).astype(np.float16)
    W1 = (rng.normal(0, 1, (128, 64, 3, 3)) / np.sqrt(576)).astype(np.float32)
    W2 = (rng.normal(0, 1, (128, 128, 1, 1)) / np.sqrt(128)).astype(np.float32)
    b1, b2 = rng.normal(0, 0.5, 128).astype(np.float32), rng.normal(0, 0.5, 128).astype(np.float32)
    wp = np.concatenate([weights.pack_ws_s2(W1.transpose(0, 2, 3, 1).reshape(128, 576).astype(np.float16)).ravel(),
                         weights.pack_ws_s2_tail(W2.reshape(128, 128).astype(np.float16)).ravel()])
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(wp).cuda(), torch.from_numpy(np.concatenate([b1, b2])).cuda()
    out = torch.full((B, H // 2, W // 2, out_ld), 7.0, dtype=torch.float16, device="cuda")
    zeros = torch.zeros(128, dtype=torch.float16, device="cuda")
    _lib.check(L.y7t_conv2d_nhwc_f16(_lib.ptr(xd), in_ld, in_coff, B, H, W, 64, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out), out_ld, out_coff, 0, 128, 128, 3, 3, 2, 1,
                                     act | act_bits(WL.WS_S2_TWIN), _lib.ptr(zeros), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert L.y7t_last_kernel().decode() == "ws_s2<2,32> + 1x1"
    f = F.silu if act == 1 else (lambda t: F.leaky_relu(t, 0.1))
    xs = torch.from_numpy(x[..., in_coff:in_coff + 64].astype(np.float32)).permute(0, 3, 1, 2).cuda()
    mid = f(F.conv2d(xs, torch.from_numpy(W1.astype(np.float16).astype(np.float32)).cuda(), torch.from_numpy(b1).cuda(), stride=2, padding=1)).half().float()
    ref = f(F.conv2d(mid, torch.from_numpy(W2.astype(np.float16).astype(np.float32)).cuda(), torch.from_numpy(b2).cuda())).permute(0, 2, 3, 1).cpu().numpy()
    got = out.float().cpu().numpy()
    # the 1-ulp differences of the fp16 tensor between the layers (the device sums in another order than cuDNN-style fp32 conv) reach the output through 128 weights of
    # size ~ 1 / sqrt(128): a few 1e-4 of the output scale, on top of the output's own fp16 rounding
    np.testing.assert_allclose(got[..., out_coff:out_coff + 128], ref, rtol=2e-3, atol=2e-3)
    mask = np.ones(out_ld, bool); mask[out_coff:out_coff + 128] = False
    assert np.all(got[..., mask] == 7.0)


def test_upsample_on_read_equals_materialised_upsample(monkeypatch):
    """nn.Upsample folded into the consuming 1x1 convs' loader (cfg/deploy/yolov7-w6.yaml:75,89,103) changes no value: heads bit-exact
    against the plan that materialises the three upsampled tensors"""
    img = torch.rand((2, 3, 256, 320), generator=torch.Generator().manual_seed(9))
    det = build("yolov7-w6", 10, (256, 320), 2)
    assert sum(int(o["up_C"]) > 0 for o in det.plan.ops) == 3 and not any(int(o["type"]) == 1 for o in det.plan.ops)
    a = [t.clone() for t in det(img)[0].raw()]
    monkeypatch.setenv("Y7T_UPSAMPLE_ON_READ", "0")
    ref = build("yolov7-w6", 10, (256, 320), 2)
    assert sum(int(o["type"]) == 1 for o in ref.plan.ops) == 3
    b = ref(img)[0].raw()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_fused_stem_equals_layout_plus_conv(monkeypatch):
    """uint8 frame -> [letterbox] -> BGR->RGB, /255, ReOrg -> stem conv as ONE kernel (y7t_det_forward_stem_u8) against the three-step
    path (y7t_letterbox_layout_u8 / y7t_input_layout, then op 0): the same MFMA K order, so the heads must be equal bit for bit --
    native-size frames, padded frames (360 x 640 -> 384 x 640) and resampled frames (540 x 960 -> 384 x 640)"""
    g = torch.Generator().manual_seed(12)
    det = build("yolov7-w6", 10, (256, 320), 2)
    assert det.plan.stem_fused and det.launch_list is not None
    frames = torch.randint(0, 256, (2, 256, 320, 3), dtype=torch.uint8, generator=g)
    small = torch.randint(0, 256, (2, 360, 640, 3), dtype=torch.uint8, generator=g)
    big = torch.randint(0, 256, (2, 540, 960, 3), dtype=torch.uint8, generator=g)
    a0 = [t.clone() for t in det(frames.cuda())[0].raw()]
    assert det.launch_list(2)[0].startswith("stem_u8")
    a0b = [t.clone() for t in det(frames.cuda())[0].raw()]
    assert all(torch.equal(x, y) for x, y in zip(a0, a0b))
    a1 = [t.clone() for t in det.forward_frames(small, img_size=640)[0].raw()]
    a2 = [t.clone() for t in det.forward_frames(big, img_size=640)[0].raw()]
    monkeypatch.setenv("Y7T_STEM_FUSED", "0")
    ref = build("yolov7-w6", 10, (256, 320), 2)
    assert not ref.plan.stem_fused
    assert all(torch.equal(x, y) for x, y in zip(a0, ref(frames.cuda())[0].raw()))
    assert all(torch.equal(x, y) for x, y in zip(a1, ref.forward_frames(small, img_size=640)[0].raw()))
    assert all(torch.equal(x, y) for x, y in zip(a2, ref.forward_frames(big, img_size=640)[0].raw()))
    assert float(a0[0].abs().max()) > 0 and float(a2[0].abs().max()) > 0


def test_head_output_behaves_like_the_reference_tensor():
    """`pred = model(img)[0]` is a (B, A, 5+nc) tensor in the reference (models/yolo.py:57); here it is a device handle that turns into
    that tensor on request: indexing, numpy conversion, .cpu() -- all equal to the oracle's Detect decode of the raw heads"""
    from oracle import detector_torch as dt
    det = build("yolov7-tiny", 80, (128, 192), 2)
    pred = det(torch.rand((2, 3, 128, 192), generator=torch.Generator().manual_seed(10)))[0]
    want = dt.decode_heads([r.cpu() for r in pred.raw()], det.spec["anchors"], 128)
    assert tuple(pred.shape) == tuple(want.shape) == (2, 3 * (16 * 24 + 8 * 12 + 4 * 6), 85)
    assert torch.allclose(pred.cpu(), want, rtol=1e-5, atol=1e-4)
    assert torch.allclose(pred[1].cpu(), want[1], rtol=1e-5, atol=1e-4)
    assert torch.allclose((pred[..., 4] > 0.5).cpu().float(), (want[..., 4] > 0.5).float())
    np.testing.assert_allclose(np.asarray(pred), want.numpy(), rtol=1e-5, atol=1e-4)
    assert len(pred) == 2


def test_attempt_load_state_dict_checkpoint(tmp_path):
    """attempt_load (models/experimental.py:83-106 seam) on a state-dict checkpoint with reference-style parameter names
    ({'model': state_dict} as the reference's training code saves, plus a bare state dict): same network, bit for bit"""
    from yolov7_tracker_amd.detector import attempt_load
    ref = build("yolov7-tiny", 80, (128, 128), 1, seed=3)
    img = torch.rand((1, 3, 128, 128), generator=torch.Generator().manual_seed(4))
    want = [t.clone() for t in ref(img)[0].raw()]
    for name, payload in (("wrapped.pt", {"model": ref._sd, "epoch": 7}), ("bare.pt", dict(ref._sd))):
        path = str(tmp_path / name)
        torch.save(payload, path)
        det = attempt_load(path, cfg="yolov7-tiny", nc=80, img_size=128)
        got = det(img)[0].raw()
        assert all(torch.equal(a, b) for a, b in zip(got, want)), name
    with pytest.raises(ValueError):
        attempt_load(str(tmp_path / "bare.pt"), img_size=128)          # a bare state dict needs the architecture
    with pytest.raises(FileNotFoundError):
        attempt_load(str(tmp_path / "missing.pt"), cfg="yolov7-tiny")
