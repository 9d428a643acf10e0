"""GPU: the memory-bound detector kernels of csrc/y7t_post.hip one by one and bit-exact -- the max-pools (LDS and generic forms, the fused SPP cascade and the
rules of forward_impl that choose between them), the nearest x2 upsample and the input layout kernels -- at the smallest shapes that reach each code path.

The pools and the upsample run as plans of one to three `y7t_op`s over an arena the test owns (y7t_det_create / y7t_det_forward_ops); the reference is
torch.nn.functional on the same fp16 values widened to fp32.  Max and copy do not round, so equality is torch.equal; outside the output slices the arena must
keep its sentinel; every case asserts y7t_last_kernel(), so a dispatch change cannot silently move a case to another kernel.

Input data: normal values around -3 (most windows are all-negative: a zero-initialised maximum fails), distinct within every channel plane (an off-by-one
window fails), seeded by the case like CONV_CASES of tests/test_detector_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import op_refs

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
CONV, UP, POOL = 0, 1, 2
E_ARG = -1


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ data
def _fp16_pool():
    """every fp16 value in [-6, -2^-6] and [2^-6, 1], with the weight a normal(-3, 1) density gives its rounding interval"""
    v = np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(np.float64)
    v = np.unique(v[np.isfinite(v) & (((v >= -6) & (v <= -2.0 ** -6)) | ((v >= 2.0 ** -6) & (v <= 1)))])
    gap = np.gradient(v)
    return v, -0.5 * (v + 3.0) ** 2 + np.log(gap)


_POOL_V, _POOL_LOGW = _fp16_pool()


def plane_distinct_fp16(rng, B, H, W, ld):
    """(B, H, W, ld) float16, ~normal(-3, 1); the H * W values of every (image, channel) plane are pairwise distinct (weighted sampling without replacement
    from the fp16 values themselves: Gumbel top-k).  Planes too many or too large for that fall back to plain rounded normals."""
    hw, planes = H * W, B * ld
    if hw > len(_POOL_V) // 2 or planes * len(_POOL_V) > 4_000_000:
        return rng.normal(-3, 1, (B, H, W, ld)).astype(np.float16)
    keys = _POOL_LOGW[None, :] + rng.gumbel(size=(planes, len(_POOL_V)))
    idx = np.argpartition(-keys, hw - 1, axis=1)[:, :hw]
    idx = rng.permuted(idx, axis=1)
    return _POOL_V[idx].reshape(B, ld, H, W).transpose(0, 2, 3, 1).astype(np.float16)


def test_the_input_data_cannot_excuse_a_wrong_kernel():
    x = plane_distinct_fp16(np.random.default_rng(0), 2, 14, 18, 48).astype(np.float32)
    planes = x.transpose(0, 3, 1, 2).reshape(96, -1)
    assert all(len(np.unique(p)) == p.size for p in planes)
    assert -3.3 < x.mean() < -2.7 and (x > 0).mean() < 0.02
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    assert float((F.max_pool2d(t, 5, 1, 2) < 0).float().mean()) > 0.9            # most windows all-negative


# ------------------------------------------------------------------------------------------------ plans over an arena of the test's own
class Arena:
    """fp16 NHWC buffers for `B` images in one device allocation, 256-byte aligned with 256 bytes of sentinel between them; everything starts as SENTINEL"""

    def __init__(self, shapes, B):
        self.B, self.shapes, self.offsets = B, shapes, []
        o = 256
        for (H, W, ld) in shapes:
            self.offsets.append(o)
            o = (o + 2 * B * H * W * ld + 255) // 256 * 256 + 256
        self.mem = torch.full((o // 2,), SENTINEL, dtype=torch.float16, device="cuda")
        self.dummy_w = torch.zeros(1, dtype=torch.float16, device="cuda")
        self.dummy_b = torch.zeros(1, dtype=torch.float32, device="cuda")

    def view(self, i):
        H, W, ld = self.shapes[i]
        o = self.offsets[i] // 2
        return self.mem[o:o + self.B * H * W * ld].view(self.B, H, W, ld)


def make_op(typ, in_buf, in_ld, in_coff, H, W, C, out_buf, out_ld, out_coff, k=0, s=1, p=0):
    from yolov7_tracker_amd.detector import graph
    op = np.zeros((), graph.OP_DTYPE)
    op["type"], op["in_buf"], op["in_ld"], op["in_coff"], op["H"], op["W"], op["Cin"] = typ, in_buf, in_ld, in_coff, H, W, C
    op["out_buf"], op["out_ld"], op["out_coff"], op["Cout"] = out_buf, out_ld, out_coff, C
    op["Ho"], op["Wo"] = (2 * H, 2 * W) if typ == UP else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    op["KH"], op["KW"], op["stride"], op["pad"], op["detect_level"] = k, k, s, p, -1
    return op


class Plan:
    def __init__(self, L, ops, arena):
        from yolov7_tracker_amd import _lib
        from yolov7_tracker_amd.detector import graph
        self.L, self.arena = L, arena
        self.ops = np.array(ops, dtype=graph.OP_DTYPE)
        self.offs = np.array(arena.offsets, dtype=np.int64)
        self.h = ctypes.c_void_p()
        _lib.check(L.y7t_det_create(self.ops.ctypes.data_as(ctypes.c_void_p), len(self.ops), self.offs.ctypes.data_as(ctypes.c_void_p), len(self.offs),
                                    _lib.ptr(arena.mem), arena.mem.numel() * 2, _lib.ptr(arena.dummy_w), _lib.ptr(arena.dummy_b), arena.B, ctypes.byref(self.h)))

    def run(self, first=0, last=-1):
        """-> (return code, name of the last kernel launched)"""
        from yolov7_tracker_amd import _lib
        rc = self.L.y7t_det_forward_ops(self.h, self.arena.B, first, last, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, self.L.y7t_last_kernel().decode()

    def close(self):
        self.L.y7t_det_destroy(self.h)


def _report(kernel, case):
    """one line per case: the kernel it ran (profiles/op_tests_margins.txt keeps the listing of one run)"""
    print("MARGIN %-44s %-60s exact" % (kernel, case))


def _ref(x_nhwc_f16, typ, k, s, p):
    x = x_nhwc_f16.float().cpu().permute(0, 3, 1, 2)
    r = F.interpolate(x, scale_factor=2, mode="nearest") if typ == UP else F.max_pool2d(x, k, s, p)
    return r.permute(0, 2, 3, 1)


def _assert_sentinel_outside(arena, written):
    """`written`: {buffer: [(c0, c1), ...]} channel ranges the plan may have written (inputs included: the test wrote them)"""
    left = arena.mem.clone()
    for i, (H, W, ld) in enumerate(arena.shapes):
        o = arena.offsets[i] // 2
        v = left[o:o + arena.B * H * W * ld].view(arena.B, H, W, ld)
        for c0, c1 in written.get(i, []):
            v[..., c0:c1] = SENTINEL
    assert bool((left == SENTINEL).all()), "%d values outside the output slices were overwritten" % int((left != SENTINEL).sum())


def run_single(L, typ, shape, k=0, s=1, p=0, in_ld=None, in_coff=0, out_ld=None, out_coff=0, same_buf=False, kernel=None):
    """one op on its own plan: input slice of buffer 0, output slice of buffer 1 (or of buffer 0 again: same_buf); asserts the kernel's name, the result, the untouched input and the sentinel everywhere else"""
    B, H, W, C = shape
    in_ld, out_ld = in_ld or C, out_ld or C
    op = make_op(typ, 0, in_ld, in_coff, H, W, C, 0 if same_buf else 1, in_ld if same_buf else out_ld, out_coff, k, s, p)
    Ho, Wo = int(op["Ho"]), int(op["Wo"])
    if same_buf:
        assert (Ho, Wo) == (H, W) and (in_coff + C <= out_coff or out_coff + C <= in_coff)
    arena = Arena([(H, W, in_ld)] if same_buf else [(H, W, in_ld), (Ho, Wo, out_ld)], B)
    rng = np.random.default_rng(hash((typ,) + tuple(shape) + (k, s, p, in_ld, in_coff, out_ld, out_coff)) % 2 ** 32)
    x = torch.from_numpy(plane_distinct_fp16(rng, B, H, W, C)).cuda()
    arena.view(0)[..., in_coff:in_coff + C] = x
    plan = Plan(L, [op], arena)
    try:
        rc, name = plan.run()
    finally:
        plan.close()
    assert rc == 0 and name == kernel, (rc, name)
    ob = 0 if same_buf else 1
    got = arena.view(ob)[..., out_coff:out_coff + C]
    want = _ref(x, typ, k, s, p)
    assert torch.equal(got.float().cpu(), want), "%s %s: %d values differ" % (name, shape, int((got.float().cpu() != want).sum()))
    assert torch.equal(arena.view(0)[..., in_coff:in_coff + C], x)                  # the input is read only
    written = {0: [(in_coff, in_coff + C)]}
    written.setdefault(ob, []).append((out_coff, out_coff + C))
    _assert_sentinel_outside(arena, written)
    _report(name, "%s k%d s%d p%d in %d+%d/%d out %d+%d/%d%s" % (shape, k, s, p, in_coff, C, in_ld, out_coff, C, in_ld if same_buf else out_ld, " same buffer" if same_buf else ""))
    return name


# ------------------------------------------------------------------------------------------------ max-pools
LDS_SHAPES = [(1, 5, 7, 16),        # every window wider than the map
              (2, 14, 18, 48),      # the 13-window smaller than the map both ways; three 16-channel groups, two images
              (1, 32, 32, 16)]      # H * W = 1024: all 65 536 bytes of dynamic LDS the dispatcher admits


@pytest.mark.parametrize("K", [5, 9, 13])
@pytest.mark.parametrize("shape", LDS_SHAPES)
def test_maxpool_lds(L, shape, K):
    run_single(L, POOL, shape, K, 1, K // 2, kernel="maxpool<%d,1> lds" % K)


@pytest.mark.parametrize("K", [5, 9, 13])
def test_maxpool_lds_slices_of_wider_buffers(L, K):
    run_single(L, POOL, (2, 14, 18, 48), K, 1, K // 2, in_ld=64, in_coff=16, out_ld=96, out_coff=32, kernel="maxpool<%d,1> lds" % K)
    run_single(L, POOL, (2, 14, 18, 16), K, 1, K // 2, in_ld=64, in_coff=16, out_coff=48, same_buf=True, kernel="maxpool<%d,1> lds" % K)      # SPP's concat buffer
    run_single(L, POOL, (1, 5, 7, 16), K, 1, K // 2, in_ld=64, in_coff=32, out_coff=0, same_buf=True, kernel="maxpool<%d,1> lds" % K)


@pytest.mark.parametrize("shape,K", [((1, 33, 32, 16), 5), ((1, 33, 32, 16), 13),      # one pixel over the LDS limit
                                     ((2, 14, 18, 24), 9),                            # C % 16 != 0
                                     ((1, 40, 40, 32), 13),                           # yolov7-tiny's stride-32 map at 1280 x 1280
                                     ((3, 512, 512, 24), 5)])                         # 2 359 296 work items > 8192 * 256 threads: the grid-stride loop's second round
def test_maxpool_generic_stride1(L, shape, K):
    run_single(L, POOL, shape, K, 1, K // 2, kernel="maxpool<%d,1>" % K)


def test_maxpool_2x2_stride2(L):
    run_single(L, POOL, (2, 16, 24, 32), 2, 2, 0, kernel="maxpool<2,2>")
    run_single(L, POOL, (1, 15, 21, 8), 2, 2, 0, kernel="maxpool<2,2>")                                       # odd sizes: floor
    run_single(L, POOL, (2, 15, 21, 24), 2, 2, 0, in_ld=40, in_coff=8, out_ld=64, out_coff=32, kernel="maxpool<2,2>")


def test_maxpool_1x1_is_the_concat_copy(L):
    run_single(L, POOL, (2, 9, 11, 40), 1, 1, 0, in_ld=48, in_coff=8, out_ld=96, out_coff=48, kernel="maxpool<1,1>")


# ------------------------------------------------------------------------------------------------ the SPP cascade and forward_impl's fusion rules
def _spp_plan(L, shape, in_coff, out_coff, ld):
    """three chained 5 x 5 / 1 pools in ONE buffer as detector/graph.py emits them for SPPCSPC: pool i reads the slice pool i - 1 wrote and writes the next one"""
    B, H, W, C = shape
    arena = Arena([(H, W, ld)], B)
    ops = [make_op(POOL, 0, ld, in_coff if i == 0 else out_coff + (i - 1) * C, H, W, C, 0, ld, out_coff + i * C, 5, 1, 2) for i in range(3)]
    x = torch.from_numpy(plane_distinct_fp16(np.random.default_rng(hash(tuple(shape) + (in_coff, out_coff, ld)) % 2 ** 32), B, H, W, C)).cuda()
    arena.view(0)[..., in_coff:in_coff + C] = x
    return arena, Plan(L, ops, arena), x


def _spp_check(arena, x, shape, in_coff, out_coff, input_survives=True):
    C = shape[3]
    for i, K in enumerate((5, 9, 13)):                                    # 5 o 5 o 5 == the 5 / 9 / 13 pools of the input (models/common.py:262-280)
        got = arena.view(0)[..., out_coff + i * C:out_coff + (i + 1) * C].float().cpu()
        assert torch.equal(got, _ref(x, POOL, K, 1, K // 2)), "slice %d (k = %d)" % (i, K)
    written = [(out_coff, out_coff + 3 * C)]
    if input_survives:
        assert torch.equal(arena.view(0)[..., in_coff:in_coff + C], x)
        written.append((in_coff, in_coff + C))
    _assert_sentinel_outside(arena, {0: written})


@pytest.mark.parametrize("shape", [(2, 20, 20, 32), (1, 32, 32, 16), (1, 3, 4, 16)])
def test_spp3_fused_cascade_and_the_cut_chain(L, shape):
    C = shape[3]
    arena, plan, x = _spp_plan(L, shape, 0, C, 4 * C + 8)
    try:
        rc, name = plan.run(0, 3)
        assert rc == 0 and name == "spp3<5,5,5> lds", (rc, name)
        _spp_check(arena, x, shape, 0, C)
        fused = arena.view(0).clone()
        # a range that cuts the chain: single pools, bit-identical results
        arena.view(0)[..., C:4 * C] = SENTINEL
        rc, name = plan.run(0, 2)
        assert rc == 0 and name == "maxpool<5,1> lds", (rc, name)
        assert bool((arena.view(0)[..., 3 * C:4 * C] == SENTINEL).all())            # the third pool has not run
        rc, name = plan.run(2, 3)
        assert rc == 0 and name == "maxpool<5,1> lds", (rc, name)
        _spp_check(arena, x, shape, 0, C)
        assert torch.equal(arena.view(0), fused)
        _report("spp3<5,5,5> lds == 3 x maxpool<5,1> lds", "%s chain cut at op 2" % (shape,))
    finally:
        plan.close()


def test_spp3_declines_overlapping_slices(L):
    """the chain's input slice is the slice its third pool writes: the in-place guard of forward_impl declines the fused launch; three launches in order are correct"""
    shape, C = (2, 20, 20, 32), 32
    arena, plan, x = _spp_plan(L, shape, 2 * C, 0, 3 * C + 8)
    try:
        names = []
        for i in range(3):                                                 # the launch list of the plan, op by op ...
            rc, name = plan.run(i, i + 1)
            assert rc == 0
            names.append(name)
        assert names == ["maxpool<5,1> lds"] * 3
        _spp_check(arena, x, shape, 2 * C, 0, input_survives=False)
        arena.view(0)[...] = SENTINEL
        arena.view(0)[..., 2 * C:3 * C] = x
        rc, name = plan.run(0, 3)                                          # ... and in one call: the whole chain is in range, the guard must decline the fusion
        assert rc == 0 and name == "maxpool<5,1> lds", (rc, name)
        _spp_check(arena, x, shape, 2 * C, 0, input_survives=False)
        _report("3 x maxpool<5,1> lds (fusion declined)", "%s input slice = third output slice" % (shape,))
    finally:
        plan.close()


def test_spp3_falls_back_to_three_launches(L):
    """shapes the fused kernel cannot run (y7t_spp3_try answers 1): C % 16 != 0, and a map over the LDS limit -- three generic launches, same results"""
    for shape in [(2, 14, 18, 24), (1, 33, 32, 16)]:
        C = shape[3]
        arena, plan, x = _spp_plan(L, shape, 0, C, 4 * C)
        try:
            rc, name = plan.run(0, 3)
            assert rc == 0 and name == "maxpool<5,1>", (rc, name)
            _spp_check(arena, x, shape, 0, C)
            _report("3 x maxpool<5,1> (spp3 cannot run the shape)", "%s" % (shape,))
        finally:
            plan.close()


# ------------------------------------------------------------------------------------------------ upsample
def test_upsample2x(L):
    run_single(L, UP, (2, 5, 7, 8), kernel="upsample2x")
    run_single(L, UP, (1, 20, 20, 72), in_ld=96, in_coff=16, out_ld=128, out_coff=40, kernel="upsample2x")
    run_single(L, UP, (2, 80, 80, 512), kernel="upsample2x")              # 3 276 800 16-byte items > 8192 * 256 threads: the grid-stride loop's second round


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("typ,k,p", [(POOL, 5, 2), (POOL, 2, 0), (UP, 0, 0)])
@pytest.mark.parametrize("bad", ["C", "in_coff", "out_coff", "in_ld", "out_ld"])
def test_misaligned_channels_are_refused_and_nothing_is_written(L, typ, k, p, bad):
    a = dict(C=16, in_ld=32, in_coff=8, out_ld=32, out_coff=8)
    a[bad] = {"C": 12, "in_coff": 4, "out_coff": 12, "in_ld": 36, "out_ld": 28}[bad]
    H, W, s = 6, 8, 2 if k == 2 else 1
    op = make_op(typ, 0, a["in_ld"], a["in_coff"], H, W, a["C"], 1, a["out_ld"], a["out_coff"], k, s, p)
    arena = Arena([(H, W, a["in_ld"]), (int(op["Ho"]), int(op["Wo"]), a["out_ld"])], 2)
    plan = Plan(L, [op], arena)
    try:
        rc, _ = plan.run()
    finally:
        plan.close()
    assert rc == E_ARG and b"channel alignment" in L.y7t_last_error()
    assert bool((arena.mem == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ input layout
def _layout(L, img, is_u8, reorg, ldout):
    """y7t_input_layout on a host array -> (B, Ho, Wo, ldout) float16 numpy; the 4096 sentinel values behind the tensor must survive"""
    from yolov7_tracker_amd import _lib
    B = img.shape[0]
    H, W = (img.shape[1], img.shape[2]) if is_u8 else (img.shape[2], img.shape[3])
    Ho, Wo = (H // 2, W // 2) if reorg else (H, W)
    n = B * Ho * Wo * ldout
    out = torch.full((n + 4096,), SENTINEL, dtype=torch.float16, device="cuda")
    d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    _lib.check(L.y7t_input_layout(_lib.ptr(d), int(is_u8), B, H, W, int(reorg), _lib.ptr(out), ldout, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all())
    return out[:n].view(B, Ho, Wo, ldout).cpu().numpy()


def _layout_kernel(is_u8, reorg, W):
    """the launcher's rule (y7t_input_layout sets no kernel name): csrc/y7t_post.hip"""
    return "k_input_layout_u8_reorg4" if is_u8 and reorg and W % 8 == 0 else "k_input_layout<%s>%s" % ("true" if is_u8 else "false", " reorg" if reorg else "")


def _image(rng, is_u8, B, H, W):
    return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) if is_u8 else rng.random((B, 3, H, W), dtype=np.float32)


LAYOUT_CASES = [
    # is_u8, reorg, ldout, H, W
    (0, 0, 8, 10, 14),            # k_input_layout<false>, yolov7-tiny's input
    (0, 1, 16, 10, 14),           # ... with ReOrg
    (1, 0, 8, 9, 13),             # k_input_layout<true>
    (1, 1, 16, 10, 24),           # k_input_layout_u8_reorg4 (W % 8 == 0)
    (1, 1, 16, 10, 26),           # k_input_layout<true> with ReOrg: the generic path behind the fast one
]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", LAYOUT_CASES)
def test_input_layout(L, case, B):
    is_u8, reorg, ldout, H, W = case
    img = _image(np.random.default_rng(hash(case + (B,)) % 2 ** 32), is_u8, B, H, W)
    got, want = _layout(L, img, is_u8, reorg, ldout), op_refs.input_layout(img, is_u8, reorg, ldout)
    c = 12 if reorg else 3
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))                # bit-equal: also the sign of a zero
    assert not got[..., c:].view(np.uint16).any()                                   # pad channels exactly +0
    _report(_layout_kernel(is_u8, reorg, W), "B%d %dx%d ldout %d" % (B, H, W, ldout))


@pytest.mark.parametrize("is_u8,reorg,ldout,H,W,B", [(1, 1, 16, 1536, 1536, 1),      # the fast path at a frame-sized input
                                                     (0, 0, 8, 1536, 1536, 1),      # 2 359 296 pixels > 8192 * 256 threads: k_input_layout<false>'s grid-stride loop
                                                     (1, 0, 8, 1536, 1536, 1),      # ... and k_input_layout<true>'s
                                                     (1, 1, 16, 2902, 2902, 1)])    # ... and with ReOrg (1451^2 = 2 105 401 output pixels), W % 8 != 0
def test_input_layout_frame_sized(L, is_u8, reorg, ldout, H, W, B):
    img = _image(np.random.default_rng(hash((is_u8, reorg, ldout, H, W, B)) % 2 ** 32), is_u8, B, H, W)
    got, want = _layout(L, img, is_u8, reorg, ldout), op_refs.input_layout(img, is_u8, reorg, ldout)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    _report(_layout_kernel(is_u8, reorg, W), "B%d %dx%d ldout %d" % (B, H, W, ldout))


def test_input_layout_fast_path_grid_stride(L):
    """k_input_layout_u8_reorg4 launches at most 16384 * 256 threads, one per 8 x 2 pixel block: its grid-stride loop runs a second round only above 67 108 864
    pixels (1536 x 1536 is 147 456 blocks).  One 8208 x 8208 frame has 4 210 704 blocks; the rows of the second round are the last 16 output rows.  Compared with the
    numpy reference: the first 8 and the last 40 output rows; the whole tensor against the same 256 numpy values gathered on the device."""
    from yolov7_tracker_amd import _lib
    H = W = 8208
    g = torch.Generator(device="cuda").manual_seed(H)
    img = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    n = (H // 2) * (W // 2) * 16
    out = torch.full((n + 4096,), SENTINEL, dtype=torch.float16, device="cuda")
    _lib.check(L.y7t_input_layout(_lib.ptr(img), 1, 1, H, W, 1, _lib.ptr(out), 16, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all())
    got = out[:n].view(1, H // 2, W // 2, 16)
    for r0, r1 in ((0, 8), (H // 2 - 40, H // 2)):
        want = op_refs.input_layout(img[:, 2 * r0:2 * r1].cpu().numpy(), 1, 1, 16)
        assert np.array_equal(got[:, r0:r1].cpu().numpy().view(np.uint16), want.view(np.uint16)), (r0, r1)
    lut = torch.from_numpy((np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float16)).cuda()      # the 256 values there are, from numpy
    f = torch.index_select(lut, 0, img.flip(-1).reshape(-1).int()).view(1, H, W, 3)  # (1, H, W, 3) RGB
    want = torch.cat([f[:, 0::2, 0::2], f[:, 1::2, 0::2], f[:, 0::2, 1::2], f[:, 1::2, 1::2]], -1)
    assert torch.equal(got[..., :12], want) and not bool(got[..., 12:].any())
    _report("k_input_layout_u8_reorg4", "B1 %dx%d ldout 16 (grid stride)" % (H, W))


@pytest.mark.parametrize("B", [1, 3])
def test_input_layout_fast_and_generic_paths_agree(L, B):
    """W = 24 takes k_input_layout_u8_reorg4; the same pixels inside a 26-wide image take k_input_layout<true>: identical tensors on the shared columns"""
    rng = np.random.default_rng(24 + B)
    img = rng.integers(0, 256, (B, 12, 24, 3), dtype=np.uint8)
    wide = rng.integers(0, 256, (B, 12, 26, 3), dtype=np.uint8)
    wide[:, :, :24] = img
    fast, generic = _layout(L, img, 1, 1, 16), _layout(L, wide, 1, 1, 16)
    assert np.array_equal(fast.view(np.uint16), generic[:, :, :12].view(np.uint16))
    _report("k_input_layout_u8_reorg4 == k_input_layout<true> reorg", "B%d 12x24 inside 12x26" % B)


def test_input_layout_refusals(L):
    from yolov7_tracker_amd import _lib
    img = torch.zeros((1, 6, 6, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), SENTINEL, dtype=torch.float16, device="cuda")
    for H, W, reorg, ld in [(6, 6, 0, 12), (6, 6, 1, 8), (5, 6, 1, 16), (6, 5, 1, 16)]:
        assert L.y7t_input_layout(_lib.ptr(img), 1, 1, H, W, reorg, _lib.ptr(out), ld, _lib.stream_ptr()) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
