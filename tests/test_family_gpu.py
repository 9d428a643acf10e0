"""GPU: the YOLOv7 family beyond w6 / tiny on the device -- the add kernel (Y7T_OP_ADD) as a one-op plan, every op of the five graphs teacher-forced, the raw heads
of the whole networks against goldens recorded from the reference, the convolution shapes the new graphs bring, and the tracker CLI on two of the graphs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import family_ref as fr
from tests import family_teacher, util
from yolov7_tracker_amd.detector.layout import layout_of

pytestmark = pytest.mark.gpu

ADD = 3
E_ARG = -1


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ a. the add kernel
def _special_fp16(rng, shape):
    """fp16 values that try an adder: normals of every magnitude, subnormals, +-65504, pairs that overflow to +-inf, and -- planted by the caller -- x + (-x)"""
    n = int(np.prod(shape))
    v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 5, n)
    kind = rng.integers(0, 8, n)
    v[kind == 0] = rng.integers(-1023, 1024, int((kind == 0).sum())) * 2.0 ** -24            # subnormals (and zero)
    v[kind == 1] = rng.choice([65504.0, -65504.0, 40000.0, -40000.0], int((kind == 1).sum()))  # sums of these pass +-65504
    return np.clip(v, -65504, 65504).astype(np.float16).reshape(shape)


def _add_op(a_buf, a_ld, a_coff, b_buf, b_ld, b_coff, H, W, C, out_buf, out_ld, out_coff):
    from tests.test_membound_gpu import make_op
    op = make_op(ADD, a_buf, a_ld, a_coff, H, W, C, out_buf, out_ld, out_coff)
    op["Ho"], op["Wo"] = H, W
    op["up_buf"], op["up_ld"], op["up_coff"] = b_buf, b_ld, b_coff
    return op


def _run_add(L, B, H, W, C, a, b, out, seed, expect_rc=0):
    """a, b, out: (buffer, ld, coff); buffers are created as wide as their `ld`.  -> nothing; asserts"""
    from tests.test_membound_gpu import Arena, Plan, SENTINEL, _assert_sentinel_outside
    lds = {}
    for buf, ld, _ in (a, b, out):
        assert lds.setdefault(buf, ld) == ld or expect_rc
    arena = Arena([(H, W, lds[i]) for i in sorted(lds)], B)
    rng = np.random.default_rng(seed)
    xa = _special_fp16(rng, (B, H, W, C))
    xb = _special_fp16(rng, (B, H, W, C))
    flat = xb.reshape(-1)
    flat[::7] = -xa.reshape(-1)[::7]                                                          # x + (-x)
    if expect_rc == 0:
        arena.view(a[0])[..., a[2]:a[2] + C] = torch.from_numpy(xa).cuda()
        arena.view(b[0])[..., b[2]:b[2] + C] = torch.from_numpy(xb).cuda()
    plan = Plan(L, [_add_op(a[0], a[1], a[2], b[0], b[1], b[2], H, W, C, out[0], out[1], out[2])], arena)
    rc, kernel = plan.run()
    plan.close()
    if expect_rc:
        assert rc == expect_rc
        assert bool((arena.mem == SENTINEL).all()), "a refused add wrote something"
        return
    assert rc == 0 and kernel == "add"
    want = (torch.from_numpy(xa).float() + torch.from_numpy(xb).float()).half()
    got = arena.view(out[0])[..., out[2]:out[2] + C].cpu()
    assert bool((want == 0).any())                                                           # cancellation
    if want.numel() >= 2000:                                                                  # ... and in every case but the smallest: overflow and subnormal results
        assert bool(torch.isinf(want).any()) and bool(((want != 0) & (want.abs() < 6.0e-5)).any())
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "%d of %d values differ" % (int((got.view(torch.int16) != want.view(torch.int16)).sum()), want.numel())
    written = {}
    for buf, _, coff in (a, b, out):
        written.setdefault(buf, []).append((coff, coff + C))
    _assert_sentinel_outside(arena, written)


ADD_CASES = [
    # B, H, W, C, (a buffer, ld, coff), (b ...), (out ...)
    ("smallest legal", 1, 1, 1, 8, (0, 8, 0), (1, 8, 0), (2, 8, 0)),
    ("slices of wider buffers", 2, 5, 7, 40, (0, 72, 8), (1, 48, 8), (2, 56, 16)),
    ("both operands in one buffer", 2, 5, 7, 40, (0, 96, 8), (0, 96, 56), (1, 40, 0)),
    ("all three in one buffer", 2, 3, 5, 16, (0, 64, 0), (0, 64, 16), (0, 64, 40)),
    ("workload-like, grid-striding", 3, 20, 20, 1280, (0, 1280, 0), (1, 1280, 0), (2, 1280, 0)),      # e6e's coarsest Shortcut: 192 000 lanes of work, 750 workgroups
    ("more work than the grid", 2, 64, 64, 1280, (0, 1280, 0), (1, 1280, 0), (2, 2560, 1280)),       # 1.3 M lanes of work on 2048 workgroups of 256: every lane strides
]


@pytest.mark.parametrize("case", ADD_CASES, ids=[c[0] for c in ADD_CASES])
def test_add_kernel_is_bit_exact(L, case):
    name, B, H, W, C, a, b, out = case
    _run_add(L, B, H, W, C, a, b, out, seed=len(name))


REFUSALS = [
    ("C not a multiple of 8", 12, (0, 16, 0), (1, 16, 0), (2, 16, 0)),
    ("ld of A", 8, (0, 12, 0), (1, 16, 0), (2, 16, 0)),
    ("ld of B", 8, (0, 16, 0), (1, 20, 0), (2, 16, 0)),
    ("ld of the output", 8, (0, 16, 0), (1, 16, 0), (2, 28, 0)),
    ("coff of A", 8, (0, 16, 4), (1, 16, 0), (2, 16, 0)),
    ("coff of B", 8, (0, 16, 0), (1, 16, 4), (2, 16, 0)),
    ("coff of the output", 8, (0, 16, 0), (1, 16, 0), (2, 16, 4)),
    ("output on operand A", 16, (0, 32, 0), (1, 16, 0), (0, 32, 0)),
    ("output overlaps operand A", 16, (0, 32, 0), (1, 16, 0), (0, 32, 8)),
    ("output overlaps operand B", 16, (1, 16, 0), (0, 32, 16), (0, 32, 8)),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_add_refusals_write_nothing(L, case):
    name, C, a, b, out = case
    _run_add(L, 2, 3, 5, C, a, b, out, seed=1, expect_rc=E_ARG)


def test_det_create_range_checks_the_second_operand(L):
    from tests.test_membound_gpu import Arena
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.detector import graph
    arena = Arena([(2, 2, 8)] * 3, 1)
    offs = np.array(arena.offsets, dtype=np.int64)
    for bad in (3, -1):
        ops = np.array([_add_op(0, 8, 0, bad, 8, 0, 2, 2, 8, 2, 8, 0)], dtype=graph.OP_DTYPE)
        h = ctypes.c_void_p()
        rc = L.y7t_det_create(ops.ctypes.data_as(ctypes.c_void_p), 1, offs.ctypes.data_as(ctypes.c_void_p), 3, _lib.ptr(arena.mem), arena.mem.numel() * 2,
                              _lib.ptr(arena.dummy_w), _lib.ptr(arena.dummy_b), 1, ctypes.byref(h))
        assert rc == E_ARG and not h.value


# ------------------------------------------------------------------------------------------------ b. / c. the five graphs
_dets = {}


def _detector(name, tag="default"):
    """the seeded, conditioned network of the goldens (tests/family_ref.py::seeded(name)) on the device after one forward of the golden images"""
    from yolov7_tracker_amd.detector import model
    if (name, tag) not in _dets:
        spec, nodes, plan, sd = fr.seeded(name)
        det = model.Detector(spec, sd, img_size=fr.small_hw(name), max_batch=2)
        img = fr.golden_image(name)
        out = det(img)[0]
        torch.cuda.synchronize()
        _dets[(name, tag)] = (det, img, out)
    return _dets[(name, tag)]


def _teacher_forced(name, tag="default"):
    det, img, out = _detector(name, tag)
    names = det.launch_list(2)
    det(img)                                                     # launch_list re-ran the ops one by one: the same values; one clean forward again
    torch.cuda.synchronize()
    x = img.half().float()
    x0 = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1) if det.plan.reorg else x
    st = family_teacher.check_every_op(det, 2, [0, 1], x0, names)
    print("FAMILY %s (%s): %d ops, worst err / tol per kernel %s" % (name, tag, len(names), {k: round(v, 3) for k, v in sorted(st["worst"].items())}))
    # the census of tests/test_family_cpu.py, on the launch list
    assert names.count("add") == st["n_add"] == (11 if name == "yolov7-e6e" else 0)
    assert st["n_rep"] == (3 if name == "yolov7" else 0) and st["n_copy"] == 0
    pools22 = sum(1 for n, op in zip(names, det.plan.ops) if int(op["type"]) == 2 and n == "maxpool<2,2>")
    assert pools22 == (8 if name in fr.P6 else 5)
    assert st["n_conv"] + st["n_add"] + st["n_pool"] + st["n_up"] == len(names) == len(det.plan.ops)
    return st


@pytest.mark.parametrize("name", fr.FAMILY)
def test_every_op_teacher_forced(name):
    st = _teacher_forced(name)
    assert st["n_up_on_read"] > 0 and st["n_up"] == 0            # default lowering: the upsamples are read through, never materialised


def test_every_op_teacher_forced_e6e_with_materialised_upsamples(monkeypatch):
    monkeypatch.setenv("Y7T_UPSAMPLE_ON_READ", "0")
    st = _teacher_forced("yolov7-e6e", "materialised")
    assert st["n_up"] == 3 and st["n_up_on_read"] == 0


_walk16 = {}


@pytest.mark.parametrize("name", fr.FAMILY)
def test_whole_network_heads_against_the_reference_golden(name):
    """device raw heads vs the fp32 reference's (golden): mean and max deviation per level at most 3 x what the CPU walk at the device's storage precision
    (fp16 = True) deviates from the SAME golden -- the yardstick is the reference, never the device"""
    g = np.load(os.path.join(util.GOLDEN, "family_%s.npz" % name))
    spec, nodes, plan, sd = fr.seeded(name)
    assert fr.state_digest(sd) == str(g["state_digest"]), "the seeded state dict of %s is not the one the golden was recorded with" % name
    det, img, out = _detector(name)
    det(img)
    torch.cuda.synchronize()
    raw = [r.cpu() for r in out.raw()]
    _, walk = fr.forward(nodes, sd, img, spec["anchors"], fp16=True)
    for l, (d, w) in enumerate(zip(raw, walk)):
        ref = torch.from_numpy(g["raw%d" % l])
        dev_mean, dev_max = float((d - ref).abs().mean()), float((d - ref).abs().max())
        cpu_mean, cpu_max = float((w - ref).abs().mean()), float((w - ref).abs().max())
        print("FAMILY %s level %d (logit std %.3f): device mean %.3e max %.3e | fp16 walk mean %.3e max %.3e" % (name, l, float(ref.std()), dev_mean, dev_max, cpu_mean, cpu_max))
        assert dev_mean <= 3 * cpu_mean and dev_max <= 3 * cpu_max


# ------------------------------------------------------------------------------------------------ d. the convolution shapes the graphs bring
def new_conv_cases():
    """every distinct (korder, Cin, Cout, k, stride) of the five plans at their nominal size (max_batch 8) that no case list of tests/test_detector_gpu.py runs,
    as a case of that file's test: the smallest map the kernel family of that weight order takes, batch 1, sliced into wider buffers where the plan slices"""
    from tests import test_detector_gpu as tdg
    from yolov7_tracker_amd.detector import arch, graph
    from yolov7_tracker_amd.detector.layout import WeightLayout as WL, act_bits
    have = set()
    for attr in dir(tdg):
        if attr.endswith("_CASES"):
            for c in getattr(tdg, attr):
                if isinstance(c, tuple) and len(c) == 13:
                    have.add((layout_of(c[7])[0], c[3], c[4], c[5], c[6]))
    cases, seen = [], set()
    for name in fr.FAMILY:
        hw = fr.nominal_hw(name)
        p = graph.lower(graph.parse(arch.ARCHS[name](80))[0], hw[0], hw[1], 8)
        for op in p.ops:
            o = {k: int(op[k]) for k in op.dtype.names}
            key = (o["korder"], o["Cin"], o["Cout"], o["KH"], o["stride"])
            if o["type"] != 0 or o["korder"] == WL.WS_S2_TWIN or key in have or key in seen:      # (WS_S2_TWIN, the fused stride-2 + twin op, is w6's: tests/test_detector_pinned_gpu.py)
                continue
            seen.add(key)
            H, W = {WL.TAP_MAJOR: (12, 20), WL.LINE_MAJOR: (12, 20), WL.PANEL_1X1: (12, 20), WL.PANEL_1X1_N64: (12, 20), WL.P8: (16, 16)}.get(o["korder"], (16, 64))
            act = o["act"] | act_bits(o["korder"])
            cases.append((1, H, W, o["Cin"], o["Cout"], o["KH"], o["stride"], act, o["in_ld"], o["in_coff"], o["out_ld"], o["out_coff"], o["out_f32"]))
    return cases


NEW_CONV_CASES = new_conv_cases()


@pytest.mark.parametrize("case", NEW_CONV_CASES, ids=["k%d-%dto%d-%dx%ds%d" % (layout_of(c[7])[0], c[3], c[4], c[5], c[5], c[6]) for c in NEW_CONV_CASES])
def test_new_conv_shapes_match_torch_fp32(L, case):
    from tests.test_detector_gpu import test_conv_layer_matches_torch_fp32
    test_conv_layer_matches_torch_fp32(L, case, util.conv_dispatch_name(case))      # (the cases come out of the plans: the name from the dispatch rule restated in tests/util.py)


def test_new_conv_shapes_cover_the_named_ones():
    keys = {(c[3], c[4], c[5], c[6]) for c in NEW_CONV_CASES}
    for k in ((8, 40, 3, 1), (40, 80, 3, 2), (80, 80, 3, 1), (160, 320, 3, 1), (320, 255, 1, 1), (16, 80, 3, 1), (16, 96, 3, 1)):
        assert k in keys, k


# ------------------------------------------------------------------------------------------------ e. the CLI
@pytest.mark.parametrize("model,size,frames", [("random:yolov7", 640, 6), ("random:yolov7-e6e", 256, 6)])
def test_track_cli_runs_the_new_graphs(tmp_path, model, size, frames):
    from tests.test_cli_gpu import oracle_file
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    folder = track.cli(["--dataset", "synthetic", "--tracker", "bytetrack", "--model_path", model, "--nc", "10", "--img_size", str(size), "--synthetic_dets",
                        "--synthetic_frames", str(frames), "--synthetic_objs", "20", "--results_root", str(tmp_path)])
    got = open(os.path.join(folder, "synthetic-000.txt")).read().splitlines()
    want = oracle_file("bytetrack", frames, 20, size).splitlines()
    assert len(got) > 0 and [l.split(",")[:2] for l in got] == [l.split(",")[:2] for l in want]      # every frame's rows: frame number and id
    assert max(int(l.split(",")[0]) for l in got) == frames
