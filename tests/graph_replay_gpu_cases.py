"""GPU, in a child process (tests/test_graph_replay_gpu.py): launch lists captured into a hipGraph and REPLAYED -- the path bench.py's latency mode, --hipgraph 1 and
--hipgraph 2 time -- against eager runs of the same entry points.  DESIGN.md section 2 "What a replayed launch list relies on" names the state; every item has a case here.

Rules of every case
  * poison before every replay: whatever the replay has to write holds a value it cannot produce (one-op plans: NaN in the output slice; whole networks: NaN in dets,
    -1 in ndets / cand / keep, 2^30 in the candidate counters -- a counter that is not zeroed then drops every candidate instead of indexing with it).  The poison is
    enqueued on the stream the replay runs on.  A replay that launches nothing, or without the node that zeroes the counters, fails;
  * a fresh input before every replay, written into the fixed device buffer the graph reads: at least 4 replays over at least 3 distinct inputs, the last one the first
    again -- state that only goes wrong after k replays shows on the way, and the last replay is held against the first;
  * the reference is an EAGER run of the same entry points on the same input, and the comparison is bit equality: the kernels are the same, and
    tests/test_conv_forms_gpu.py asserts run-to-run bit identity for each of them.  Whole networks: a second Detector built from the same state dict (no plan, counter,
    slab or workspace shared with the graph), compared as tests/test_detector_gpu.py::test_staged_heads_give_identical_detections compares (row counts, and the rows
    up to the count, bit for bit) plus the candidate counts.  Candidate ARRAYS are filled in order of arrival: compared as sets keyed by cidx, as the conv-forms file does;
  * one-op plans: the first and the last replay also against float64 at the bar of tests/conv_ref.py (Case.check_values: no new number), one MARGIN line each
    (profiles/graph_replay_margins.txt keeps one run's listing); after the last replay the arena write check of Case.run and the op's tile counters == 0;
  * the capture is one stream, linear, with nothing that synchronises inside: y7t_det_forward_ops / y7t_det_forward_fused are enqueued directly after one eager warm-up,
    y7t_last_kernel() is read after the warm-up; the graph object is deleted before its plan is closed.

The shapes are the smallest of tests/test_conv_forms_gpu.py for each form (its constructors are imported, not copied); the networks 128 x 192 (tiny) and 64 x 64 (w6)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import post_scenes
from tests.test_conv_forms_gpu import (DYN_FORMS, DYN_WHICH, WS_FILL, Case, DetectPlan, _assert_untouched_behind, _by_cidx, _span, bits, conv_op, dyn_case, p8_plan_case,
                                       poison_reads, ws_s2_case)
from tests.test_membound_gpu import Arena, Plan, _spp_check, _spp_plan, plane_distinct_fp16
from tests.util import pack_w
from yolov7_tracker_amd.detector.layout import WeightLayout as WL

pytestmark = pytest.mark.gpu

CONF, IOU = 0.01, 0.45
COUNT_POISON = 1 << 30          # a candidate counter that is not zeroed: every slot it hands out is >= cap, so nothing is stored and the count cannot match


@pytest.fixture(scope="module")
def L():
    from yolov7_tracker_amd import _lib
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def stop_after_a_device_error():
    """a case that left the device in an error state ends the child: nothing more is started on a device that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error after a case, no further case is started: %s" % e, returncode=3)


# ------------------------------------------------------------------------------------------------ harness
def capture(enqueue):
    """one eager warm-up has run; -> the graph of `enqueue()` (return codes of liby7t calls), captured on torch's capture stream alone"""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rcs = enqueue()
    assert all(rc == 0 for rc in rcs), rcs
    return g


def tile_counters(L, h, op):
    from yolov7_tracker_amd import _lib
    ctr = (ctypes.c_int * 8)()
    _lib.check(L.y7t_det_tile_counters(h, op, ctr))
    return list(ctr)


def replay_sequence(n_distinct=3):
    """input index of every replay: all distinct inputs, then the first again"""
    return list(range(n_distinct)) + [0]


def replay_one_op(c, kernel, rows=None):
    """A. the one-op plan of Case `c` captured and replayed over three inputs (the Case's own and two more from its generator)"""
    from yolov7_tracker_amd import _lib
    L = c.L
    assert not c.up, "the replay harness writes the input slice only"
    xs = [torch.from_numpy(c.x).cuda()] + [torch.from_numpy(c.rng.normal(0, 1, c.x.shape).astype(np.float16)).cuda() for _ in range(2)]
    in_slice = c.arena.view(1)[..., c.in_coff:c.in_coff + c.Cin]
    snap = c.arena.mem.clone()
    plan = Plan(L, [c.op], c.arena)
    g = None
    try:
        eager = []
        for x in xs:                                                                    # the eager runs: the reference, and the warm-up of the capture
            in_slice.copy_(x)
            c.out_slice().fill_(float("nan"))
            rc, name = plan.run()
            assert rc == 0, (rc, L.y7t_last_error())
            assert name == kernel, "%s ran %r, the dispatch code says %r" % (c.label, name, kernel)
            eager.append(c.out_slice().clone())
            assert not bool(torch.isnan(eager[-1]).any()), c.label
        assert not torch.equal(bits(eager[0]), bits(eager[1])) and not torch.equal(bits(eager[1]), bits(eager[2]))
        g = capture(lambda: [L.y7t_det_forward_ops(plan.h, c.B, 0, -1, _lib.stream_ptr())])
        seq = replay_sequence()
        for r, i in enumerate(seq):
            in_slice.copy_(xs[i])
            c.out_slice().fill_(float("nan"))                                           # same stream as the replay
            g.replay()
            torch.cuda.synchronize()
            out = c.out_slice().clone()
            assert torch.equal(bits(out), bits(eager[i])), "%s: replay %d (input %d) differs from the eager run in %d values, %d of them still poison" % (
                c.label, r, i, int((bits(out) != bits(eager[i])).sum()), int(torch.isnan(out).sum()))
            if r in (0, len(seq) - 1):
                c.check_values(out, kernel, rows, "   replay %d of %d == eager" % (r + 1, len(seq)))
        c.assert_only_the_output_slice_changed(snap)
        ctr = tile_counters(L, plan.h, 0)
        assert ctr == [0] * 8, "%s: tile counters after the last replay: %s" % (c.label, ctr)
    finally:
        del g
        plan.close()


# ------------------------------------------------------------------------------------------------ A. tile-counter forms
@pytest.mark.parametrize("which", DYN_WHICH)
@pytest.mark.parametrize("kernel", sorted(DYN_FORMS))
def test_tile_counter_forms_replayed(L, ncu, kernel, which):
    korder, s, Cin, Cout, TH, TW, n_nt, act_of = DYN_FORMS[kernel]
    c, rows = dyn_case(L, ncu, which, korder, s, Cin, Cout, TH, TW, n_nt, act_of(DYN_WHICH.index(which)))
    replay_one_op(c, kernel, rows)


@pytest.mark.parametrize("Cout", [256, 768], ids=["one channel tile", "three channel tiles"])
def test_p8_persistent_form_replayed(L, ncu, Cout):
    c, rows = p8_plan_case(L, ncu, 128, Cout, "persistent")                            # (asserts the launcher's rule for the persistent form)
    replay_one_op(c, "p8<256,256,64> 1x1", rows)


@pytest.mark.parametrize("twin", [False, True], ids=["ws_s2", "ws_s2 + 1x1"])
@pytest.mark.parametrize("which", ["one tile", "more tiles than workgroups"])
def test_ws_s2_replayed(L, ncu, which, twin):
    c, rows = ws_s2_case(L, ncu, which, twin)
    replay_one_op(c, "ws_s2<2,32> + 1x1" if twin else "ws_s2<2,32>", rows)


# ------------------------------------------------------------------------------------------------ A. split-K
SPLITK_CASES = [
    # the two split-K cases of tests/test_conv_forms_gpu.py::IGEMM_CASES with fp16 and fp32 outputs, and its LINE_MAJOR one
    ("split-K, fp16 out Cout 46 ld 48", "igemm<128,64,32,2> 1x1 splitK", (2, 10, 14, 512, 46, 1, 1, 2, WL.TAP_MAJOR, 512, 0, 48, 0, 0)),
    ("split-K, fp32 out Cout 45", "igemm<128,64,32,2> 1x1 splitK", (2, 10, 14, 256, 45, 1, 1, 0, WL.TAP_MAJOR, 256, 0, 45, 0, 1)),
    ("split-K, LINE_MAJOR s2 Cin 192, splits start inside a group", "igemm<128,64,64,2> splitK", (1, 33, 31, 192, 64, 3, 2, 1, WL.LINE_MAJOR, 256, 64, 64, 0, 0)),
]


@pytest.mark.parametrize("label,kernel,case", SPLITK_CASES, ids=[c[0] for c in SPLITK_CASES])
def test_split_k_replayed(L, label, kernel, case):
    B, H, W, Cin, Cout, k, s, act, korder, in_ld, in_coff, out_ld, out_coff, out_f32 = case
    replay_one_op(Case(L, "%s %s" % (label, case[:8]), B, H, W, Cin, Cout, k, s, act, korder, in_ld, in_coff, out_ld, out_coff, out_f32), kernel)


def test_two_split_k_ops_share_the_slab_in_one_graph(L):
    """op 0: 1x1 512 -> 64 on 2 x 10 x 14 (3 tiles, 16 K-steps: 4 splits); op 1: 3x3 / 2 64 -> 64 on op 0's output (1 tile, 9 K-steps: 2 splits).  Both write their partial
    sums into the plan's ONE slab, and op 1 reads what op 0's reduce stored -- in a graph as in a stream the order of the four launches is all that keeps them apart.
    float64: op 0's output at its bar; op 1 teacher-forced on the device's own fp16 tensor between the ops, at its bar."""
    from yolov7_tracker_amd import _lib
    B, H, W, C0, C1 = 2, 10, 14, 512, 64
    rng = np.random.default_rng(77)
    arena = Arena([(8, 8, 64), (H, W, C0), (H, W, C1), (H // 2, W // 2, C1), (8, 8, 64)], B)
    poison_reads(arena, [1])
    W0, b0 = (rng.normal(0, 1, (C1, C0, 1, 1)) / np.sqrt(C0)).astype(np.float16), rng.normal(0, 0.5, C1).astype(np.float32)
    W1, b1 = (rng.normal(0, 1, (C1, C1, 3, 3)) / np.sqrt(9 * C1)).astype(np.float16), rng.normal(0, 0.5, C1).astype(np.float32)
    arena.dummy_w = torch.from_numpy(np.concatenate([pack_w(W0.astype(np.float32), C0, 64, WL.TAP_MAJOR).ravel(), pack_w(W1.astype(np.float32), C1, 64, WL.TAP_MAJOR).ravel()])).cuda()
    arena.dummy_b = torch.from_numpy(np.concatenate([b0, b1])).cuda()
    ops = [conv_op(1, C0, 0, H, W, C0, 2, C1, 0, 0, C1, 64, 1, 1, 1, WL.TAP_MAJOR), conv_op(2, C1, 0, H, W, C1, 3, C1, 0, 0, C1, 64, 3, 2, 2, WL.TAP_MAJOR, w_off=64 * C0, bias_off=64)]
    xs = [rng.normal(0, 1, (B, H, W, C0)).astype(np.float16) for _ in range(3)]
    plan = Plan(L, ops, arena)
    g = None

    def poison():
        arena.view(2).fill_(float("nan"))
        arena.view(3).fill_(float("nan"))

    try:
        arena.view(1).copy_(torch.from_numpy(xs[0]).cuda())
        names = []
        for i in range(2):                                                              # the names, op by op
            rc, name = plan.run(i, i + 1)
            assert rc == 0, (rc, L.y7t_last_error())
            names.append(name)
        assert names == ["igemm<128,64,32,2> 1x1 splitK", "igemm<128,64,64,2> splitK"], names
        snap = arena.mem.clone()
        eager = []
        for x in xs:
            arena.view(1).copy_(torch.from_numpy(x).cuda())
            poison()
            rc, _ = plan.run()
            assert rc == 0, (rc, L.y7t_last_error())
            eager.append((arena.view(2).clone(), arena.view(3).clone()))
        g = capture(lambda: [L.y7t_det_forward_ops(plan.h, B, 0, -1, _lib.stream_ptr())])
        seq = replay_sequence()
        for r, i in enumerate(seq):
            arena.view(1).copy_(torch.from_numpy(xs[i]).cuda())
            poison()
            g.replay()
            torch.cuda.synchronize()
            mid, out = arena.view(2).clone(), arena.view(3).clone()
            assert torch.equal(bits(mid), bits(eager[i][0])) and torch.equal(bits(out), bits(eager[i][1])), "replay %d (input %d) differs from the eager run" % (r, i)
            if r in (0, len(seq) - 1):
                ref0, ab0 = cr.conv_ref(xs[i], W0, b0, 1, 1, 1)
                ref1, ab1 = cr.conv_ref(mid.cpu().numpy(), W1, b1, 3, 2, 2)
                r0 = cr.worst_ratio(mid.double().cpu().numpy().reshape(-1, C1), ref0, cr.tolerance(ref0, ab0, C0))
                r1 = cr.worst_ratio(out.double().cpu().numpy().reshape(-1, C1), ref1, cr.tolerance(ref1, ab1, 9 * C1))
                print("\nMARGIN %-44s %-86s %.3f / %.3f   replay %d of %d == eager" % (" + ".join(names), "two split-K ops on one slab, B 2 10x14 512 -> 64 -> 64 /2", r0, r1, r + 1, len(seq)))
                assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)
        after = arena.mem.clone()                                                       # nothing but the two output buffers has changed
        for i in (2, 3):
            a, b = _span(arena, i)
            after[a:b] = snap[a:b]
        assert int((bits(after) != bits(snap)).sum()) == 0
        assert tile_counters(L, plan.h, 0) == [0] * 8 and tile_counters(L, plan.h, 1) == [0] * 8
    finally:
        del g
        plan.close()


# ------------------------------------------------------------------------------------------------ A. the fused Detect epilogue
def _count_words(ws, B, cap, max_nms=30000):
    o, nbytes = post_scenes.ws_layout(B, cap, max_nms)["count"]
    return ws[o:o + nbytes].view(torch.int32)


def replay_fused_detect(dp, kernel, label, conf, cap, shifts, up_then_down):
    """y7t_det_forward_fused of a DetectPlan replayed.  shifts: input channel 0 (weight 1 into every objectness logit) of the non-empty images per distinct input: the
    candidate COUNT moves with it.  Every replay: counts and candidate rows (by cidx) == the eager run's, nothing written behind the count, the arena untouched."""
    from yolov7_tracker_amd import _lib
    L, max_nms = dp.L, 30000
    nonempty = [b for b in range(dp.B) if dp.x[0][b, 0, 0, 0] == 0]
    base = [torch.from_numpy(x).cuda() for x in dp.x]

    def write_input(shift):
        for l, xb in enumerate(base):
            x = xb.clone()
            x[nonempty, ..., 0] = shift
            dp.arena.view(1 + 2 * l).copy_(x)

    g = None
    try:
        eager = []
        for sft in shifts:                                                              # DetectPlan.fused: a fresh workspace, the kernel's name, the arena untouched
            write_input(sft)
            eager.append(dp.fused(conf, cap, kernel))
        totals = [int(e[4].sum()) for e in eager]
        assert max(int(e[4].max()) for e in eager) <= cap and min(totals) > 0, totals
        assert (totals[0] < totals[1] and totals[2] < totals[1]) if up_then_down else len(set(totals)) == 3, totals
        ws = dp._ws(cap, max_nms)
        g = capture(lambda: [L.y7t_det_forward_fused(dp.plan.h, dp.B, 0, -1, float(conf), cap, max_nms, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())])
        seq = replay_sequence()
        for r, i in enumerate(seq):
            write_input(shifts[i])
            snap = dp.arena.mem.clone()
            ws.fill_(WS_FILL)
            _count_words(ws, dp.B, cap).fill_(COUNT_POISON)
            g.replay()
            torch.cuda.synchronize()
            got, want = post_scenes.unpack_candidates(ws.cpu().numpy(), dp.B, cap, max_nms), eager[i]
            assert np.array_equal(got[4], want[4]), "%s: replay %d (input %d): counts %s, eager %s" % (label, r, i, got[4], want[4])
            for b in range(dp.B):
                n = int(want[4][b])
                assert _by_cidx(got, b, n) == _by_cidx(want, b, n), "%s: replay %d: image %d: candidate rows differ from the eager run" % (label, r, b)
                _assert_untouched_behind(got, b, n, label)
            assert torch.equal(bits(dp.arena.mem), bits(snap)), "the replayed fused forward wrote into the arena"
        for l in range(len(dp.levels)):
            assert tile_counters(L, dp.plan.h, l) == [0] * 8
        print("\nMARGIN %-44s %-86s %d replays == eager, candidates per input %s" % (kernel, label, len(seq), totals))
    finally:
        del g


def test_fused_detect_epilogue_replayed(L):
    """the candidate count goes up and then down between replays: a counter that is not zeroed again shows in both directions"""
    label = "5x5 B7 no 15: six images in one tile, image 3 empty"
    dp = DetectPlan(L, 7, [(5, 5, 8)], 192, 15, WL.TAP_MAJOR, 1.0, (3,), seed=len(label))
    try:
        replay_fused_detect(dp, "igemm<128,64,32,4> 1x1 detect-decode", label, 0.25, 128, [0.0, 2.0, -2.0], up_then_down=True)
    finally:
        dp.close()


def test_fused_detect_two_stage_instance_replayed(L):
    """the instance of test_fused_detect_epilogue_two_stage_instance (more than 4096 pixel tiles keep the two-stage ring).  Its cap of 2048 holds the candidates of the
    case's own input; the other two inputs lower the objectness, so no image passes the cap (above it the subset kept depends on the order of arrival): down, up, up"""
    dp = DetectPlan(L, 21, [(160, 160, 8)], 64, 6, WL.PANEL_1X1, -3.5, (9,), seed=21)
    try:
        replay_fused_detect(dp, "igemm<128,64,32,2> 1x1 detect-decode", "160x160 B21 Cin 64 no 6, image 9 empty", 0.25, 2048, [0.0, -1.0, -0.5], up_then_down=False)
    finally:
        dp.close()


# ------------------------------------------------------------------------------------------------ A. controls: nothing that can go wrong between replays
def test_control_stateless_igemm_replayed(L):
    case = (2, 128, 128, 64, 512, 3, 2, 1, WL.TAP_MAJOR, 64, 0, 512, 0, 0)
    B, H, W, Cin, Cout, k, s, act, korder, in_ld, in_coff, out_ld, out_coff, out_f32 = case
    replay_one_op(Case(L, "control: uniform taps, no split-K, TAP_MAJOR %s" % (case[:8],), B, H, W, Cin, Cout, k, s, act, korder, in_ld, in_coff, out_ld, out_coff, out_f32),
                  "igemm<128,128,64,2>")


def test_control_spp3_pool_chain_replayed(L):
    """the fused SPP cascade (three pools, one launch): the reference of tests/test_membound_gpu.py (torch max-pools of the same fp16 values, exact)"""
    from yolov7_tracker_amd import _lib
    shape, C = (2, 20, 20, 32), 32
    arena, plan, x0 = _spp_plan(L, shape, 0, C, 4 * C + 8)
    xs = [x0] + [torch.from_numpy(plane_distinct_fp16(np.random.default_rng(500 + i), *shape)).cuda() for i in range(2)]
    g = None
    try:
        rc, name = plan.run(0, 3)
        assert rc == 0 and name == "spp3<5,5,5> lds", (rc, name)
        g = capture(lambda: [L.y7t_det_forward_ops(plan.h, shape[0], 0, 3, _lib.stream_ptr())])
        for i in replay_sequence():
            arena.view(0)[..., 0:C] = xs[i]
            arena.view(0)[..., C:4 * C] = float("nan")
            g.replay()
            torch.cuda.synchronize()
            _spp_check(arena, xs[i], shape, 0, C)
        print("\nMARGIN %-44s %-86s exact, 4 replays" % ("spp3<5,5,5> lds", "control: %s" % (shape,)))
    finally:
        del g
        plan.close()


# ------------------------------------------------------------------------------------------------ B. whole networks through Detector.capture
_NETS = {}


def net_pair(name, hw, max_batch, u8):
    """(det, ref, frames): two Detectors from ONE state dict (seeded weights, planted objectness bias) that share nothing on the device, and four frames of the plan's
    size -- seeded noise, then the synthetic scene of synth.py -- as float32 CHW RGB in [0, 1] or uint8 HWC BGR device tensors.  Built once per configuration."""
    key = (name, hw, max_batch, u8)
    if key not in _NETS:
        from yolov7_tracker_amd import synth
        from yolov7_tracker_amd.detector import arch, model
        H, W = hw
        rng = np.random.default_rng(H * 1000 + W)
        scene = synth.make_frames(3, 12, max(H, W), seq_idx=4)[:, :H, :W]
        host = np.concatenate([rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8), scene])
        frames = torch.from_numpy(host).cuda()
        if not u8:
            frames = (frames.flip(-1).permute(0, 3, 1, 2).float() / 255.0).contiguous()
        det = model.Detector(arch.ARCHS[name](10), None, img_size=hw, max_batch=max_batch, seed=3)
        n_anchors = sum(det.plan.det["na"] * h["ny"] * h["nx"] for h in det.plan.heads)
        det.plant_objectness_bias(frames[:1], target=min(300, n_anchors // 2))
        ref = model.Detector(det.spec, det._sd, img_size=hw, max_batch=max_batch)
        assert det.plan.fusable and ref.plan.fusable
        _NETS[key] = (det, ref, frames)
    return _NETS[key]


def eager_reference(ref, img, ori_shapes=None):
    out = ref.forward(img, fuse_decode=CONF)
    d, n = ref.postprocess(out, CONF, IOU, ori_shapes)
    torch.cuda.synchronize()
    B = img.shape[0]
    assert int(n[:B].sum()) > 0, "an empty reference: 'equal' would mean 'both empty'"
    return d[:B].clone(), n[:B].clone(), ref.plan.post[0].cand[:B].clone(), ref.candidate_arrays(0, B)[4].clone()


def poison_outputs(det, B, pset=0):
    ps = det.plan.post[pset]
    ps.dets.fill_(float("nan"))
    ps.ndets.fill_(-1)
    ps.cand.fill_(-1)
    ps.keep.fill_(-1)
    det.candidate_arrays(pset, B)[4].fill_(COUNT_POISON)


def assert_equal_to_reference(det, B, want, what, dets=None, ndets=None, pset=0):
    """row counts, the rows up to the count bit for bit (test_staged_heads_give_identical_detections), candidate counts; the kept slots are real slots"""
    ps = det.plan.post[pset]
    d, n = (ps.dets, ps.ndets) if dets is None else (dets, ndets)
    wd, wn, wcand, wcount = want
    assert torch.equal(n[:B], wn), "%s: ndets %s, eager reference %s" % (what, n[:B].tolist(), wn.tolist())
    assert torch.equal(ps.cand[:B], wcand) and torch.equal(det.candidate_arrays(pset, B)[4], wcount), "%s: candidate counts %s / %s, eager reference %s" % (
        what, ps.cand[:B].tolist(), det.candidate_arrays(pset, B)[4].tolist(), wcount.tolist())
    for b in range(B):
        k = int(wn[b])
        assert torch.equal(d[b, :k].view(torch.int32), wd[b, :k].view(torch.int32)), "%s: image %d: %d of %d detection values differ from the eager reference" % (
            what, b, int((d[b, :k].view(torch.int32) != wd[b, :k].view(torch.int32)).sum()), 6 * k)
        assert bool(((ps.keep[b, :k] >= 0) & (ps.keep[b, :k] < wcount[b])).all()), "%s: image %d: keep holds a slot that is no candidate" % (what, b)


def replay_network(det, ref, batches, what, ori_shapes=None):
    """Detector.capture on a fixed input buffer, replayed over `batches` (a list of input tensors: >= 3 distinct, then the first again)"""
    B = batches[0].shape[0]
    wants = [eager_reference(ref, x, ori_shapes) for x in batches[:-1]]
    wants.append(wants[0])
    dev_in = batches[0].clone()
    g, g_dets, g_nd = det.capture(dev_in, CONF, IOU, ori_shapes)
    try:
        for r, x in enumerate(batches):
            dev_in.copy_(x)
            poison_outputs(det, B)
            g.replay()
            torch.cuda.synchronize()
            assert_equal_to_reference(det, B, wants[r], "%s: replay %d" % (what, r), g_dets, g_nd)
        print("\nNET %-60s %d replays == eager reference; detections per replay %s, candidates %s" % (what, len(batches), [int(w[1].sum()) for w in wants], [int(w[3].sum()) for w in wants]))
    finally:
        del g


def test_tiny_batch_1_capture_replays_equal_eager():
    """yolov7-tiny (nc 10: 45 head channels, the fused Detect epilogues) at 128 x 192, float32 CHW input, max_batch 1: the batch-1 launch list holds split-K forms"""
    det, ref, f = net_pair("yolov7-tiny", (128, 192), 1, False)
    det.forward(f[:1])
    names = det.launch_list(1)
    print("\nlaunch list, tiny 128 x 192 batch 1:", names)
    assert any("splitK" in n for n in names), names
    replay_network(det, ref, [f[0:1], f[1:2], f[2:3], f[0:1]], "tiny 128x192 B1 of max_batch 1")


def test_tiny_batch_2_capture_replays_equal_eager():
    det, ref, f = net_pair("yolov7-tiny", (128, 192), 2, False)
    det.forward(f[:2])
    names = det.launch_list(2)
    print("\nlaunch list, tiny 128 x 192 batch 2:", names)
    assert any("splitK" in n for n in names), names
    replay_network(det, ref, [f[0:2], f[1:3], f[2:4], f[0:2]], "tiny 128x192 B2 of max_batch 2")


def test_tiny_batch_1_capture_on_a_max_batch_2_detector():
    """the workspace arrays are laid out for the batch of the capture (y7t_post_ws), not for max_batch"""
    det, ref, f = net_pair("yolov7-tiny", (128, 192), 2, False)
    replay_network(det, ref, [f[3:4], f[1:2], f[0:1], f[3:4]], "tiny 128x192 B1 of max_batch 2")


def test_w6_uint8_fused_stem_capture_replays_equal_eager():
    """yolov7-w6 (nc 10) on uint8 HWC frames at 64 x 64 -- the smallest size the stride-64 head allows, and a multiple of 32, so the fused frame -> stem kernel takes the
    frames: the counters are zeroed from Detector._front with an empty op range, and that launch must be a node of the graph"""
    det, ref, f = net_pair("yolov7-w6", (64, 64), 1, True)
    assert det.plan.stem_fused and ref.plan.stem_fused and f.dtype == torch.uint8
    replay_network(det, ref, [f[0:1], f[1:2], f[2:3], f[0:1]], "w6 64x64 uint8 B1, fused stem")


def test_eager_work_between_replays():
    """replay; an eager forward + post-process of another frame on the SAME plan with pset 1; replay the first frame; an eager run with pset 0 (it rewrites the dets,
    ndets and workspace the graph writes); replays.  Every replay equals the independent eager reference, and so does every eager run."""
    det, ref, f = net_pair("yolov7-tiny", (128, 192), 1, False)
    want = [eager_reference(ref, f[i:i + 1]) for i in range(3)]
    dev_in = f[0:1].clone()
    g, g_dets, g_nd = det.capture(dev_in, CONF, IOU, None)

    def replay(i, what):
        dev_in.copy_(f[i:i + 1])
        poison_outputs(det, 1)
        g.replay()
        torch.cuda.synchronize()
        assert_equal_to_reference(det, 1, want[i], what, g_dets, g_nd)

    def eager(i, pset, what):
        poison_outputs(det, 1, pset)
        out = det.forward(f[i:i + 1], fuse_decode=CONF, pset=pset)
        d, n = det.postprocess(out, CONF, IOU, None)
        torch.cuda.synchronize()
        assert_equal_to_reference(det, 1, want[i], what, d, n, pset)

    try:
        replay(0, "replay 0")
        eager(1, 1, "eager, pset 1")
        replay(0, "replay 1, after an eager run with pset 1")
        eager(2, 0, "eager, pset 0")
        replay(1, "replay 2, after an eager run with pset 0")
        replay(2, "replay 3")
        replay(0, "replay 4")
        print("\nNET %-60s 5 replays and 2 eager runs == eager reference" % "tiny 128x192 B1, eager work between replays")
    finally:
        del g


def test_a_captured_graph_owns_its_letterbox():
    """capture with ori_shapes = [(100, 170)] (gain 1.129, a pad on top and bottom); an eager post-process with other ori_shapes on the same plan uploads another letterbox
    into the plan's shared tensor; the next replay still rescales with the capture-time letterbox (Detector.capture's docstring: which tensors a graph owns)"""
    det, ref, f = net_pair("yolov7-tiny", (128, 192), 1, False)
    ori, other = [(100, 170)], [(64, 96)]
    want = [eager_reference(ref, f[i:i + 1], ori) for i in range(3)]
    want_other = eager_reference(ref, f[1:2], other)
    assert not torch.equal(want[1][0], want_other[0])
    dev_in = f[0:1].clone()
    g, g_dets, g_nd = det.capture(dev_in, CONF, IOU, ori)
    try:
        for r, i in enumerate([0, 1, 2, 0]):
            if r == 1:
                out = det.forward(f[1:2], fuse_decode=CONF, pset=1)
                d, n = det.postprocess(out, CONF, IOU, other)
                torch.cuda.synchronize()
                assert_equal_to_reference(det, 1, want_other, "eager, other ori_shapes", d, n, 1)
            dev_in.copy_(f[i:i + 1])
            poison_outputs(det, 1)
            g.replay()
            torch.cuda.synchronize()
            assert_equal_to_reference(det, 1, want[i], "replay %d%s" % (r, " after an eager post-process with other ori_shapes" if r == 1 else ""), g_dets, g_nd)
        print("\nNET %-60s 4 replays == eager reference with the capture-time ori_shapes" % "tiny 128x192 B1, letterbox ownership")
    finally:
        del g


def test_capture_in_two_pieces():
    """as bench.py --hipgraph 2: forward_part(img, 0, k) in one graph, forward_part(None, k, -1) + postprocess in a second one, both captured on one side stream and
    replayed in order on it; k is the first op of the backbone that runs on a map of an eighth of the image"""
    det, ref, f = net_pair("yolov7-tiny", (128, 192), 1, False)
    want = [eager_reference(ref, f[i:i + 1]) for i in range(3)]
    dev_in = f[0:1].clone()
    side = torch.cuda.Stream()
    n_ops = len(det.plan.ops)
    k = next(i for i, op in enumerate(det.plan.ops) if int(op["H"]) <= 128 // 8)
    assert 0 < k < min(det.plan.detect_ops) and k < n_ops, (k, n_ops)
    with torch.cuda.stream(side):
        out = det.forward(dev_in, fuse_decode=CONF)                                     # warm-up: plan selection, kernel attributes, letterbox upload
        det.postprocess(out, CONF, IOU, None)
    torch.cuda.synchronize()
    g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g1, stream=side):
            det.forward_part(dev_in, 0, k, fuse_decode=CONF)
        with torch.cuda.graph(g2, stream=side):
            det.forward_part(None, k, -1, fuse_decode=CONF)
            g_dets, g_nd = det.postprocess(out, CONF, IOU, None)
        for r, i in enumerate([0, 1, 2, 0]):
            with torch.cuda.stream(side):
                dev_in.copy_(f[i:i + 1])
                poison_outputs(det, 1)
                g1.replay()
                g2.replay()
            torch.cuda.synchronize()
            assert_equal_to_reference(det, 1, want[i], "two graphs, replay %d" % r, g_dets, g_nd)
        print("\nNET %-60s 4 replays of two graphs (cut at op %d of %d) == eager reference" % ("tiny 128x192 B1, captured in two pieces", k, n_ops))
    finally:
        del g1, g2
