"""CPU: the staged references of the fused OSNet kernel's taps (tests/reid_fused_ref.py) pinned before the GPU tests rest on them
(tests/test_reid_fused_taps_gpu.py): each against torch.nn.functional in float64; chained, against the oracle network; and the bars themselves -- a host emulation of
the kernel (fp32 sums in a shuffled order, fp16 stores) passes every one of them, and the same emulation with ONE planted fault trips the bar of the faulty tensor,
for faults that the whole-network bars (3e-3 of max|feature|, cosine >= 1 - 1e-5) let through: their end-to-end effect is printed as a record, not asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import op_refs as R
from tests import reid_fused_ref as FR
from tests.test_reid_gpu import _edge_boxes, _edge_frames

RTOL = 1e-12


def params(sd):
    from yolov7_tracker_amd.tracker import reid
    return FR.decode_blob(reid.pack_fused(sd, reid.osnet_spec(0.25)))


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).permute(0, 3, 1, 2)


def close(ref, want_nchw):
    np.testing.assert_allclose(ref, want_nchw.permute(0, 2, 3, 1).numpy(), rtol=RTOL, atol=1e-13)


@pytest.fixture(scope="module")
def P():
    return params(FR.gate_scaled_state_dict(FR.GATE_FACTOR))


def test_staged_references_against_torch_functional(P):
    rng = R.rng_for("fused refs")
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    # stem over the haloed crop == conv2d(padding=3) over its interior
    cr = np.zeros((2, 134, 72, 4))
    cr[:, 3:131, 3:67, :3] = rng.standard_normal((2, 128, 64, 3))
    ref, b = FR.ref_c1(P, cr)
    close(ref, F.relu(F.conv2d(nchw(cr[:, 3:131, 3:67, :3]), t64(P["stem"][0]), t64(P["stem"][1]), 2, 3)))
    assert ref.shape == (2, 64, 32, 16) and (b > 0).all()
    c1 = np.abs(rng.standard_normal((2, 64, 32, 16)))
    close(FR.ref_x0(c1)[0], F.max_pool2d(nchw(c1), 3, 2, 1))
    for blk, (name, H, W, cin, cout, mid, Rr, mid_real) in zip(P["blocks"], FR.BLOCKS):
        x = rng.standard_normal((2, H, W, cin))
        x1, _ = FR.ref_conv1x1(x, blk["c1w"], blk["c1b"], True)
        close(x1, F.relu(F.conv2d(nchw(x), t64(blk["c1w"])[:, :, None, None], t64(blk["c1b"]))))
        w, dw, db = blk["lights"][3]
        u, ub = FR.ref_u(x1, w)
        close(u[:, 1:-1, 1:-1], F.conv2d(nchw(x1), t64(w)[:, :, None, None]))
        assert not u[:, 0].any() and not u[:, -1].any() and not u[:, :, 0].any() and not u[:, :, -1].any() and not ub[:, 0].any()
        t, tb = FR.ref_t(u, dw, db)
        close(t, F.relu(F.conv2d(nchw(u[:, 1:-1, 1:-1]), t64(dw).reshape(mid, 1, 3, 3), t64(db), padding=1, groups=mid)))
        s, sb = FR.ref_s(t, tb)
        np.testing.assert_allclose(s, nchw(t).sum((2, 3)).numpy(), rtol=RTOL)
        assert (sb >= tb.sum((1, 2))).all()
        parts = rng.uniform(0, 1, (2, FR.NW, mid)) * (H * W / FR.NW)
        g, gb = FR.ref_gate(blk, parts, H * W)
        pooled = t64(parts.sum(1) / (H * W))
        want = torch.sigmoid(F.relu(pooled @ t64(blk["g_w1"]).T + t64(blk["g_b1"])) @ t64(blk["g_w2"]) + t64(blk["g_b2"]))
        np.testing.assert_allclose(g, want.numpy(), rtol=RTOL)
        assert (gb >= 2.5 * R.U32).all() and np.isfinite(gb).all()
        # block output: plain gates against torch; the fp16-rounded gated weights against their own definition
        ts = [np.abs(rng.standard_normal((2, H, W, mid))) for _ in range(4)]
        gs = [rng.uniform(0, 1, (2, mid)).astype(np.float32) for _ in range(4)]
        got, _ = FR.ref_x(blk, x, ts, gs, emulate_f16=False)
        x2 = sum(nchw(t_) * t64(g_)[:, :, None, None] for t_, g_ in zip(ts, gs))
        y = F.conv2d(x2, t64(blk["c3w"])[:, :, None, None], t64(blk["c3b"]))
        close(got, F.relu(y + (F.conv2d(nchw(x), t64(blk["dnw"])[:, :, None, None]) if blk["dnw"] is not None else nchw(x))))
        wg = FR.gated_w3(blk["c3w"], gs[0])
        assert np.array_equal(wg, wg.astype(np.float16).astype(np.float64))
        exact = blk["c3w"].astype(np.float64)[None] * gs[0].astype(np.float64)[:, None, :]
        assert (np.abs(wg - exact) <= 2.0 ** -11 * np.abs(exact) * (1 + 2.0 ** -23) + 2.0 ** -25).all()
        got16, _ = FR.ref_x(blk, x, ts, gs)
        assert np.abs(got16 - got).max() <= 2e-3 * np.abs(got).max() and not np.array_equal(got16, got)
        if name in FR.TRANS:
            tn, c = FR.TRANS[name]
            xo = rng.standard_normal((2, H, W, c))
            yy, _ = FR.ref_conv1x1(xo, P[tn][0], P[tn][1], True)
            close(yy, F.relu(F.conv2d(nchw(xo), t64(P[tn][0])[:, :, None, None], t64(P[tn][1]))))
            close(FR.ref_pool(yy)[0], F.avg_pool2d(nchw(yy), 2))
    y5 = rng.standard_normal((2, 8, 4, 128))
    v, _ = FR.ref_v(y5)
    np.testing.assert_allclose(v, nchw(y5).mean((2, 3)).numpy(), rtol=RTOL)
    np.testing.assert_allclose(FR.ref_feats(P, v)[0], F.relu(t64(v) @ t64(P["fc"][0]).T + t64(P["fc"][1])).numpy(), rtol=RTOL, atol=1e-13)
    # the fp16 bar: the bound itself, half an fp16 ulp of |ref| + bound, half the subnormal spacing
    assert FR.f16_bar(np.float64(1.0), 1e-6) == 1e-6 + 2.0 ** -11 * (1 + 1e-6) + 2.0 ** -25
    with pytest.raises(AssertionError):
        FR.f16_bar(np.float64(70000.0), 0.0)


def test_crop_reference_against_the_preprocessing_oracle():
    """ref_cr (float64 blend with the kernel's float32 geometry) against oracle/reid_torch.preprocess (float32 throughout) on the edge boxes: a few float32 roundings"""
    from oracle import reid_torch
    noise, _ = _edge_frames()
    full, empty = _edge_boxes(96, 80)
    boxes = np.concatenate([full, empty])
    ref, bar = FR.ref_cr(noise, boxes, np.zeros(len(boxes), np.int32))
    want = reid_torch.preprocess(noise[0], full).numpy().transpose(0, 2, 3, 1)
    np.testing.assert_allclose(ref[:len(full), 3:131, 3:67, :3], want, rtol=1e-5, atol=2e-5)
    assert not ref[len(full):].any() and not bar[len(full):].any() and not ref[..., 3].any() and not ref[:, :3].any() and not ref[:, :, 67:].any()
    assert (bar[:len(full), 3:131, 3:67, :3] < 2.0 ** -11 * (np.abs(want) + 1e-3) + 1e-5).all()


def test_chained_references_are_the_oracle_network():
    """the staged references chained without teacher forcing and without fp16 stores == oracle/reid_torch.osnet_forward in float64, up to the fp16 rounding of the
    blob's weights (the 2e-3 bar of test_fused_blob_encodes_the_network)"""
    from oracle import reid_torch
    from yolov7_tracker_amd.tracker import reid
    sd = reid.random_state_dict(reid.osnet_spec(0.25), 5)
    x = torch.randn((3, 3, 128, 64), generator=torch.Generator().manual_seed(4))
    got = FR.chain(params(sd), x.numpy())
    want = reid_torch.osnet_forward(sd, x, dtype=torch.float64).numpy()
    assert got.shape == want.shape == (3, 512) and float(np.abs(want).mean()) > 0.05
    assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------- the bars, on a host emulation of the kernel
@pytest.fixture(scope="module")
def scene():
    """four of the edge boxes on the noise frames (the whole frame, fractional corners, a 2 x 3 enlargement, an empty crop), one of them on another frame"""
    noise, _ = _edge_frames()
    full, empty = _edge_boxes(96, 80)
    return noise, np.stack([full[4], full[8], full[3], empty[1]]), np.array([0, 2, 1, 0], np.int32)


@pytest.fixture(scope="module")
def clean(P, scene):
    return FR.emulate(P, *scene, seed=1)


def tripped(P, scene, taps):
    return {name for fam, name, got, ref, bar in FR.staged(P, *scene, taps) if not FR.worst(got, ref, bar)[0]}


def test_emulated_kernel_passes_every_bar(P, scene, clean):
    rows = [(fam, name) + FR.worst(got, ref, bar) for fam, name, got, ref, bar in FR.staged(P, *scene, clean)]
    assert {r[0] for r in rows} == set(FR.FAMILIES) and len(rows) > 6 * 30
    for fam in FR.FAMILIES:
        print("MARGIN emulation %-12s worst err/bar %.3f over %d tensors" % (fam, max(r[3] for r in rows if r[0] == fam), sum(r[0] == fam for r in rows)))
    assert not [r for r in rows if not r[2]]
    assert np.isfinite(clean["feats"]).all() and float(np.abs(clean["feats"]).mean()) > 0.05


@pytest.mark.parametrize("fault", sorted(FR.FAULTS))
def test_the_bars_have_teeth(P, scene, clean, fault):
    """one planted fault at a time: the bar of the faulty tensor trips.  The record printed is what the fault does to the 512-d feature -- what the whole-network
    test sees of it (bars there: 3e-3 of max|feature|, 1 - cos <= 1e-5)"""
    taps = FR.emulate(P, *scene, seed=1, fault=fault)
    names = tripped(P, scene, taps)
    a, b = taps["feats"].reshape(-1, 512).astype(np.float64), clean["feats"].reshape(-1, 512).astype(np.float64)
    err = float(np.abs(a - b).max() / np.abs(b).max())
    cos = float((1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))).max())
    print("FAULT %-62s trips %-28s end to end: err/scale %.1e, 1 - cos %.1e" % (fault, FR.FAULTS[fault], err, cos))
    assert FR.FAULTS[fault] in names, sorted(names)[:8]
