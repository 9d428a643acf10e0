"""CPU: the instrument of tests/test_conv_forms_gpu.py has teeth.  (1) tests/conv_ref.py::conv_ref equals torch.nn.functional.conv2d in float64 on every geometry kind the
GPU file uses (k 1 / 3, stride 1 / 2, odd maps, channel slices, the upsampled channel range, the twin form) at small sizes.  (2) A numpy emulation of a kernel -- exact
fp16 x fp16 products, fp32 partial sums in a shuffled order, optionally split into S slabs of 64-wide K-steps that are summed in order, fp32 bias and activation, fp16 (or
fp32) store into a slice of a wider buffer with a sentinel around it -- passes every bar on three seeds.  (3) The same emulation with ONE planted fault trips every time:
the faults are the index and rounding mistakes that kernels of this family make (a dropped tap, the wrapped padding column, the neighbour's bias, a skipped K-step, the
unshifted upsample column, fp16 accumulation, a tile stored one image too far; for the Detect epilogue two candidates in one slot and a block based on the wrong image's
counter).  `python -m pytest -s` prints the table of worst err / tol per geometry and fault (profiles/conv_forms_margins.txt keeps one)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as cr

SENTINEL = 7.0
SEEDS = (0, 1, 2)

# name -> B, H, W, Cin, Cout, k, s, act, S (slabs), f32 out, up (up_c0, up_C) or None
GEOMETRIES = {
    "3x3 s1 9x11 64->24 silu":            (2, 9, 11, 64, 24, 3, 1, 1, 1, 0, None),
    "3x3 s1 9x11 128->24 silu splitK 3":  (2, 9, 11, 128, 24, 3, 1, 1, 3, 0, None),
    "3x3 s2 10x14 64->20 leaky":          (2, 10, 14, 64, 20, 3, 2, 2, 1, 0, None),
    "3x3 s2 13x9 8->16 silu (K = 72)":    (3, 13, 9, 8, 16, 3, 2, 1, 1, 0, None),
    "1x1 10x14 40->45 fp32 head":         (2, 10, 14, 40, 45, 1, 1, 0, 1, 1, None),
    "1x1 10x14 512->44 splitK 4":         (2, 10, 14, 512, 44, 1, 1, 1, 4, 0, None),
    "1x1 10x14 160->16 up [32, 128)":     (2, 10, 14, 160, 16, 1, 1, 1, 1, 0, (32, 96)),
    "1x1 10x14 160->16 up [96, 160)":     (2, 10, 14, 160, 16, 1, 1, 2, 1, 0, (96, 64)),
}
ROWS = []      # (geometry, fault, seed, worst err / tol, guard values overwritten)


def _data(g, seed, in_ld_extra=8):
    B, H, W, Cin, Cout, k, s, act, S, f32, up = GEOMETRIES[g]
    rng = np.random.default_rng(seed)
    buf = rng.normal(0, 1, (B, H, W, Cin + in_ld_extra)).astype(np.float16)           # the input is channels [8, 8 + Cin) of a wider buffer
    lo = rng.normal(0, 1, (B, H // 2, W // 2, 32 + (up[1] if up else 0))).astype(np.float16) if up else None
    w = (rng.normal(0, 1, (Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float16)
    b = rng.normal(0, 0.5, Cout).astype(np.float32)
    return buf, lo, w, b


def _gather(buf, lo, g, fault):
    """-> cols (M, taps, Cin) float32: what the kernel multiplies, tap by tap (zeros for padding taps)"""
    B, H, W, Cin, Cout, k, s, act, S, f32, up = GEOMETRIES[g]
    x = np.array(buf[..., 8:8 + Cin], np.float32)
    if up:
        c0, C = up
        l = lo[..., 32:32 + C].astype(np.float32)
        yy, xx = np.arange(H) >> 1, np.arange(W) >> 1
        if fault == "upsample column not shifted":      # (y >> 1, x): the flat offset runs into the following rows of the half-resolution image
            flat = (yy[:, None] * (W // 2) + np.arange(W)[None, :]) % ((H // 2) * (W // 2))
            x[..., c0:c0 + C] = l.reshape(B, -1, C)[:, flat]
        else:
            x[..., c0:c0 + C] = l[:, yy][:, :, xx]
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    cols = np.zeros((B, Ho, Wo, k * k, Cin), np.float32)
    flat = x.reshape(B * H * W, Cin)
    for kh in range(k):
        for kw in range(k):
            for ho in range(Ho):
                hi = ho * s + kh - p
                if not 0 <= hi < H:
                    continue
                for wo in range(Wo):
                    wi = wo * s + kw - p
                    if 0 <= wi < W:
                        cols[:, ho, wo, kh * k + kw] = x[:, hi, wi]
                    elif fault == "left padding tap wraps" and wi == -1:      # offset (b, hi, -1): the previous row's last pixel, the previous image's for hi == 0
                        idx = (np.arange(B) * H + hi) * W - 1
                        cols[idx >= 0, ho, wo, kh * k + kw] = flat[idx[idx >= 0]]
    if fault == "one tap dropped at a border pixel":
        cols[B - 1, 0, Wo - 1, (k * k) // 2] = 0                                  # the centre tap of the last image's top right pixel
    return cols.reshape(B * Ho * Wo, k * k, Cin), Ho, Wo


def emulate(g, seed, fault=None):
    """-> (out (rows, ld) with the guard rows behind M and the channels outside [4, 4 + Cout) left at SENTINEL, M)"""
    B, H, W, Cin, Cout, k, s, act, S, f32, up = GEOMETRIES[g]
    buf, lo, w, b = _data(g, seed)
    cols, Ho, Wo = _gather(buf, lo, g, fault)
    M, K = cols.shape[0], k * k * Cin
    A = cols.reshape(M, K)
    Wm = w.astype(np.float32).transpose(0, 2, 3, 1).reshape(Cout, K)
    steps = [np.arange(i, min(i + 64, K)) for i in range(0, K, 64)]
    per = -(-len(steps) // S)
    rng = np.random.default_rng(1000 + seed)
    accdt = np.float16 if fault == "fp16 accumulation" else np.float32
    total = None
    for sl in range(S):
        mine = steps[sl * per:(sl + 1) * per]
        if fault == "last K-step of one split skipped" and sl == S // 2:
            mine = mine[:-1]
        acc = np.zeros((M, Cout), accdt)
        for kk in rng.permutation(np.concatenate(mine)) if mine else []:
            acc = (acc + (A[:, kk:kk + 1] * Wm[None, :, kk]).astype(accdt)).astype(accdt)       # fp16 x fp16 is exact in fp32
        total = acc.astype(np.float32) if total is None else total + acc.astype(np.float32)
    bias = np.roll(b, -1) if fault == "bias of channel n + 1" else b
    v = total + bias
    v = (v / (np.float32(1) + np.exp(-v))).astype(np.float32) if act == 1 else np.where(v > 0, v, np.float32(0.1) * v) if act == 2 else v
    ld = Cout + 12
    out = np.full((M + Ho * Wo, ld), SENTINEL, np.float32 if f32 else np.float16)
    dst = np.arange(M)
    if fault == "last pixel tile one image too far":
        dst = np.where(dst >= (M - 1) // 128 * 128, dst + Ho * Wo, dst)
    out[dst, 4:4 + Cout] = v
    return out, M


def reference(g, seed):
    B, H, W, Cin, Cout, k, s, act, S, f32, up = GEOMETRIES[g]
    buf, lo, w, b = _data(g, seed)
    x = cr.concat_input(buf, 8, Cin, (lo, 32) + up if up else None)
    ref, absum = cr.conv_ref(x, w, b, k, s, act)
    return ref, absum, cr.tolerance(ref, absum, k * k * Cin)


def verdict(g, seed, fault=None):
    """-> (worst err / tol on the output slice, guard values overwritten); a case passes with ratio <= 1 and 0"""
    Cout = GEOMETRIES[g][4]
    out, M = emulate(g, seed, fault)
    ref, absum, tol = reference(g, seed)
    guard = out.astype(np.float64).copy()
    guard[:M, 4:4 + Cout] = SENTINEL
    ratio, spoiled = cr.worst_ratio(out[:M, 4:4 + Cout], ref, tol), int((guard != SENTINEL).sum())
    ROWS.append((g, fault or "none", seed, ratio, spoiled))
    return ratio, spoiled


# ------------------------------------------------------------------------------------------------ (1) the reference
@pytest.mark.parametrize("g", list(GEOMETRIES))
def test_reference_equals_torch_float64(g):
    B, H, W, Cin, Cout, k, s, act, S, f32, up = GEOMETRIES[g]
    buf, lo, w, b = _data(g, 5)
    xt = torch.from_numpy(buf[..., 8:8 + Cin].astype(np.float64)).permute(0, 3, 1, 2).clone()
    if up:
        l = torch.from_numpy(lo[..., 32:32 + up[1]].astype(np.float64)).permute(0, 3, 1, 2)
        xt[:, up[0]:up[0] + up[1]] = F.interpolate(l, scale_factor=2, mode="nearest")
    wt, bt = torch.from_numpy(w.astype(np.float64)), torch.from_numpy(b.astype(np.float64))
    want = F.conv2d(xt, wt, bt, stride=s, padding=k // 2)
    want = F.silu(want) if act == 1 else F.leaky_relu(want, 0.1) if act == 2 else want
    want_abs = F.conv2d(xt.abs(), wt.abs(), bt.abs(), stride=s, padding=k // 2)
    ref, absum, _ = reference(g, 5)
    np.testing.assert_allclose(ref, want.permute(0, 2, 3, 1).reshape(-1, Cout).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(absum, want_abs.permute(0, 2, 3, 1).reshape(-1, Cout).numpy(), rtol=1e-12, atol=1e-13)
    rows = cr.pixel_rows(B, *want.shape[2:], 16, 3)
    sub, sub_abs = cr.conv_ref(cr.concat_input(buf, 8, Cin, (lo, 32) + up if up else None), w, b, k, s, act, rows)
    assert np.array_equal(sub, ref[rows]) and np.array_equal(sub_abs, absum[rows]) and rows[0] == 0 and rows[-1] == len(ref) - 1


def test_twin_reference_equals_torch_float64():
    rng = np.random.default_rng(4)
    x = rng.normal(0, 1, (2, 10, 14, 16)).astype(np.float16)
    w1 = (rng.normal(0, 1, (32, 16, 3, 3)) / 12).astype(np.float16)
    w2 = (rng.normal(0, 1, (24, 32, 1, 1)) / np.sqrt(32)).astype(np.float16)
    b1, b2 = rng.normal(0, 0.5, 32).astype(np.float32), rng.normal(0, 0.5, 24).astype(np.float32)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    mid = F.silu(F.conv2d(t(x).permute(0, 3, 1, 2), t(w1), t(b1), stride=2, padding=1)).half().double()
    want = F.silu(F.conv2d(mid, t(w2), t(b2))).permute(0, 2, 3, 1).reshape(-1, 24).numpy()
    ref, absum = cr.twin_ref(x, w1, b1, w2, b2, 1)
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=1e-13)
    assert absum.shape == ref.shape and (absum >= np.abs(b2)).all()


# ------------------------------------------------------------------------------------------------ (2) the unfaulted emulation passes
@pytest.mark.parametrize("g", list(GEOMETRIES))
def test_unfaulted_emulation_passes_every_bar(g):
    for seed in SEEDS:
        ratio, spoiled = verdict(g, seed)
        assert ratio <= 1.0 and spoiled == 0, (g, seed, ratio, spoiled)


def test_fp32_outputs_stay_inside_the_fp32_only_bound():
    """the bound that the GPU file prints beside the bar for fp32 outputs: the emulation (fp32 sums in any order) must not pass it"""
    g = "1x1 10x14 40->45 fp32 head"
    for seed in SEEDS:
        out, M = emulate(g, seed)
        ref, absum, _ = reference(g, seed)
        assert cr.worst_ratio(out[:M, 4:49], ref, cr.f32_bound(ref, absum, 40)) <= 1.0


# ------------------------------------------------------------------------------------------------ (3) one planted fault each
FAULTS = {
    "one tap dropped at a border pixel": [g for g in GEOMETRIES if g.startswith("3x3")],
    "left padding tap wraps": [g for g in GEOMETRIES if g.startswith("3x3")],
    "bias of channel n + 1": list(GEOMETRIES),
    "last K-step of one split skipped": ["3x3 s1 9x11 64->24 silu", "3x3 s1 9x11 128->24 silu splitK 3", "1x1 10x14 512->44 splitK 4"],
    "upsample column not shifted": [g for g in GEOMETRIES if " up " in g],
    "fp16 accumulation": [g for g in GEOMETRIES if "K = 72" not in g and "40->45" not in g],      # (K >= 128: at K = 40 / 72 fp16 sums of a few terms can stay inside the bar)
    "last pixel tile one image too far": list(GEOMETRIES),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_trips(fault):
    for g in FAULTS[fault]:
        for seed in SEEDS:
            ratio, spoiled = verdict(g, seed, fault)
            assert ratio > 1.0 or spoiled > 0, (fault, g, seed, ratio, spoiled)
            if fault == "last pixel tile one image too far":
                assert spoiled > 0 and ratio > 1.0           # both instruments see it: the guard rows are written, the tile's own rows still hold the sentinel


# ------------------------------------------------------------------------------------------------ the Detect epilogue's bookkeeping
def _found(seed, B=7, HoWo=25, na=3, p=0.3):
    rng = np.random.default_rng(seed)
    found = [(m, (a * HoWo + m % HoWo)) for m in range(B * HoWo) for a in range(na) if m // HoWo != 3 and rng.random() < p]     # image 3 has no candidate
    return [found[i] for i in rng.permutation(len(found))]


def _check_candidates(found, count, slots, B, cap, HoWo):
    """what the GPU file asserts of the candidate arrays: per image the count is the number found; up to cap the slots hold exactly the found cidx, each once (all of
    them when the count fits); nothing is written behind min(count, cap)"""
    for b in range(B):
        want = sorted(c for m, c in found if m // HoWo == b)
        n = min(len(want), cap)
        got = sorted(slots[b, :n])
        if count[b] != len(want) or (slots[b, n:] != -1).any() or len(set(got)) != n or not set(got) <= set(want) or (len(want) <= cap and got != want):
            return False
    return True


@pytest.mark.parametrize("cap", [64, 8])
def test_candidate_bookkeeping_and_its_two_faults(cap):
    for seed in SEEDS:
        found = _found(seed)
        assert max(sum(1 for m, _ in found if m // 25 == b) for b in range(7)) > 8
        count, slots = cr.append_candidates(found, 7, cap, 25)
        assert count[3] == 0 and _check_candidates(found, count, slots, 7, cap, 25)
        for fault in ("two candidates share a slot", "block based on the previous image's counter"):
            count, slots = cr.append_candidates(found, 7, cap, 25, fault=fault)
            ok = _check_candidates(found, count, slots, 7, cap, 25)
            ROWS.append(("Detect epilogue 5x5 B7 cap %d" % cap, fault, seed, float("nan") if ok else float("inf"), 0))
            assert not ok, (fault, seed)


def test_decode_reference_equals_the_oracle_decode():
    """tests/conv_ref.py::decode_bounds against oracle/detector_torch.py::decode_level (the reference's Detect decode, pinned in tests/test_detector_oracle.py) in float64;
    the bounds are positive and grow with the logit bar"""
    from oracle import detector_torch as dt
    rng = np.random.default_rng(6)
    B, ny, nx, na, no, stride = 2, 3, 7, 3, 9, 16.0
    anchors = [(12.0, 16.0), (19.0, 36.0), (40.0, 28.0)]
    v = rng.normal(0, 2, (B, ny, nx, na * no))
    d = cr.decode_bounds(v, np.full(v.shape, 1e-3), na, no, ny, nx, stride, anchors, row0=5)
    y = dt.decode_level(torch.from_numpy(v).view(B, ny, nx, na, no).permute(0, 3, 1, 2, 4).contiguous(), torch.tensor(anchors, dtype=torch.float32), stride)
    want = y.double().numpy()[:, d["cidx"] - 5]                                 # (B, ny, nx, na, no): xywh, obj, class probabilities
    xywh = want[..., :4]
    box = np.concatenate([xywh[..., :2] - xywh[..., 2:] / 2, xywh[..., :2] + xywh[..., 2:] / 2], -1)
    np.testing.assert_allclose(d["box"], box, rtol=1e-5, atol=1e-4)             # (decode_level computes in float32)
    np.testing.assert_allclose(d["obj"], want[..., 4], rtol=1e-6)
    np.testing.assert_allclose(d["sc"], want[..., 5:] * want[..., 4:5], rtol=1e-5, atol=1e-7)
    d2 = cr.decode_bounds(v, np.full(v.shape, 2e-3), na, no, ny, nx, stride, anchors)
    assert (d["d_obj"] == 2.5e-4).all() and (d["d_sc"] == 5e-4).all() and (d["d_box"] > 0).all() and (d2["d_box"] > d["d_box"]).all() and (d2["d_sc"] == 2 * d["d_sc"]).all()


def test_dispatch_restatement_gives_the_hand_written_names():
    """tests/util.py::conv_dispatch_name (what tests/test_family_gpu.py asserts for the shapes its plans bring) against every name written by hand in the case lists of
    tests/test_detector_gpu.py"""
    from tests import test_detector_gpu as tdg, util
    for case in tdg.CONV_CASES:
        assert util.conv_dispatch_name(case) == case[13], (case, util.conv_dispatch_name(case))
    for cases, name in ((tdg.WS_CASES, "ws64<16,16>"), (tdg.WS128_CASES, "ws128<4,16>"), (tdg.WS128_S2_CASES, "ws128_s2<2,16>"), (tdg.WS_S2_CASES, "ws_s2<2,32>"),
                        (tdg.P8_CASES, "p8<256,256,64> 1x1")):
        assert all(util.conv_dispatch_name(c) == name for c in cases), name
    assert {util.conv_dispatch_name(c) for c in tdg.S2_CASES} == {"patch_s2<128>", "patch_s2<256>"}


def test_print_the_table():
    """(runs last in the file: one line per geometry and fault, the worst of the seeds)"""
    worst = {}
    for g, fault, seed, ratio, spoiled in ROWS:
        r0, s0 = worst.get((g, fault), (None, 0))
        lo_hi = min if fault != "none" else max                                    # a fault's weakest showing, the clean emulation's worst
        worst[(g, fault)] = (ratio if r0 is None else lo_hi(r0, ratio), max(s0, spoiled))
    print("\n%-40s %-46s %14s %8s" % ("geometry", "planted fault", "worst err/tol", "guard"))
    for (g, fault), (ratio, spoiled) in worst.items():
        print("TABLE %-40s %-46s %14.3g %8d" % (g, fault, ratio, spoiled))
    assert all(r <= 1.0 for (g, f), (r, s) in worst.items() if f == "none")
