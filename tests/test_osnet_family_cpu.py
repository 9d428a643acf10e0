"""CPU: the references of the general OSNet path (tests/osnet_f16_ref.py) and its lowering (tracker/reid.py::lower_osnet_f16), without a GPU.

  * chain() -- the op list and its weight blob interpreted in float64 without fp16 stores -- equals the reference module's float64 embedding of every fixture
    (tests/golden/osnet_family_<name>.npz, made from the reference's own constructors) up to the fp16 rounding of the weights;
  * emulate() passes every per-op bar of staged() and keeps every pad channel zero; each planted fault trips a bar (or the pad check);
  * the lowering: op count, buffer sizes, IBN detection, and random_state_dict(ibn=False) bit-equal to the digests recorded from the commit before the IBN
    parameters existed."""
import hashlib
import os

import numpy as np
import pytest

from tests import osnet_f16_ref as O
from yolov7_tracker_amd.tracker import reid

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = list(reid.OSNET_NAMES)
# sha256 over the sorted (name, float32 bytes) of random_state_dict(osnet_spec(width), seed) at the parent commit
PARENT_DIGESTS = {(0.25, 0): "3445076c426f1f6e8b18534498ffa1a8e29e2b979e71b61f17e07eebbe38c28e", (0.5, 3): "013d2535f92878d26b368ccfd0257f9c147db94027980d28ee081d2698415779",
                  (0.75, 7): "b599f4c862eb069dd6599f9f3810b0b16115509d4649702ee19f72fa60e6d512", (1.0, 11): "92caaabe49c9b6e413c3902f776b8a333ab6418d47b1caf39f2051fb975d458a"}
_CACHE = {}


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].numpy()).tobytes())
    return h.hexdigest()


def fixture(name):
    """-> (npz, spec, state dict): the seeded weights the fixture was made with, checked against its digest"""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLD, "osnet_family_%s.npz" % name))
        width, ibn = reid.OSNET_NAMES[name]
        spec = reid.osnet_spec(width, ibn=ibn)
        sd = reid.random_state_dict(spec, int(z["seed"]))
        assert digest(sd) == str(z["digest"]), "the seeded state dict is not the one the fixture was recorded with"
        _CACHE[name] = (z, spec, sd)
    return _CACHE[name]


def lowered(name, key, strip=0):
    z, spec, sd = fixture(name)
    x = z["crops_" + key]
    k = (name, x.shape[1:3], strip)
    if k not in _CACHE:
        _CACHE[k] = reid.lower_osnet_f16(sd, spec, x.shape[1], x.shape[2], strip=strip)
    return _CACHE[k] + (x, z["emb_" + key], spec)


@pytest.mark.parametrize("name", NAMES)
def test_random_state_dict_matches_its_fixture_digest(name):
    fixture(name)


@pytest.mark.parametrize("width,seed", sorted(PARENT_DIGESTS))
def test_random_state_dict_without_ibn_draws_the_parent_sequence(width, seed):
    assert digest(reid.random_state_dict(reid.osnet_spec(width), seed)) == PARENT_DIGESTS[(width, seed)]


def test_ibn_state_dict_and_detection():
    sd = reid.random_state_dict(reid.osnet_spec(1.0, ibn=True), 2)
    plain = reid.random_state_dict(reid.osnet_spec(1.0), 2)
    assert reid.is_ibn(sd) and not reid.is_ibn(plain) and reid.is_ibn({"module." + k: v for k, v in sd.items()})
    assert "conv1.bn.running_mean" not in sd and sd["conv1.bn.weight"].shape == (64,) and sd["conv2.1.IN.bias"].shape == (256,)
    shared = [k for k in plain if not k.startswith("conv1.bn.")]
    assert all(np.array_equal(sd[k].numpy(), plain[k].numpy()) for k in shared)           # the IBN parameters are drawn after everything else
    assert set(sd) - set(plain) == {"conv2.0.IN.weight", "conv2.0.IN.bias", "conv2.1.IN.weight", "conv2.1.IN.bias"}


@pytest.mark.parametrize("name", NAMES)
def test_lowering_op_count_and_buffers(name):
    ops, bufs, w, x, _, spec = lowered(name, "c")
    ibn = bool(spec.get("ibn"))
    # stem, pool, 6 blocks of (conv1, 4 levels, gate-sum, conv3 [+ IN]), 2 transitions of (1x1, avgpool), conv5, gap-fc
    assert len(ops) == 2 + 6 * 7 + 4 + 2 + (3 if ibn else 0) and len(O.real_channels(spec)) == len(ops)
    launches = len(ops) + 1 + 1                                  # + the crop sampler, + the gap of the tail
    assert launches <= 60
    assert [int(o["type"]) for o in ops].count(reid.H_OS_LIGHT) == 24
    for o in ops:
        assert int(o["w_off"]) % 4 == 0 and (int(o["b_off"]) < 0 or int(o["b_off"]) % 4 == 0) and int(o["C"]) % (1 if int(o["type"]) == reid.H_OS_STEM else 16) == 0
        t, H, W, C, Co = int(o["type"]), int(o["H"]), int(o["W"]), int(o["C"]), int(o["Co"])
        if t == reid.H_OS_PW:
            assert bufs[int(o["out_buf"])] == H * W * Co // 2 and bufs[int(o["in_buf"])] == H * W * C // 2
        if t == reid.H_OS_LIGHT:
            S, strips = O.strips_of(o)
            assert S >= 1 and bufs[int(o["out_buf"])] == reid.OS_SLOTS * H * W * C // 2 and bufs[int(o["aux_buf"])] == 4 * strips * C
    assert bufs[0] == 128 * 64 * 3 and bufs[int(ops[-1]["out_buf"])] == 512
    ch = spec["channels"]
    assert int(ops[0]["Co"]) == reid.pad16(ch[0]) and (int(ops[0]["Ho"]), int(ops[0]["Wo"])) == (64, 32)


def test_strip_rule_at_the_real_geometry():
    """x1_0 on 128 x 256 crops (StrongSORT): stage-2 maps are 32 x 64 with mid 64 -- one crop's plane is 256 KB, the strip must fit 60 KB with its halo"""
    assert reid.os_strip_rows(32, 64, 64) == 5 and (5 + 2) * 66 * 64 * 2 <= reid.OS_LDS_BUDGET < (6 + 2) * 66 * 64 * 2
    assert reid.os_strip_rows(4, 1, 16) == 4 and reid.os_strip_rows(7, 4, 32, 3) == 3 and reid.os_strip_rows(7, 4, 32, 100) == 7
    assert reid.os_strip_rows(8, 1000, 128) == 0
    assert [reid.os_level_slot(j) for j in range(4)] == [0, 4, 7, 9]
    with pytest.raises(ValueError):
        reid.lower_osnet_f16(fixture("osnet_x0_25")[2], reid.osnet_spec(0.25), 120, 64)


@pytest.mark.parametrize("key", ["a", "b", "c"])
@pytest.mark.parametrize("name", NAMES)
def test_chain_is_the_reference_module(name, key):
    """float64, no fp16 stores: what is left is the fp16 rounding of the 1x1 / stem / fc weights -- each weight off by at most 2^-11 relative, ~60 layers deep.  The
    bar is 60 layers x 2^-11 relative L2 (first order, every layer's perturbation arriving whole)"""
    ops, bufs, w, x, emb, spec = lowered(name, key)
    got = O.chain(ops, w, x)
    d = O.rel_l2(got, emb)
    print("CHAIN %-16s %s  rel L2 %.3e" % (name, x.shape, d))
    assert d <= 60 * 2.0 ** -11


@pytest.mark.parametrize("key,strip", [("a", 0), ("a", 3), ("b", 1)])
@pytest.mark.parametrize("name", NAMES)
def test_emulation_passes_its_own_bars(name, key, strip):
    ops, bufs, w, x, emb, spec = lowered(name, key, strip)
    feats, B = O.emulate(ops, w, x)
    res = O.worst(ops, w, B, x.shape[0])
    bad = [r for r in res if r[2] > 1.0]
    print("EMU %-16s %s strip %d: %d comparisons, worst err/bar %.3f, rel L2 to the fixture %.3e" % (name, x.shape, strip, len(res), max(r[2] for r in res), O.rel_l2(feats, emb)))
    assert not bad, bad[:5]
    assert O.pads_nonzero(ops, B, x.shape[0], O.real_channels(spec)) == []


# fault -> (network, crop set, strip rows): a configuration in which the fault changes something (strips > 1 for the halo faults, pads for the pad fault)
FAULT_CASES = {"halo_wrong_side": ("osnet_x0_5", "a", 2), "halo_clamped": ("osnet_x0_5", "a", 3), "gate_shift": ("osnet_x0_25", "a", 0),
               "unbiased_var": ("osnet_ibn_x1_0", "a", 0), "no_relu_pool": ("osnet_x0_5", "b", 0), "pad_nonzero": ("osnet_x0_75", "a", 0)}


@pytest.mark.parametrize("fault", O.FAULTS)
def test_planted_fault_trips_a_bar(fault):
    name, key, strip = FAULT_CASES[fault]
    ops, bufs, w, x, emb, spec = lowered(name, key, strip)
    feats, B = O.emulate(ops, w, x, fault=fault)
    res = O.worst(ops, w, B, x.shape[0])
    over = [r for r in res if r[2] > 1.0]
    pads = O.pads_nonzero(ops, B, x.shape[0], O.real_channels(spec))
    print("FAULT %-16s over the bar: %d of %d comparisons (first %s), pad checks failed: %d" % (fault, len(over), len(res), over[:1], len(pads)))
    assert over or pads
    if fault == "pad_nonzero":
        assert pads
