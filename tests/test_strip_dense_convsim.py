"""CPU: the DENSE strip form of the LDS-patch kernel (csrc/y7t_conv_patch.hip, FLAT: W = 20, 40) from its real source on the host model of tests/_convsim.
The strip is the B*H*W pixels of the launch with no padding position; a tap that leaves the image would read the wrapped neighbour (the end of the previous
row, the last row of the previous image) and is replaced, lane by lane, by a read of a zeroed LDS region.  Pinned here: the dense load geometry and epilogue
(tiles that straddle rows and images, a ragged last tile, one to three chunk pairs, slices, every weight order), that the replacement is a SELECTION (NaN in
the wrapped neighbour never reaches a pixel whose window does not hold it), and -- statically, the host model has no banks -- that a service group of the
masked fragment reads still touches 16 different 16-byte slots."""
import numpy as np
import pytest
import torch

from tests import _convsim as cs
from tests import test_convsim as t

pytestmark = pytest.mark.skipif(not __import__("os").path.exists(cs._CLANG), reason="needs the ROCm clang++ (host compile of the kernel source)")

# B, H, W, Cin, Cout, act, korder, slices
DENSE_CASES = [
    (3, 20, 20, 64, 64, 1, t.WL.LINE_MAJOR, {}),                                      # 1200 pixels: tiles straddle image boundaries, ragged last tile
    (2, 7, 20, 128, 128, 1, t.WL.PATCH, {}),                                          # 280 pixels: one tile spans two image boundaries; two chunk pairs, 128-row panels
    (1, 13, 40, 192, 64, 2, t.WL.LINE_MAJOR, {"in_ld": 256, "in_coff": 64, "out_ld": 192, "out_coff": 64}),  # three passes of the chunk-pair loop, slices, LeakyReLU
    (2, 20, 20, 64, 128, 1, t.WL.PATCH_N64, {}),                                      # 64-row panels on a 128-channel layer
]


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: "%dx%dx%d_%d-%d_o%d" % (c[0], c[1], c[2], c[3], c[4], c[6]))
def test_dense_strip_kernel_source_on_the_host(case):
    B, H, W, Cin, Cout, act, korder, kw = case
    name = t.run_case(cs.lib(), B, H, W, Cin, Cout, 3, 1, act, 0, korder=korder, force_patch=1, **kw)
    assert name.startswith("patch_strip<%d," % W), name


def poisoned_input(B, H, W, C, seed):
    """normal input with NaN in column W-1 and row H-1 of every image: exactly the pixels a wrapped tap would read (x = 0 reads the previous row's last column,
    y = 0 the previous image's last row) -- and the NaN mask a 3x3 / pad 1 convolution must produce from it"""
    x = np.random.default_rng(seed).normal(0, 1, (B, H, W, C)).astype(np.float16)
    x[:, :, W - 1, :] = np.nan
    x[:, H - 1, :, :] = np.nan
    bad = torch.zeros(B, 1, H, W)
    bad[:, :, :, W - 1] = 1
    bad[:, :, H - 1, :] = 1
    return x, torch.nn.functional.max_pool2d(bad, 3, 1, 1)[:, 0].bool().numpy()


def test_dense_strip_border_taps_are_selected_not_multiplied_on_the_host():
    """act 0 on the 3 x 20 x 20 shape: isnan(out) == isnan(reference) exactly (a border tap multiplied by zero, or not masked, would spread NaN to x = 0 and
    y = 0), and the finite values within the bar of the other cases"""
    B, H, W, Cin, Cout = 3, 20, 20, 64, 64
    x, want_nan = poisoned_input(B, H, W, Cin, 3)
    rng = np.random.default_rng(4)
    Wt = (rng.normal(0, 1, (Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    bias = rng.normal(0, 0.5, Cout).astype(np.float32)
    wp = t.pack_w(Wt, Cin, Cout, t.WL.LINE_MAJOR)
    out = np.full((B, H, W, Cout), 7.0, np.float16)
    L = cs.lib()
    rc = L.cs_conv(x.ctypes.data, Cin, 0, B, H, W, Cin, wp.ctypes.data, bias.ctypes.data, out.ctypes.data, Cout, 0, 0, Cout, Cout, 3, 3, 1, 1, 0, t.WL.LINE_MAJOR, 0, 0, 1)
    assert rc == 0, L.cs_last_error().decode()
    assert L.cs_last_kernel().decode().startswith("patch_strip<20,")
    ref = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), torch.from_numpy(Wt.astype(np.float16).astype(np.float32)),
                                     torch.from_numpy(bias), 1, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(np.isnan(ref), np.broadcast_to(want_nan[..., None], ref.shape))      # (the reference itself: NaN exactly where the window holds one)
    assert 0 < want_nan.sum() < want_nan.size
    got = out.astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=2e-3, atol=2e-3)


def _cfg(PW, BN):
    """PatchCfg<0, PW, BN> of csrc/y7t_conv_patch.hip"""
    npos = 256 + 2 * PW + 2
    patch_bytes = (npos * 80 + 1023) // 1024 * 1024
    w_bytes = BN * 64
    p_off = 3 * w_bytes
    lds_loop, lds_epi = p_off + 2 * patch_bytes, 256 * (BN * 2 + 16)
    bias_off = max(lds_loop, lds_epi + 1024)
    wn = BN // 64
    return dict(P_OFF=p_off, PATCH_BYTES=patch_bytes, ZERO_OFF=bias_off + BN * 4, ZERO_BYTES=576, TM=8 // (4 // wn), WM=4 // wn)


def test_dense_strip_fragment_reads_are_bank_conflict_free():
    """Static model of the patch fragment addresses of the dense strip (the simulator does not model banks).  ds_read_b128 is served in four groups of 16 lanes --
    {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- and a group is conflict-free when the 16-byte units it touches are distinct mod 256 bytes, lanes
    that read the same address counting once.  Every tap, MFMA tile, k-substep, wave and patch buffer of tiles that hold row ends and image boundaries, for
    (a) the address select the kernel uses -- a lane whose tap leaves the image reads ZERO_OFF + its own slot -- and (b) plain reads of the wrapped neighbour
    (fragment zeroing).  A zero region addressed without the lane's slot is checked to collide, so that the model is known to see it."""
    g1 = list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28))
    g2 = list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))
    groups = [g1, g2, [l + 32 for l in g1], [l + 32 for l in g2]]

    def conflict_free(addrs):
        return all(len({(a // 16) % 16 for a in {addrs[l] for l in g}}) == len({addrs[l] for l in g}) for g in groups)

    seen_masked = seen_collision = 0
    for PW, H, g0s in ((20, 7, (0, 256)), (20, 20, (256, 1024)), (40, 13, (256, 512)), (40, 40, (1536,))):
        for BN in (64, 128):
            c = _cfg(PW, BN)
            assert c["ZERO_OFF"] % 256 == 0 and c["P_OFF"] % 256 == 0 and c["PATCH_BYTES"] % 256 == 0 and c["ZERO_OFF"] + c["ZERO_BYTES"] <= 81920
            for g0 in g0s:
                for wm in range(c["WM"]):
                    for j in range(c["TM"]):
                        facts = []
                        for l31 in range(32):
                            g = g0 + (wm * c["TM"] + j) * 32 + l31
                            x, y = g % PW, (g // PW) % H
                            facts.append((x == 0, x == PW - 1, y == 0, y == H - 1))
                        for kh in range(3):
                            for kw in range(3):
                                shift = kh * PW + kw
                                for ks in range(2):
                                    for pb in range(2):
                                        real, sel, naive = {}, {}, {}
                                        for lane in range(64):
                                            l31, hi32 = lane & 31, lane >> 5
                                            x0, xw, y0, yh = facts[l31]
                                            out = (kh == 0 and y0) or (kh == 2 and yh) or (kw == 0 and x0) or (kw == 2 and xw)
                                            a = c["P_OFF"] + pb * c["PATCH_BYTES"] + ((wm * c["TM"] + j) * 32 + l31 + shift) * 80 + hi32 * 16 + ks * 32
                                            z = c["ZERO_OFF"] + (((5 * l31 + hi32) & 15) << 4) + (((5 * shift) & 15) << 4) + ks * 32
                                            assert c["ZERO_OFF"] <= z and z + 16 <= c["ZERO_OFF"] + c["ZERO_BYTES"]
                                            assert (z // 16) % 16 == (a // 16) % 16          # the zero address keeps the slot of the address it replaces
                                            real[lane], sel[lane], naive[lane] = a, (z if out else a), (c["ZERO_OFF"] + hi32 * 16 if out else a)
                                            seen_masked += out
                                        assert conflict_free(real)                             # (b): the wrapped neighbour is an ordinary patch read
                                        assert conflict_free(sel), (PW, H, BN, g0, wm, j, kh, kw, ks)      # (a)
                                        seen_collision += not conflict_free(naive)
    assert seen_masked > 1000 and seen_collision > 100
