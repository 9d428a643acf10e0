"""The margins of the host-build tests of csrc/y7t_tta.h (tests/test_tta_cpu.py item 2), per geometry and source kind, over flips 0 / 2 / 3 with and without ReOrg:
the worst |value - float64 bilinear| over its bound (half an fp16 ulp + 8 x 2^-24), the worst distance from fp16(torch's scale_img) in fp16 ulps, and the share of
resampled cells that differ from fp16(torch's scale_img) at all -- reported, not asserted: torch's association and contraction belong to the torch build.  CPU only.
    python scripts/tta_margins.py      # prints the table of profiles/tta_margins.txt"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import tta_ref as tr
from tests._hostsim import tta as host
from tests.test_tta_cpu import FP32_SLACK, torch_scale_pad

print("%-34s %-4s %12s %14s %16s" % ("geometry (source-to-resampled-in-padded)", "src", "err / bound", "ulps from torch", "cells != torch"))
for geom, gid in zip(tr.GEOMS, tr.GEOM_IDS):
    (H, W), (hs, ws), (Hp, Wp) = geom
    for kind in ("f32", "u8"):
        img = tr.source_image(kind, 2, H, W, seed=7)
        worst, ulps, diff, cells = 0.0, 0.0, 0, 0
        for flip in (0, 2, 3):
            v64 = np.full((2, 3, Hp, Wp), float(host.pad_value()), np.float64)
            v64[:, :, :hs, :ws] = tr.bilinear64(img, flip, hs, ws)
            t32 = torch_scale_pad(img, flip, hs, ws, Hp, Wp)
            for reorg in (0, 1):
                got = host.scale_layout(img, flip, hs, ws, Hp, Wp, reorg)
                live = ~tr.pad_mask(hs, ws, Hp, Wp, reorg) & ~tr.zero_mask(Hp, Wp, reorg)
                g, want = got[:, live].astype(np.float64), tr.layout_ref(v64, reorg)[:, live]
                ref16 = tr.layout_ref(t32, reorg)[:, live].astype(np.float16).astype(np.float64)
                worst = max(worst, float((np.abs(g - want) / (0.5 * tr.ulp_f16(want) + FP32_SLACK)).max()))
                ulps = max(ulps, float((np.abs(g - ref16) / tr.ulp_f16(np.maximum(np.abs(g), np.abs(ref16)))).max()))
                diff += int((g != ref16).sum())
                cells += g.size
        print("%-34s %-4s %12.3f %14.1f %9d of %-9d = %.3f %%" % (gid, kind, worst, ulps, diff, cells, 100.0 * diff / cells))
