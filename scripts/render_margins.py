"""CPU: how far the NumPy restatement of the JPEG encoder (tests/render_np.py) falls short of Pillow's encoder (libjpeg) at the same quality and subsampling, in PSNR
and in file size, over the scenes and shapes of tests/render_scenes.py -> profiles/render_margins.txt.  tests/test_render_cpu.py allows the host build TWICE the
largest shortfall recorded here (two correct encoders differ by their rounding); the device is compared with the host build byte for byte.

    python scripts/render_margins.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import render_np as rn, render_scenes as rs      # noqa: E402


def main():
    lines, worst_db, worst_bytes = [], 0.0, 0.0
    for sub in rs.SUBSAMPLINGS:
        for W, H in rs.shapes(sub):
            for name in rs.SCENES:
                frame = rs.scene(name, W, H)
                for q in rs.QUALITIES:
                    ours, theirs, n_ours, n_theirs = rn.against_pillow(frame, rn.encode(frame, q, sub), q, sub)
                    short, extra = theirs - ours, (n_ours - n_theirs) / n_theirs
                    worst_db, worst_bytes = max(worst_db, short), max(worst_bytes, extra)
                    lines.append("%-10s %4dx%-4d %s q%-3d  PSNR ours %7.3f dB  Pillow %7.3f dB  short %+7.3f dB   bytes ours %7d  Pillow %7d  extra %+7.4f"
                                 % (name, W, H, sub, q, ours, theirs, short, n_ours, n_theirs, extra))
    head = ["JPEG: the NumPy restatement against Pillow's encoder, both decoded by Pillow, PSNR against the source frame (the MSE floored at 1e-3)",
            "largest PSNR shortfall %.4f dB  -> margin of tests/test_render_cpu.py (twice that): %.4f dB" % (worst_db, 2 * worst_db),
            "largest relative size excess %.5f -> margin (twice that): %.5f   (ours carries DRI and one RSTm per MCU row: small files are mostly header)" % (worst_bytes, 2 * worst_bytes), ""]
    out = os.path.join(ROOT, "profiles", "render_margins.txt")
    open(out, "w").write("\n".join(head + lines) + "\n")
    print("\n".join(head[:3]))


if __name__ == "__main__":
    main()
