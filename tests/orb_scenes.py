"""tests/orb_scenes.py -- the fixtures of the feature-based camera-motion tests: the smallest planes at which each mechanism of the estimator can break (a plane must
exceed 62 pixels each way, or ORB's border rule leaves nothing), their NumPy references (tests/orb_np.py), computed once and shared, and the figures measured on
the RESTATEMENT alone: the counts of good matches and inliers every ordinary fixture has, and the distance of the restatement's warp from the planted one."""
import functools

import numpy as np

from tests import orb_np

MOTION = (0.01, 1.7, -2.3)      # the planted step: theta (rad), tx, ty (full-resolution pixels)
TURN = (0.12, -3.1, 2.2)        # ... and the larger rotation

# name: frame (H, W), downscale, scene seed, planted step, detections (tlbr, conf, class; full-resolution pixels) or None, max_keypoints[, scene arguments]
FIXTURES = {
    "ragged": ((191, 253), 2, 12, MOTION, None, 8192),                  # odd sides, plane 126 x 95: ragged FAST / smoothing tiles
    "full": ((96, 128), 1, 30, MOTION, None, 8192, dict(per_kilopixel=30.0, sides=(4.0, 12.0))),      # downscale 1: no resize; a denser scene for the 66 x 34 interior
    "wide": ((300, 520), 2, 13, MOTION, None, 8192),                     # plane 260 x 150: five FAST tiles across, more keypoints than one matching tile (256) and one wave
    "boxes": ((300, 520), 2, 13, MOTION, "BOXES", 8192),                 # detection boxes masked out, one with negative corners (a Python slice from the far end)
    "capped": ((300, 520), 2, 13, MOTION, None, 150),                    # capacity below the corner count: the first 150 in row-major order, `truncated` set
    "turned": ((300, 520), 2, 14, TURN, None, 8192),
}
BOXES = np.array([[150.0, 90.0, 260.5, 170.0, 0.9, 0.0], [-40.0, 120.0, 130.0, 200.0, 0.8, 1.0], [300.0, -50.0, 420.0, 131.9, 0.7, 0.0],
                  [433.0, 160.0, 470.0, 220.0, 0.6, 2.0]], np.float32)
ORDINARY = ["ragged", "full", "wide", "boxes", "turned"]

# measured on the restatement (python -m tests.orb_scenes prints them): {name: (keypoints of frame 0, of frame 1, good matches, inliers)}
COUNTS = {
    "ragged": (49, 47, 38, 36),
    "full": (53, 55, 41, 39),
    "wide": (344, 341, 257, 256),
    "boxes": (282, 280, 209, 208),
    "capped": (150, 150, 116, 115),      # (of 344 and 341 corners)
    "turned": (368, 354, 219, 216),
}
# |restatement's warp - planted warp|: (largest difference of the four rotation entries, of the two translations in full-resolution pixels).  The error belongs to the
# algorithm -- integer keypoints on point-sampled edges, half-resolution pixels doubled -- not to the device; tests assert twice these figures
TRUTH_ERR = {
    "ragged": (0.01865, 2.566),          # (a 64 x 33 interior far from the origin: the rotation is poorly constrained and the translation extrapolates it)
    "full": (0.002775, 0.1920),
    "wide": (0.0005395, 0.2028),
    "boxes": (0.0003005, 0.2290),
    "capped": (0.0006652, 0.1880),
    "turned": (0.001093, 0.4370),
}


def dets(name):
    return BOXES if FIXTURES[name][4] == "BOXES" else None


@functools.lru_cache(maxsize=None)
def frames(name):
    from yolov7_tracker_amd import synth
    size, _, seed, step = FIXTURES[name][:4]
    f, warps = synth.make_corner_frames(2, size, seed, steps=[step], **(FIXTURES[name][6] if len(FIXTURES[name]) > 6 else {}))
    f.setflags(write=False)
    return f, warps[1]


@functools.lru_cache(maxsize=None)
def extracted(name):
    """the restatement's two extractions"""
    ds, cap = FIXTURES[name][1], FIXTURES[name][5]
    return tuple(orb_np.extract(f, ds, dets(name), cap) for f in frames(name)[0])


@functools.lru_cache(maxsize=None)
def estimated(name):
    a, b = extracted(name)
    return orb_np.estimate(a, b, FIXTURES[name][1])


def truth_error(name, warp6):
    d = np.abs(np.asarray(warp6, np.float64).reshape(2, 3) - frames(name)[1])
    return float(d[:, :2].max()), float(d[:, 2].max())


@functools.lru_cache(maxsize=None)
def sequence(n=4):
    """a short moving-camera sequence with detections for the estimator inside the trackers: frames (n, 288, 384, 3), planted warps, detections"""
    from yolov7_tracker_amd import synth
    f, planted = synth.make_corner_frames(n, (288, 384), 4, rot=0.006, shift=2.0)
    return f, planted, synth.make_detections(n, 16, 288, seq_idx=4)


if __name__ == "__main__":
    for name in FIXTURES:
        a, b = extracted(name)
        e = estimated(name)
        print('    "%s": (%d, %d, %d, %d),' % (name, len(a["kp"]), len(b["kp"]), int(e["status"][2]), int(e["status"][3])),
              "# flag %d total %d/%d truth error %s" % (int(e["status"][4]), a["total"], b["total"], truth_error(name, e["warp"])))
