"""tests/gsi_scenes.py -- TEST INFRASTRUCTURE: what the GSI tests share -- the seeded track tables the fixtures were recorded from (tests/golden/make_golden_gsi.py)
and the recorded fixtures themselves.

A scene is a rows table [frame, id, x, y, w, h, cls] with a tau.  Track lengths are stated AFTER interpolation:
  t10    tau 10: 1, 2, 15, 16, 17, 31, 33, 64, 65, 128 and 129 (either side of the LDS / HBM switch), 131 (with gaps of 20 and 21 that stay open, so its frames
         are not equally spaced) and 300 rows
  t6p5   tau 6.5: a 300-row track at the 1 / tau clip (tau**3 = 274.6 < 300) beside a 40-row one
  t2     tau 2: a 1-row track at the tau**2 clip, a 3-row one between the clips, a 20-row one at 1 / tau
Non-contiguous ids, rows shuffled, one duplicated (frame, id) placed behind its original (it must be dropped), frame steps of 1, 2, 3 and 19 (filled), 20 and 21
(left open), jitter of 1.5 px on a smooth path, so that smoothing moves values by pixels."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INTERVAL = 20
SCENES = {"t10": (10.0, (1, 2, 15, 16, 17, 31, 33, 64, 65, 128, 129, 131, 300)), "t6p5": (6.5, (300, 40)), "t2": (2.0, (1, 3, 20))}
STEPS = (1, 1, 2, 1, 19, 1, 1, 3, 1, 1, 1, 2, 1, 1, 1, 1)
_cache = {}


def _frames(first, length, open_gaps):
    """frames from `first` on whose track has `length` rows once every step below 20 is filled; open_gaps: after how many rows a gap of 20, then 21, is left open"""
    f, out, rows, k = first, [first], 1, 0
    opened = list(open_gaps)
    gap = 20
    while rows < length:
        if opened and rows >= opened[0]:
            opened.pop(0)
            f += gap
            gap += 1
            rows += 1
        else:
            step = min(STEPS[k % len(STEPS)], length - rows)
            k += 1
            f += step
            rows += step
        out.append(f)
    return np.array(out, np.float64)


def scene_rows(name):
    """-> (rows (R, 7) float64 as a tracker would have written them: shuffled, with the duplicate; tau)"""
    tau, lengths = SCENES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    rows = []
    for k, length in enumerate(lengths):
        tid = 3 + 7 * k + (k % 3)
        f = _frames(2 + 5 * k, length, (50, 90) if length == 131 else ())
        x = 200.0 + 40.0 * k + 1.2 * (f - f[0]) + 25.0 * np.sin(f / 23.0)
        y = 150.0 + 15.0 * k - 0.6 * (f - f[0]) + 18.0 * np.cos(f / 31.0)
        box = np.column_stack([x, y, 40.0 + 0.02 * (f - f[0]), 90.0 + 0.03 * (f - f[0])]) + rng.normal(0.0, 1.5, (len(f), 4))
        rows.append(np.column_stack([f, np.full(len(f), float(tid)), box, (f + k) % 3]))
    rows = np.concatenate(rows, 0)
    rows = rows[rng.permutation(len(rows))]
    dup = rows[len(rows) // 2].copy()
    dup[2:6] += 100.0
    dup[6] = 9.0
    return np.concatenate([rows, dup[None]], 0), tau


def goldens():
    """-> {name: arrays} of every recorded scene"""
    if "g" not in _cache:
        paths = sorted(glob.glob(os.path.join(GOLDEN, "gsi_*.npz")))
        _cache["g"] = {os.path.basename(p)[len("gsi_"):-4]: dict(np.load(p)) for p in paths}
    return _cache["g"]


def bound():
    """(E, 4 E): E = the largest |NumPy float64 - exact| over the whole recorded set"""
    E = max(float(g["E"]) for g in goldens().values())
    return E, 4 * E
