"""Records tests/golden/np_norms.npz: what numpy itself returns for the two norms DeepSORT's and StrongSORT's appearance arithmetic restates
(csrc/y7t_track_deepsort.h: y7t_np_pairwise_sumsq, y7t_blas_sdot_self), bit for bit, on seeded vectors.

    python tests/golden/make_golden_np_norms.py

For each width in WIDTHS: 64 float32 vectors normal(0, 1) * uniform(0.1, 5) (`x_<width>`, (64, width)), the uint32 bit patterns of
np.linalg.norm(x[None], axis=1)[0] (`rows_<width>`: the row norm of cal_cosine_distance, add.reduce's pairwise sum) and of np.linalg.norm(x)
(`vec_<width>`: the 1-D norm of STrack.update, sqrt(sdot(x, x))).  `numpy_version` says which numpy wrote them; the BLAS is the one its wheel ships."""
import os

import numpy as np

WIDTHS = (1, 2, 3, 7, 8, 31, 32, 33, 64, 96, 100, 128, 160, 200, 256, 384, 512, 1024)
N_VEC = 64
SEED = 20261019


def vectors(width):
    rng = np.random.default_rng(SEED + width)
    return (rng.normal(0, 1, (N_VEC, width)) * rng.uniform(0.1, 5, (N_VEC, 1))).astype(np.float32)


def record():
    out = {"numpy_version": np.array(np.__version__), "widths": np.array(WIDTHS, np.int32)}
    for w in WIDTHS:
        x = vectors(w)
        rows = np.array([np.linalg.norm(v[None], axis=1)[0] for v in x])
        vec = np.array([np.linalg.norm(v) for v in x])
        assert rows.dtype == np.float32 and vec.dtype == np.float32
        out["x_%d" % w], out["rows_%d" % w], out["vec_%d" % w] = x, rows.view(np.uint32), vec.view(np.uint32)
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "np_norms.npz")
    np.savez_compressed(path, **record())
    print(path, os.path.getsize(path), "bytes")
