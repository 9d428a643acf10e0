"""tests/gsi_np.py -- TEST INFRASTRUCTURE ONLY: the NumPy statement of GSI, the Gaussian-smoothed interpolation of StrongSORT++ (DESIGN.md section 4 "GSI").
The reference ships no GSI code; this restates the StrongSORT release's GSI.py: linear interpolation of gaps shorter than `interval`, then one Gaussian-process
regression per track and column -- scikit-learn's GaussianProcessRegressor(RBF(len_scale, 'fixed')) with its defaults, fitted and predicted on the same frames,
written out as the Cholesky solve it performs (NumPy + LAPACK, float64).  tests/golden/make_golden_gsi.py records scikit-learn's own prediction beside it."""
import numpy as np

REG = 1e-10      # GaussianProcessRegressor's default alpha


def order(rows):
    """step 1: stable sort by frame, the first row of every (frame, id) kept -> the rows in (id, frame) order, the ascending ids, offsets (N + 1,)"""
    rows = np.asarray(rows, np.float64)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    seen, keep = set(), []
    for k, key in enumerate(zip(rows[:, 0].tolist(), rows[:, 1].tolist())):
        if key not in seen:
            seen.add(key)
            keep.append(k)
    rows = rows[keep]
    rows = rows[np.argsort(rows[:, 1], kind="stable")]      # (frames stay ascending inside an id)
    ids, counts = np.unique(rows[:, 1], return_counts=True)
    offsets = np.zeros(len(ids) + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    return rows, ids, offsets


def interpolate(runs, offsets, interval=20):
    """step 2 on the tracks' [frame, x, y, w, h] runs -> (runs with their gaps filled, new offsets, the source row of every output row: a new row's is the row at f0)"""
    runs = np.asarray(runs, np.float64).reshape(-1, 5)
    out, src, new_off = [], [], [0]
    for k in range(len(offsets) - 1):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        for r in range(lo, hi):
            out.append(runs[r].copy())
            src.append(r)
            if r + 1 < hi:
                f0, f1 = int(runs[r, 0]), int(runs[r + 1, 0])
                if f0 + 1 < f1 < f0 + interval:
                    v0, v1 = runs[r, 1:], runs[r + 1, 1:]
                    for f in range(f0 + 1, f1):
                        i = f - f0
                        out.append(np.concatenate([[np.float64(f)], v0 + (v1 - v0) / np.float64(f1 - f0) * np.float64(i)]))
                        src.append(r)
        new_off.append(len(out))
    return np.array(out, np.float64).reshape(-1, 5), np.array(new_off, np.int32), np.array(src, np.int32)


def len_scale(n, tau=10):
    """the length scale of a track of n rows: clip(tau * log(tau**3 / n), 1 / tau, tau**2) -- what the product computes on the host, too"""
    n = np.asarray(n, np.float64)
    return np.clip(tau * np.log(tau ** 3 / n), tau ** -1, tau ** 2)


def kernel(t, ls):
    t = np.asarray(t, np.float64)
    return np.exp(-0.5 * ((t[:, None] - t[None, :]) / ls) ** 2)


def smooth_track(t, Y, ls, reg=REG):
    """step 3: K a with a = (K + reg I)^-1 Y by Cholesky; Y (n, 4)"""
    from scipy.linalg import cho_solve, cholesky
    K = kernel(t, ls)
    L = cholesky(K + reg * np.eye(len(K)), lower=True)
    return K @ cho_solve((L, True), np.asarray(Y, np.float64))


def smooth(runs, offsets, tau=10, reg=REG):
    runs = np.asarray(runs, np.float64).reshape(-1, 5)
    out = np.empty((len(runs), 4))
    for k in range(len(offsets) - 1):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        if hi > lo:
            out[lo:hi] = smooth_track(runs[lo:hi, 0], runs[lo:hi, 1:], float(len_scale(hi - lo, tau)), reg)
    return out


def apply(rows, interval=20, tau=10):
    """the whole procedure on rows [frame, id, x, y, w, h, ...] -> all rows sorted by (frame, id), boxes smoothed, every other column kept (a new row's from f0)"""
    rows = np.asarray(rows, np.float64)
    if len(rows) == 0:
        return rows.copy()
    rows, ids, offsets = order(rows)
    runs, off2, src = interpolate(rows[:, [0, 2, 3, 4, 5]], offsets, interval)
    out = rows[src].copy()
    out[:, 0] = runs[:, 0]
    out[:, 2:6] = smooth(runs, off2, tau)
    return out[np.lexsort((out[:, 1], out[:, 0]))]
