"""Records tests/golden/gsi_<scene>.npz from the seeded tables of tests/gsi_scenes.py.  Needs mpmath and scikit-learn (the tests need neither).

    python tests/golden/make_golden_gsi.py

Per scene: rows_in, tau, interval; the ordered runs (runs_in, offsets_in, ids); the interpolated rows (runs, offsets, src) of tests/gsi_np.py; len_scale; and the
smoothed columns three times:
  exact    step 3 solved with 50 digits (mpmath): K from the float64 frames and length scale, A = K + 1e-10 I, Cholesky, K a
  cols_np  the NumPy + LAPACK float64 restatement (tests/gsi_np.py)
  cols_sk  scikit-learn's own GaussianProcessRegressor(RBF(len_scale, 'fixed')).fit(t, y).predict(t), one column at a time: the restatement is the release's regressor
E = the largest |cols_np - exact| over ALL scenes (the same number in every file); rows_out = gsi_np.apply(rows_in)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import gsi_np, gsi_scenes as sc      # noqa: E402


def exact_track(t, Y, ls, reg=gsi_np.REG):
    import mpmath as mp
    mp.mp.dps = 50
    n = len(t)
    tt, l, r = [mp.mpf(float(v)) for v in t], mp.mpf(float(ls)), mp.mpf(float(reg))
    K = [[mp.exp(-((tt[i] - tt[j]) / l) ** 2 / 2) for j in range(n)] for i in range(n)]
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        d = K[j][j] + r - mp.fsum(L[j][k] * L[j][k] for k in range(j))
        assert d > 0
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i][j] = (K[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    out = np.empty((n, 4))
    for c in range(4):
        z = [mp.mpf(0)] * n
        for i in range(n):
            z[i] = (mp.mpf(float(Y[i, c])) - mp.fsum(L[i][k] * z[k] for k in range(i))) / L[i][i]
        a = [mp.mpf(0)] * n
        for i in range(n - 1, -1, -1):
            a[i] = (z[i] - mp.fsum(L[k][i] * a[k] for k in range(i + 1, n))) / L[i][i]
        for i in range(n):
            out[i, c] = float(mp.fsum(K[i][j] * a[j] for j in range(n)))
    return out


def sklearn_track(t, Y, ls):
    from sklearn.gaussian_process import GaussianProcessRegressor as GPR
    from sklearn.gaussian_process.kernels import RBF
    t = np.asarray(t, np.float64).reshape(-1, 1)
    return np.column_stack([GPR(RBF(float(ls), "fixed")).fit(t, Y[:, c].reshape(-1, 1)).predict(t).reshape(-1) for c in range(4)])


def main():
    recs = {}
    for name in sc.SCENES:
        rows_in, tau = sc.scene_rows(name)
        rows, ids, off_in = gsi_np.order(rows_in)
        runs_in = np.ascontiguousarray(rows[:, [0, 2, 3, 4, 5]])
        runs, off, src = gsi_np.interpolate(runs_in, off_in, sc.INTERVAL)
        ls = gsi_np.len_scale(np.diff(off), tau)
        exact, cols_np, cols_sk = (np.empty((len(runs), 4)) for _ in range(3))
        for k in range(len(ids)):
            lo, hi = int(off[k]), int(off[k + 1])
            t, Y = runs[lo:hi, 0], runs[lo:hi, 1:]
            exact[lo:hi] = exact_track(t, Y, ls[k])
            cols_np[lo:hi] = gsi_np.smooth_track(t, Y, float(ls[k]))
            cols_sk[lo:hi] = sklearn_track(t, Y, ls[k])
            print("%s id %d: %d rows, len_scale %.4g, shift %.3g px, |np - exact| %.3g, |sk - exact| %.3g" % (
                name, int(ids[k]), hi - lo, ls[k], np.abs(exact[lo:hi] - Y).max(), np.abs(cols_np[lo:hi] - exact[lo:hi]).max(), np.abs(cols_sk[lo:hi] - exact[lo:hi]).max()), flush=True)
        recs[name] = dict(rows_in=rows_in, tau=np.float64(tau), interval=np.int32(sc.INTERVAL), ids=ids, runs_in=runs_in, offsets_in=off_in, runs=runs, offsets=off, src=src,
                          len_scale=ls, exact=exact, cols_np=cols_np, cols_sk=cols_sk, rows_out=gsi_np.apply(rows_in, sc.INTERVAL, tau))
    E = max(float(np.abs(r["cols_np"] - r["exact"]).max()) for r in recs.values())
    print("E = %.4g" % E)
    for name, r in recs.items():
        np.savez_compressed(os.path.join(sc.GOLDEN, "gsi_%s.npz" % name), E=np.float64(E), **r)


if __name__ == "__main__":
    main()
