"""GSI on the device: the Gaussian-smoothed interpolation of StrongSORT++ (the reference ships no GSI code: `use_GSI` is never read in tracker/strongsort.py).
After a sequence, the short gaps a missed detection leaves in a track are filled linearly and every track is smoothed by a Gaussian-process regression over its
frames, from the result rows (frame, id, x, y, w, h) alone, so it applies to every tracker; with AFLink (tracker/aflink.py) in front of it this is StrongSORT++'s
pair of steps after a sequence.

The device does the rows (include/y7t.h: y7t_gsi_interpolate, y7t_gsi_smooth; csrc/y7t_gsi.hip): one launch group fills the gaps, one workgroup per track then
solves that track's own dense system in float64.  The host orders the table, computes one length scale per track and puts the rows back together.  The procedure
is this project's restatement of the StrongSORT release's GSI.py (DESIGN.md section 4 "GSI"; tests/gsi_np.py).

    python -m yolov7_tracker_amd.tracker.gsi --input results.txt --output smoothed.txt [--interval 20 --tau 10]
"""
import argparse
import ctypes
import weakref

import numpy as np

from .. import _lib
from .aflink import read_results, results_rows, write_results

REG = 1e-10                                  # GaussianProcessRegressor's default alpha
ROWS_OVERFLOW, LEN_OVERFLOW = 1, 2           # Y7T_GSI_ROWS_OVERFLOW, Y7T_GSI_LEN_OVERFLOW
NOT_PD, TOO_LONG, PENDING = 1, 2, 4          # Y7T_GSI_NOT_PD, Y7T_GSI_TOO_LONG, Y7T_GSI_PENDING


class DeviceGSI:
    """The interpolation and the smoother on the device, for tables of up to max_rows rows and tracks of up to max_len rows, both counted after interpolation;
    max_tracks tracks go into one group of launches (a longer table is taken in groups, with the same result)."""

    def __init__(self, max_tracks=4096, max_rows=1 << 20, max_len=4096):
        import torch
        _lib.require_gpu()
        self._L = _lib.load()
        self.max_tracks, self.max_rows, self.max_len = int(max_tracks), int(max_rows), int(max_len)
        nbytes = int(self._L.y7t_gsi_workspace_bytes(self.max_tracks, self.max_rows, self.max_len))
        if nbytes == 0:
            raise ValueError("GSI capacities out of range: %d tracks, %d rows, %d rows a track" % (self.max_tracks, self.max_rows, self.max_len))
        self._blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        weakref.finalize(self._blob, DeviceGSI._release, self._L, int(self._blob.data_ptr()))
        _lib.check(self._L.y7t_gsi_init(_lib.ptr(self._blob), nbytes, self.max_tracks, self.max_rows, self.max_len, _lib.stream_ptr()))
        self._runs = torch.zeros((self.max_rows, 5), dtype=torch.float64, device="cuda")
        self._src = torch.zeros(self.max_rows, dtype=torch.int32, device="cuda")
        self._cols = torch.zeros((self.max_rows, 4), dtype=torch.float64, device="cuda")
        self._head = torch.zeros(2, dtype=torch.int32, device="cuda")      # count, status

    @staticmethod
    def _release(L, address):
        try:
            L.y7t_gsi_release(address)
        except Exception:
            pass

    @property
    def ptr(self):
        return _lib.ptr(self._blob)

    @staticmethod
    def _table(runs, offsets):
        import torch
        runs = np.ascontiguousarray(runs, np.float64).reshape(-1, 5)
        offsets = np.ascontiguousarray(offsets, np.int32)
        if len(offsets) < 1 or len(runs) != int(offsets[-1]) or np.any(np.diff(offsets) < 0) or offsets[0] != 0:
            raise ValueError("offsets do not describe the table")
        return runs, offsets, torch.from_numpy(runs).cuda(), torch.from_numpy(offsets).cuda()

    def _interpolate(self, t, o, n, interval):
        import torch
        off2 = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        _lib.check(self._L.y7t_gsi_interpolate(self.ptr, _lib.ptr(t) if t.numel() else None, _lib.ptr(o), n, int(interval), _lib.ptr(self._runs), _lib.ptr(off2), _lib.ptr(self._src),
                                               _lib.ptr(self._head), ctypes.c_void_p(self._head.data_ptr() + 4), _lib.stream_ptr()))
        return off2

    def _smooth(self, t, o, ls, n, longest, reg, cols):
        import torch
        status = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        _lib.check(self._L.y7t_gsi_smooth(self.ptr, _lib.ptr(t) if n else None, _lib.ptr(o), _lib.ptr(ls) if n else None, n, int(longest), float(reg), _lib.ptr(cols) if n else None,
                                          _lib.ptr(status), _lib.stream_ptr()))
        return status

    def interpolate(self, runs, offsets, interval=20):
        """runs (R, 5) float64 [frame, x, y, w, h], the tracks' runs one after the other; offsets (N + 1,) -> dict(runs (m, 5), offsets (N + 1,), src (m,), count,
        status) as NumPy arrays, m = min(count, max_rows).  status & ROWS_OVERFLOW: more rows than max_rows; & LEN_OVERFLOW: a track longer than max_len."""
        runs, offsets, t, o = self._table(runs, offsets)
        off2 = self._interpolate(t, o, len(offsets) - 1, interval)
        count, status = (int(v) for v in self._head.cpu())      # (the one read-back, after the last launch)
        m = min(count, self.max_rows)
        return dict(runs=self._runs[:m].cpu().numpy(), offsets=off2.cpu().numpy(), src=self._src[:m].cpu().numpy(), count=count, status=status)

    def smooth(self, runs, offsets, len_scale, reg=REG, longest=None):
        """-> (the (R, 4) smoothed columns, one status word per track) as NumPy arrays; longest: the rows of the longest track (default: from the offsets)"""
        import torch
        runs, offsets, t, o = self._table(runs, offsets)
        n = len(offsets) - 1
        if len(runs) > self.max_rows:
            raise _lib.Y7TError("GSI: %d rows exceed this object's capacity (%d)" % (len(runs), self.max_rows))
        longest = (int(np.diff(offsets).max()) if n else 0) if longest is None else int(longest)
        ls = torch.from_numpy(np.ascontiguousarray(len_scale, np.float64).reshape(n)).cuda()
        cols = torch.zeros((max(len(runs), 1), 4), dtype=torch.float64, device="cuda")
        status = self._smooth(t, o, ls, n, longest, reg, cols)
        return cols[:len(runs)].cpu().numpy(), status[:n].cpu().numpy()

    def run(self, runs, offsets, len_scale, interval=20, reg=REG, longest=0):
        """both stages back to back, nothing read back in between: the smoother takes the interpolated runs and offsets where the first stage left them.  len_scale
        and longest are the caller's, from the lengths AFTER interpolation (GSI.apply counts them on the host).  -> interpolate()'s dict plus cols (m, 4) and
        track_status (N,)"""
        import torch
        runs, offsets, t, o = self._table(runs, offsets)
        n = len(offsets) - 1
        ls = torch.from_numpy(np.ascontiguousarray(len_scale, np.float64).reshape(n)).cuda()
        off2 = self._interpolate(t, o, n, interval)
        status = self._smooth(self._runs, off2, ls, n, longest, reg, self._cols)
        count, st = (int(v) for v in self._head.cpu())      # (the one read-back, after the last launch)
        m = min(count, self.max_rows)
        return dict(runs=self._runs[:m].cpu().numpy(), offsets=off2.cpu().numpy(), src=self._src[:m].cpu().numpy(), count=count, status=st,
                    cols=self._cols[:m].cpu().numpy(), track_status=status[:n].cpu().numpy())


def order_rows(rows):
    """step 1: stable sort by frame, the first row of every (frame, id) kept (as aflink.relabel keeps it) -> (the rows in (id, frame) order, ascending ids, offsets)"""
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    if len(rows):
        _, index = np.unique(rows[:, :2], return_index=True, axis=0)
        rows = rows[np.sort(index)]
    rows = rows[np.argsort(rows[:, 1], kind="stable")]
    ids, counts = np.unique(rows[:, 1], return_counts=True)
    offsets = np.zeros(len(ids) + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    return rows, ids, offsets


def lengths_after(frames, offsets, interval):
    """rows of every track once its gaps are filled: counted on the host from the frames alone, so that capacity is checked and the length scales are known
    before any launch"""
    n = np.diff(offsets).astype(np.int64)
    if len(frames) == 0:
        return n
    d = np.diff(frames.astype(np.int64))
    fill = np.where((d > 1) & (d < int(interval)), d - 1, 0)
    fill[np.asarray(offsets[1:-1], np.int64) - 1] = 0      # (the step from one track's last row to the next track's first)
    csum = np.concatenate([[0], np.cumsum(fill)])
    lo, hi = np.asarray(offsets[:-1], np.int64), np.asarray(offsets[1:], np.int64)
    return n + np.where(hi > lo, csum[np.maximum(hi - 1, 0)] - csum[np.minimum(lo, len(csum) - 1)], 0)


def length_scales(n, tau):
    """clip(tau * log(tau**3 / n), 1 / tau, tau**2), NumPy float64"""
    tau = float(tau)
    return np.clip(tau * np.log(tau ** 3 / np.asarray(n, np.float64)), tau ** -1, tau ** 2)


class GSI:
    """GSI(model, interval, tau).apply(rows): model is a DeviceGSI; gaps shorter than `interval` frames are filled; tau sets the length scale of the smoother."""

    def __init__(self, model, interval=20, tau=10):
        self.model, self.interval, self.tau = model, int(interval), float(tau)

    def apply(self, rows):
        """(R, >= 6) float64 [frame, id, x, y, w, h, ...] -> every row and the rows of the filled gaps, sorted by (frame, id); x, y, w, h smoothed, every other
        column kept (a new row takes them from the row at the start of its gap)"""
        rows = np.asarray(rows, np.float64)
        if rows.ndim != 2 or rows.shape[1] < 6:
            raise ValueError("rows must be (R, >= 6): [frame, id, x, y, w, h, ...]")
        if len(rows) == 0:
            return rows.copy()
        rows, ids, offsets = order_rows(rows)
        runs = np.ascontiguousarray(rows[:, [0, 2, 3, 4, 5]])
        n_after = lengths_after(runs[:, 0], offsets, self.interval)
        longest = _check_len(ids, n_after, self.model.max_len)
        if int(n_after.sum()) > self.model.max_rows:
            raise _lib.Y7TError("GSI: %d rows after interpolation exceed max_rows = %d of this DeviceGSI; nothing was smoothed" % (int(n_after.sum()), self.model.max_rows))
        res = self.model.run(runs, offsets, length_scales(n_after, self.tau), self.interval, REG, longest)
        if res["status"] or res["count"] != int(n_after.sum()) or not np.array_equal(np.diff(res["offsets"]), n_after):
            raise _lib.Y7TError("GSI: the interpolation reports status %d and %d rows, %d were expected" % (res["status"], res["count"], int(n_after.sum())))
        bad = np.nonzero(res["track_status"])[0]
        if len(bad):
            raise _lib.Y7TError("GSI: track id %d was not smoothed (status %d: 1 = a non-positive pivot, 2 = too long, 4 = not reached)"
                                % (int(ids[bad[0]]), int(res["track_status"][bad[0]])))
        self.last = res
        out = rows[res["src"]].copy()
        out[:, 0] = res["runs"][:, 0]
        out[:, 2:6] = res["cols"]
        return out[np.lexsort((out[:, 1], out[:, 0]))]


def _check_len(ids, n_after, max_len):
    k = int(np.argmax(n_after))
    if n_after[k] > max_len:
        raise _lib.Y7TError("GSI: track id %d has %d rows after interpolation, more than max_len = %d; nothing was smoothed" % (int(ids[k]), int(n_after[k]), max_len))
    return int(n_after[k])


def _model_for(rows, interval, max_len):
    """a DeviceGSI sized for this table: its pool holds slots for the longest track there is, not for max_len"""
    rows, ids, offsets = order_rows(np.asarray(rows, np.float64))
    n_after = lengths_after(rows[:, 0], offsets, interval)
    longest = _check_len(ids, n_after, int(max_len))
    return DeviceGSI(max(1, min(len(ids), 32768)), max(1, int(n_after.sum())), max(1, longest))


def smooth_results(results, interval=20, tau=10, max_len=4096, model=None):
    """interpolate and smooth exactly the rows track.py would write for a sequence -> results in the same form, one entry per frame that has rows.  The rows GSI
    adds are not filtered by min_area again."""
    rows = results_rows(results)
    if len(rows) == 0:
        return results
    out = []
    for r in GSI(model or _model_for(rows, interval, max_len), interval, tau).apply(rows):
        if not out or out[-1][0] != int(r[0]):
            out.append((int(r[0]), [], [], []))
        out[-1][1].append(int(r[1])); out[-1][2].append(r[2:6]); out[-1][3].append(r[6])
    return out


def main(argv=None, model=None):
    ap = argparse.ArgumentParser(description="fill the short gaps of a results file (frame,id,x,y,w,h,...) and smooth every track with GSI")
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--interval", type=int, default=20, help="gaps of fewer than this many frames are filled")
    ap.add_argument("--tau", type=float, default=10, help="the smoother's time constant: length scale = clip(tau * log(tau^3 / rows), 1 / tau, tau^2)")
    ap.add_argument("--max_len", type=int, default=4096, help="the longest track (rows after interpolation) the device object is sized for")
    o = ap.parse_args(argv)
    rows, tails = read_results(o.input)
    out = GSI(model or _model_for(rows, o.interval, o.max_len), o.interval, o.tau).apply(rows) if len(rows) else rows
    write_results(o.output, out, tails)
    print("GSI: %d rows, %d ids -> %d rows" % (len(rows), len(set(rows[:, 1].tolist())), len(out)))


if __name__ == "__main__":
    main()
