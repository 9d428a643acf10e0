"""AFLink on the device: the appearance-free link model of StrongSORT++ (the reference ships its network, tracker/reid_models/AFLink.py: class PostLinker, and
leaves `use_AFLink` a TODO).  After a sequence, tracklets that a missed detection or an occlusion split into two ids are joined again from their result rows
(frame, id, x, y) alone, so it applies to every tracker.

The device does the pairs (include/y7t.h: y7t_aflink_candidates -- gate, compaction, pair transform and the network over every candidate, csrc/y7t_aflink.hip); the
assignment over the few surviving rows and columns stays on the host (scipy.optimize.linear_sum_assignment).  The linking procedure is this project's restatement
of the StrongSORT release's (DESIGN.md section 4 "AFLink"; tests/aflink_np.py); no trained AFLink_epoch20.pth ships with the reference, so `random:aflink[:seed[:gain]]`
gives the seeded weights of synth.make_aflink_weights.

    python -m yolov7_tracker_amd.tracker.aflink --input results.txt --output linked.txt --aflink random:aflink:0:1.5
"""
import argparse
import ctypes
import weakref

import numpy as np
import torch

from .. import _lib, synth

OVERFLOW = 1      # Y7T_AFL_OVERFLOW


def load_aflink_weights(path):
    """a file torch.load opens whose keys are PostLinker's, or random:aflink[:seed[:gain]] -> {name: float32 numpy array} in state_dict() order"""
    shapes = synth.aflink_tensor_shapes()
    if isinstance(path, str) and path.startswith("random"):
        parts = path.split(":")
        if len(parts) < 2 or parts[1] != "aflink" or len(parts) > 4:
            raise ValueError("aflink %r: random:aflink[:seed[:gain]]" % (path,))
        seed = int(parts[2]) if len(parts) > 2 and parts[2] else 0
        gain = float(parts[3]) if len(parts) > 3 and parts[3] else 1.5
        return synth.make_aflink_weights(seed, gain)
    sd = torch.load(path, map_location="cpu")
    if hasattr(sd, "state_dict"):
        sd = sd.state_dict()
    if not isinstance(sd, dict):
        raise ValueError("aflink %r does not hold a state dict" % (path,))
    sd = {k[7:] if k.startswith("module.") else k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    missing = [n for n, _ in shapes if n not in sd]
    extra = [k for k in sd if k not in dict(shapes)]
    if missing or extra:
        raise ValueError("aflink %r is not a PostLinker state dict: missing %s, unexpected %s" % (path, missing[:4], extra[:4]))
    out = {}
    for name, shape in shapes:
        a = torch.as_tensor(sd[name]).detach().cpu().to(torch.float32).numpy()
        if tuple(a.shape) != tuple(shape):
            raise ValueError("aflink %r: %s has shape %s, expected %s" % (path, name, tuple(a.shape), tuple(shape)))
        out[name] = np.ascontiguousarray(a)
    return out


def pack_aflink_weights(weights):
    """the 74 float tensors -> one float32 vector in state_dict() order (what y7t_aflink_init takes)"""
    return np.concatenate([np.asarray(weights[n], np.float32).reshape(-1) for n, _ in synth.aflink_tensor_shapes()])


class DeviceAFLink:
    """The network and the candidate stage on the device, for tables of up to max_tracklets tracklets / max_rows rows and up to max_pairs candidate pairs."""

    def __init__(self, weights, max_tracklets=4096, max_rows=1 << 20, max_pairs=1 << 16):
        _lib.require_gpu()
        self._L = _lib.load()
        self.max_tracklets, self.max_rows, self.max_pairs = int(max_tracklets), int(max_rows), int(max_pairs)
        ws = int(self._L.y7t_aflink_workspace_bytes(self.max_tracklets, self.max_rows, self.max_pairs))
        if ws == 0:
            raise ValueError("AFLink capacities out of range: %d tracklets, %d rows, %d pairs" % (self.max_tracklets, self.max_rows, self.max_pairs))
        nbytes = int(self._L.y7t_aflink_weight_bytes()) + ws
        packed = pack_aflink_weights(weights)
        if packed.size != int(self._L.y7t_aflink_num_weights()):
            raise ValueError("%d weights, the network has %d" % (packed.size, int(self._L.y7t_aflink_num_weights())))
        self._blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        weakref.finalize(self._blob, DeviceAFLink._release, self._L, int(self._blob.data_ptr()))
        _lib.check(self._L.y7t_aflink_init(_lib.ptr(self._blob), nbytes, packed.ctypes.data, self.max_tracklets, self.max_rows, self.max_pairs, _lib.stream_ptr()))
        self._pairs = torch.zeros((self.max_pairs, 2), dtype=torch.int32, device="cuda")
        self._scores = torch.zeros(self.max_pairs, dtype=torch.float32, device="cuda")
        self._head = torch.zeros(2, dtype=torch.int32, device="cuda")      # count, status
        self._blocks = None

    @staticmethod
    def _release(L, address):
        try:
            L.y7t_aflink_release(address)
        except Exception:
            pass

    @property
    def ptr(self):
        return _lib.ptr(self._blob)

    def score_pairs(self, x1, x2):
        """x1, x2 (P, 30, 3) float32 (numpy or tensor) -> (P,) float32 device tensor of link scores"""
        a = torch.as_tensor(x1).to(device="cuda", dtype=torch.float32).contiguous()
        b = torch.as_tensor(x2).to(device="cuda", dtype=torch.float32).contiguous()
        if a.shape != b.shape or a.dim() != 3 or tuple(a.shape[1:]) != (30, 3):
            raise ValueError("x1, x2 must both be (P, 30, 3): %s, %s" % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty(a.shape[0], dtype=torch.float32, device="cuda")
        _lib.check(self._L.y7t_aflink_score_pairs_f32(self.ptr, _lib.ptr(a), _lib.ptr(b), int(a.shape[0]), _lib.ptr(out), _lib.stream_ptr()))
        return out

    def candidates(self, table, offsets, thrT=(0, 30), thrS=75, blocks=False):
        """table (R, 3) float64 [frame, x, y], the tracklets' runs one after the other; offsets (N + 1,) -> dict(count, status, pairs (n, 2), scores (n,), and with
        blocks=True x1, x2 (n, 30, 3)) as NumPy arrays, n = min(count, max_pairs).  status & OVERFLOW: more candidates than max_pairs -- the list is not whole."""
        table = np.ascontiguousarray(table, np.float64).reshape(-1, 3)
        offsets = np.ascontiguousarray(offsets, np.int32)
        n = len(offsets) - 1
        if n > self.max_tracklets or len(table) > self.max_rows:
            raise _lib.Y7TError("AFLink: %d tracklets / %d rows exceed this object's capacity (%d / %d)" % (n, len(table), self.max_tracklets, self.max_rows))
        if len(table) != int(offsets[-1]) or np.any(np.diff(offsets) < 0) or offsets[0] != 0:
            raise ValueError("offsets do not describe the table")
        t = torch.from_numpy(table).cuda()
        o = torch.from_numpy(offsets).cuda()
        x1 = x2 = None
        if blocks:
            if self._blocks is None:
                self._blocks = torch.zeros((2, self.max_pairs, 30, 3), dtype=torch.float32, device="cuda")
            x1, x2 = self._blocks[0], self._blocks[1]
        _lib.check(self._L.y7t_aflink_candidates(self.ptr, _lib.ptr(t) if len(table) else None, _lib.ptr(o), n, float(thrT[0]), float(thrT[1]), float(thrS), _lib.ptr(self._pairs),
                                                 _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(self._scores), _lib.ptr(self._head), ctypes.c_void_p(self._head.data_ptr() + 4), _lib.stream_ptr()))
        count, status = (int(v) for v in self._head.cpu())      # (the one read-back, after the last launch)
        m = min(count, self.max_pairs)
        out = dict(count=count, status=status, pairs=self._pairs[:m].cpu().numpy(), scores=self._scores[:m].cpu().numpy())
        if blocks:
            out["x1"], out["x2"] = x1[:m].cpu().numpy(), x2[:m].cpu().numpy()
        return out


def build_tracklets(rows):
    """rows (R, >= 4) [frame, id, x, y, ...] sorted by frame -> (ids in order of first appearance, table (R, 3) [frame, x, y] tracklet by tracklet, offsets (N + 1,))"""
    ids, members = [], {}
    for k, i in enumerate(rows[:, 1].tolist()):
        if i not in members:
            members[i] = []
            ids.append(i)
        members[i].append(k)
    order = [k for i in ids for k in members[i]]
    table = rows[order][:, [0, 2, 3]] if len(order) else np.zeros((0, 3))
    offsets = np.zeros(len(ids) + 1, np.int32)
    offsets[1:] = np.cumsum([len(members[i]) for i in ids])
    return ids, np.ascontiguousarray(table, np.float64), offsets


def link_decisions(n, pairs, scores, thrP):
    """steps 4-8 of AFLink.link: the candidates' float32 scores -> [(row tracklet, column tracklet)] of the accepted links, in ascending row order"""
    from scipy.optimize import linear_sum_assignment
    thrP = float(thrP)
    cost = (np.float32(1) - np.asarray(scores, np.float32)).astype(np.float64)
    mat = np.full((n, n), 1e5, np.float64)
    keep = cost <= thrP
    mat[pairs[keep, 0], pairs[keep, 1]] = cost[keep]
    if n == 0:
        return []
    rsel, csel = np.nonzero(mat.min(1) < thrP)[0], np.nonzero(mat.min(0) < thrP)[0]
    if len(rsel) == 0 or len(csel) == 0:
        return []
    sub = mat[rsel][:, csel]
    ri, ci = linear_sum_assignment(sub)
    return [(int(rsel[r]), int(csel[c])) for r, c in zip(ri, ci) if sub[r, c] < thrP]


def relabel(rows, ids, links):
    """steps 8-12: the accepted links -> the relabelled rows, later duplicates of a (frame, id) dropped, sorted by (frame, id)"""
    id2id = {}
    for r, c in links:
        id2id[ids[r]] = ids[c]
    ID2ID = {}
    for k, v in id2id.items():      # (literally the release's chain resolution)
        ID2ID[v] = ID2ID[k] if k in ID2ID else k
    out = rows.copy()
    for k, v in ID2ID.items():
        out[out[:, 1] == k, 1] = v
    if len(out) == 0:
        return out
    _, index = np.unique(out[:, :2], return_index=True, axis=0)
    return out[index]


class AFLink:
    """AFLink(model, thrT, thrS, thrP).link(rows): model is a DeviceAFLink; thrT the admitted frame gap [thrT[0], thrT[1]), thrS the largest distance between the
    former's last and the latter's first position, thrP the cost 1 - score below which a pair is linked."""

    def __init__(self, model, thrT=(0, 30), thrS=75, thrP=0.05):
        self.model, self.thrT, self.thrS, self.thrP = model, (float(thrT[0]), float(thrT[1])), float(thrS), float(thrP)

    def link(self, rows):
        """(R, >= 6) float64 [frame, id, x, y, w, h, ...] -> the linked rows, sorted by (frame, id)"""
        rows = np.asarray(rows, np.float64)
        if rows.ndim != 2 or rows.shape[1] < 6:
            raise ValueError("rows must be (R, >= 6): [frame, id, x, y, w, h, ...]")
        rows = rows[np.argsort(rows[:, 0], kind="stable")]
        ids, table, offsets = build_tracklets(rows)
        res = self.model.candidates(table, offsets, self.thrT, self.thrS)
        if res["status"] & OVERFLOW:
            raise _lib.Y7TError("AFLink: %d candidate pairs exceed max_pairs = %d of this DeviceAFLink; nothing was linked" % (res["count"], self.model.max_pairs))
        self.last = res
        return relabel(rows, ids, link_decisions(len(ids), res["pairs"], res["scores"], self.thrP))


def results_rows(results):
    """track.py's per-frame results [(frame, ids, tlwhs, clses)] -> (R, 7) float64 [frame, id, x, y, w, h, cls], the box values as their %.2f text reads back"""
    rows = [[float(frame), float(i)] + [float("%.2f" % v) for v in tlwh[:4]] + [float(c)] for frame, ids, tlwhs, clses in results for i, tlwh, c in zip(ids, tlwhs, clses)]
    return np.array(rows, np.float64).reshape(-1, 7)


def link_results(weights, results, thrT=(0, 30), thrS=75, thrP=0.05, max_pairs=1 << 16):
    """link exactly the rows track.py would write for a sequence -> results in the same form, one entry per frame that still has rows"""
    rows = results_rows(results)
    if len(rows) == 0:
        return results
    model = DeviceAFLink(weights, len(set(rows[:, 1].tolist())), len(rows), max_pairs)
    linked = AFLink(model, thrT, thrS, thrP).link(rows)
    out = []
    for r in linked:
        if not out or out[-1][0] != int(r[0]):
            out.append((int(r[0]), [], [], []))
        out[-1][1].append(int(r[1])); out[-1][2].append(r[2:6]); out[-1][3].append(r[6])
    return out


def read_results(path):
    """a results file `frame,id,x,y,w,h,...` -> (rows (R, 7) float64 with the line number in column 6, the text after the sixth field of each line)"""
    rows, tails = [], []
    with open(path) as f:
        for line in f:
            parts = line.strip().split(",")
            if len(parts) < 6:
                continue
            rows.append([float(v) for v in parts[:6]] + [float(len(tails))])
            tails.append(",".join(parts[6:]))
    return np.array(rows, np.float64).reshape(-1, 7), tails


def write_results(path, rows, tails):
    with open(path, "w") as f:
        for r in rows:
            tail = tails[int(r[6])]
            f.write("%d,%d,%.2f,%.2f,%.2f,%.2f%s\n" % (int(r[0]), int(r[1]), r[2], r[3], r[4], r[5], "," + tail if tail else ""))


def main(argv=None):
    ap = argparse.ArgumentParser(description="link the fragmented tracklets of a results file (frame,id,x,y,w,h,...) with AFLink")
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--aflink", required=True, help="a PostLinker state dict file, or random:aflink[:seed[:gain]]")
    ap.add_argument("--thrT", type=float, nargs=2, default=(0, 30))
    ap.add_argument("--thrS", type=float, default=75)
    ap.add_argument("--thrP", type=float, default=0.05)
    ap.add_argument("--max_pairs", type=int, default=1 << 16)
    o = ap.parse_args(argv)
    rows, tails = read_results(o.input)
    n_ids = len(set(rows[:, 1].tolist()))
    model = DeviceAFLink(load_aflink_weights(o.aflink), max(1, n_ids), max(1, len(rows)), o.max_pairs)
    linked = AFLink(model, o.thrT, o.thrS, o.thrP).link(rows)
    write_results(o.output, linked, tails)
    print("AFLink: %d rows, %d ids -> %d rows, %d ids" % (len(rows), n_ids, len(linked), len(set(linked[:, 1].tolist()))))


if __name__ == "__main__":
    main()
