"""tests/aflink_np.py -- TEST INFRASTRUCTURE: the NumPy restatement of AFLink (DESIGN.md section 4 "AFLink"), written independently of the product code.

  forward_packed(blob, x1, x2)          PostLinker.forward (eval) from the PACKED float32 vector y7t_aflink_init takes, in float64 -> scores (P,)
  candidates(table, offsets, ...)       gate, row-major pair list, pair transform -> (pairs (n, 2) int32, x1, x2 (n, 30, 3) float32)
  link(rows, score_fn, ...)             the whole linking procedure; score_fn(pairs, x1, x2) -> float32 scores
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

N_WEIGHTS = 1075266
CHANNELS = ((1, 32), (32, 64), (64, 128), (128, 256))


def _take(blob, pos, shape):
    n = int(np.prod(shape))
    return blob[pos:pos + n].reshape(shape).astype(np.float64), pos + n


def unpack(blob):
    """the packed vector -> (branches, fusions, classifier), walking it in state_dict() order; asserts that it is used up exactly"""
    blob = np.asarray(blob)
    assert blob.dtype == np.float32 and blob.shape == (N_WEIGHTS,)
    pos, branches, fusions = 0, [], []

    def bn(c):
        nonlocal pos
        g, pos = _take(blob, pos, (c,))
        b, pos = _take(blob, pos, (c,))
        mu, pos = _take(blob, pos, (c,))
        var, pos = _take(blob, pos, (c,))
        return g, b, mu, var

    for _ in range(2):
        blocks = []
        for cin, cout in CHANNELS:
            w, pos = _take(blob, pos, (cout, cin, 7))
            blocks.append((w, [bn(cout) for _ in range(3)]))      # bnf, bnx, bny: columns 0, 1, 2
        branches.append(blocks)
    for _ in range(2):
        w, pos = _take(blob, pos, (256, 256, 3))
        fusions.append((w, bn(256)))
    fc1, pos = _take(blob, pos, (128, 512))
    b1, pos = _take(blob, pos, (128,))
    fc2, pos = _take(blob, pos, (2, 128))
    b2, pos = _take(blob, pos, (2,))
    assert pos == N_WEIGHTS
    return branches, fusions, (fc1, b1, fc2, b2)


def _bn(x, p):
    g, b, mu, var = p
    return (x - mu) / np.sqrt(var + 1e-5) * g + b


def forward_packed(blob, x1, x2):
    branches, fusions, (fc1, b1, fc2, b2) = unpack(blob)
    feats = []
    for blocks, (fw, fbn), x in zip(branches, fusions, (x1, x2)):
        h = np.asarray(x, np.float64)[:, None]                                # [P][channel][row][column], as the module has it
        for w, bns in blocks:
            rows = h.shape[2] - 6
            y = np.zeros((h.shape[0], w.shape[0], rows, 3))
            for t in range(7):
                y += np.einsum("pirc,oi->porc", h[:, :, t:t + rows], w[:, :, t], optimize=True)
            for c in range(3):
                y[:, :, :, c] = _bn(y[:, :, :, c].transpose(0, 2, 1), bns[c]).transpose(0, 2, 1)
            h = np.maximum(y, 0)
        y = np.einsum("pirc,oic->por", h, fw, optimize=True)
        y = np.maximum(_bn(y.transpose(0, 2, 1), fbn).transpose(0, 2, 1), 0)
        feats.append(y.mean(2))
    v = np.concatenate(feats, 1)
    lg = np.maximum(v @ fc1.T + b1, 0) @ fc2.T + b2
    e = np.exp(lg - lg.max(1, keepdims=True))
    return e[:, 1] / e.sum(1)


def transform(former, latter):
    """former, latter (n, 3) float64 -> two (30, 3) float32 blocks"""
    a = np.zeros((30, 3), np.float64)
    b = np.zeros((30, 3), np.float64)
    f = former[-30:]
    a[30 - len(f):] = f
    la = latter[:30]
    b[:len(la)] = la
    both = np.concatenate([a, b], 0)
    min_, max_ = both.min(0), both.max(0)
    subtractor = (max_ + min_) / 2
    divisor = (max_ - min_) / 2 + 1e-5
    return ((a - subtractor) / divisor).astype(np.float32), ((b - subtractor) / divisor).astype(np.float32)


def candidates(table, offsets, thrT=(0, 30), thrS=75):
    table = np.asarray(table, np.float64).reshape(-1, 3)
    n = len(offsets) - 1
    trk = [table[offsets[i]:offsets[i + 1]] for i in range(n)]
    pairs, x1, x2 = [], [], []
    for i in range(n):
        for j in range(n):
            if i == j or len(trk[i]) == 0 or len(trk[j]) == 0:
                continue
            fi, bi = trk[i][-1, 0], trk[i][-1, 1:3]
            fj, bj = trk[j][0, 0], trk[j][0, 1:3]
            if not thrT[0] <= fj - fi < thrT[1]:
                continue
            dx, dy = bi[0] - bj[0], bi[1] - bj[1]
            if thrS < np.sqrt(dx * dx + dy * dy):
                continue
            a, b = transform(trk[i], trk[j])
            pairs.append((i, j)); x1.append(a); x2.append(b)
    return (np.array(pairs, np.int32).reshape(-1, 2), np.array(x1, np.float32).reshape(-1, 30, 3), np.array(x2, np.float32).reshape(-1, 30, 3))


def tracklets(rows):
    """rows sorted by frame -> (ids by first appearance, table, offsets)"""
    ids = []
    for i in rows[:, 1].tolist():
        if i not in ids:
            ids.append(i)
    parts = [rows[rows[:, 1] == i][:, [0, 2, 3]] for i in ids]
    offsets = np.zeros(len(ids) + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in parts])
    return ids, (np.concatenate(parts, 0) if parts else np.zeros((0, 3))), offsets


def decide(n, pairs, scores, thrP=0.05):
    """-> the accepted (row tracklet, column tracklet) links in ascending row order"""
    cost = (np.float32(1) - np.asarray(scores, np.float32)).astype(np.float64)
    mat = np.full((n, n), 1e5)
    for (i, j), c in zip(pairs.tolist(), cost.tolist()):
        if c <= thrP:
            mat[i, j] = c
    if n == 0:
        return []
    mask_row, mask_col = mat.min(axis=1) < thrP, mat.min(axis=0) < thrP
    if not mask_row.any() or not mask_col.any():
        return []
    sub = mat[mask_row, :][:, mask_col]
    rid, cid = np.nonzero(mask_row)[0], np.nonzero(mask_col)[0]
    r, c = linear_sum_assignment(sub)
    return [(int(rid[a]), int(cid[b])) for a, b in zip(r, c) if sub[a, b] < thrP]


def apply_links(rows, ids, links):
    id2id = dict()
    for i, j in links:
        id2id[ids[i]] = ids[j]
    ID2ID = dict()
    for k, v in id2id.items():
        if k in ID2ID:
            ID2ID[v] = ID2ID[k]
        else:
            ID2ID[v] = k
    res = rows.copy()
    for k, v in ID2ID.items():
        res[res[:, 1] == k, 1] = v
    if len(res) == 0:
        return res
    _, index = np.unique(res[:, :2], return_index=True, axis=0)
    return res[index]


def link(rows, score_fn, thrT=(0, 30), thrS=75, thrP=0.05, trace=None):
    rows = np.asarray(rows, np.float64)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    ids, table, offsets = tracklets(rows)
    pairs, x1, x2 = candidates(table, offsets, thrT, thrS)
    scores = np.asarray(score_fn(pairs, x1, x2), np.float32).reshape(-1)
    links = decide(len(ids), pairs, scores, thrP)
    if trace is not None:
        trace.update(ids=ids, table=table, offsets=offsets, pairs=pairs, x1=x1, x2=x2, scores=scores, links=np.array(links, np.int32).reshape(-1, 2))
    return apply_links(rows, ids, links)
