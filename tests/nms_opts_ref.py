"""non_max_suppression (utils/general.py:629-690) with `classes`, `agnostic` and `multi_label`, restated for the tests of y7t_det_postprocess_ex, and the scenes of those
tests.  Plain helpers shared by tests/test_nms_opts_scenes.py (CPU: every scene has the property its case is about, under this restatement alone) and
tests/test_nms_opts_gpu.py (the kernels against it).  numpy only at import time.

A candidate scene is post_scenes' dict of ONE image's candidate arrays in slot order -- box (n, 4), score (n,), cls (n,), rows (n,) -- except that with multi_label
several candidates may share an anchor row: the pairs (row, cls) are unique.

The order of the walk (where the reference leaves equal scores to its sort): score descending, then anchor row ascending, then class ascending -- the order of
`nonzero()` at general.py:655 and, without multi_label, of oracle.detector_torch.nms_rows."""
import functools

import numpy as np

from tests import post_scenes as ps

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def class_filter(cls, classes):
    """general.py:662-663: (x[:, 5:6] == torch.tensor(classes)).any(1); classes None: everything stays"""
    if classes is None:
        return np.ones(len(cls), bool)
    return np.isin(np.asarray(cls, np.float32), np.asarray(list(classes), np.float32))


def walk(scene, iou_thres=0.45, max_nms=30000, max_det=300, classes=None, agnostic=False):
    """general.py:661-682 on one image's candidates: class filter, the max_nms best by (score desc, row asc, class asc), greedy NMS (oracle.cnative.nms) on the float32
    boxes offset by cls * 4096 (agnostic: by 0), first max_det.  -> the kept candidate SLOTS in output order"""
    from oracle import cnative
    box, s, c, rows = scene["box"], scene["score"], scene["cls"], scene["rows"]
    live = np.nonzero(class_filter(c, classes))[0]
    if not len(live):
        return np.zeros(0, np.int64)
    order = live[np.lexsort((c[live], rows[live], -s[live].astype(np.float64)))][:max_nms]
    off = F32(0) if agnostic else ps.MAX_WH
    k = cnative.nms((box + c[:, None] * off).astype(np.float32)[order], s[order], float(F32(iou_thres)))[:max_det]
    return order[k]


def candidates(dec, conf_thres, multi_label=False):
    """general.py:632-659 on ONE image's decoded tensor (A, 5 + nc) float32 -> a candidate scene in (row, class) order, + "vec" (n, nc): the row's class confidences"""
    dec = np.asarray(dec, np.float32)
    nc = dec.shape[1] - 5
    rows = np.nonzero(dec[:, 4] > F32(conf_thres))[0]                      # xc
    x = dec[rows]
    conf = (x[:, 5:] * x[:, 4:5]).astype(np.float32)                       # x[:, 5:] *= x[:, 4:5]
    box = np.stack([x[:, 0] - x[:, 2] / 2, x[:, 1] - x[:, 3] / 2, x[:, 0] + x[:, 2] / 2, x[:, 1] + x[:, 3] / 2], 1).astype(np.float32)
    if multi_label and nc > 1:                                             # multi_label &= nc > 1
        i, j = np.nonzero(conf > F32(conf_thres))
    else:
        j = conf.argmax(1)
        i = np.nonzero(conf[np.arange(len(rows)), j] > F32(conf_thres))[0]
        j = j[i]
    return {"box": box[i], "score": conf[i, j], "cls": j.astype(np.float32), "rows": rows[i].astype(np.int32), "vec": conf[i]}


def nms(pred, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_nms=30000, max_det=300):
    """non_max_suppression on a decoded (B, A, 5 + nc) array -> list of (n, 6) float32 arrays [xyxy, conf, cls]"""
    out = []
    for dec in np.asarray(pred, np.float32):
        c = candidates(dec, conf_thres, multi_label)
        k = walk(c, iou_thres, max_nms, max_det, classes, agnostic)
        out.append(np.concatenate([c["box"][k], c["score"][k, None], c["cls"][k, None]], 1).astype(np.float32))
    return out


def decode(scene):
    """the oracle's Detect decode of a head-logit scene -> (B, A, no) float32"""
    import torch
    from oracle import detector_torch as dt
    na, no, z = scene["na"], scene["no"], []
    for h, st, an in zip(scene["heads"], scene["strides"], scene["anchors"]):
        B, ny, nx, _ = h.shape
        x = torch.from_numpy(h.reshape(B, ny, nx, na, no)).permute(0, 3, 1, 2, 4).contiguous()
        z.append(dt.decode_level(x, torch.from_numpy(an), float(st)))
    return torch.cat(z, 1).numpy()


# ------------------------------------------------------------------------------------------------ candidate scenes
def _scene(box, score, cls, rows):
    s = {"box": np.array(box, np.float32), "score": np.array(score, np.float32), "cls": np.array(cls, np.float32), "rows": np.array(rows, np.int32)}
    n = len(s["score"])
    assert s["box"].shape == (n, 4) and len(s["cls"]) == len(s["rows"]) == n and len(set(zip(s["rows"].tolist(), s["cls"].tolist()))) == n
    for v in s.values():
        v.flags.writeable = False
    return s


@functools.lru_cache(maxsize=None)
def mixed_clusters(n=400, seed=0, nc=3):
    """post_scenes.clustered with the class drawn per CANDIDATE: every cluster holds all the classes, so the class-aware walk keeps about nc boxes per object and the
    agnostic walk one"""
    base = ps.clustered(n, seed=seed, nc=nc)
    rng = np.random.default_rng([seed, n, 21])
    return _scene(base["box"], base["score"], rng.integers(0, nc, n), base["rows"])


@functools.lru_cache(maxsize=None)
def two_class_pairs(groups=6, seed=1):
    """`groups` disjoint boxes, each bit-identically in class 0 and class 1 (IoU exactly 1 across the classes), plus per group a third box of class 2 at IoU exactly 0.5
    with them ([x, 0, x + 4, 4] and [x, 0, x + 4, 2]).  Distinct scores.  Class-aware: 3 per group; agnostic at 0.45: 1; at 0.5: 2 (the test is >); at 1.0: 3."""
    rng = np.random.default_rng([seed, groups, 22])
    x = np.repeat(np.arange(groups) * 100.0, 3)
    box = np.stack([x, 0 * x, x + 4, 0 * x + 4], 1)
    box[2::3, 3] = 2
    n = 3 * groups
    p = rng.permutation(n)
    return _scene(box[p], ps._distinct_scores(rng, n)[p], np.tile([0, 1, 2], groups)[p], ps._rows(rng, n))


@functools.lru_cache(maxsize=None)
def tied_pairs(groups=40, seed=2):
    """`groups` disjoint boxes, each twice bit-identically in two classes with the SAME score bit for bit: the agnostic walk keeps the one with the smaller anchor row;
    the class of the smaller row is drawn, so neither "class 0 wins" nor "slot order wins" gives the answer"""
    rng = np.random.default_rng([seed, groups, 23])
    x = np.repeat(np.arange(groups) * 50.0 + rng.uniform(0, 9, groups), 2)
    box = np.stack([x, 0 * x + 1.5, x + 30.25, 0 * x + 41], 1)
    s = np.repeat(ps._distinct_scores(rng, groups // 4), 8)[:2 * groups]                    # ... and four groups share a score too
    cls = np.stack([rng.permutation(2) for _ in range(groups)]).ravel()
    n = 2 * groups
    p = rng.permutation(n)
    return _scene(box[p], s[p], cls[p], ps._rows(rng, n))


@functools.lru_cache(maxsize=None)
def filter_before_cut(max_nms=4, seed=3):
    """the `max_nms` best candidates are of class 0 and mutually disjoint; below them 12 disjoint boxes of classes 1 and 2.  classes=[1, 2] at this max_nms keeps the best
    four of those; cutting first and filtering afterwards keeps nothing"""
    rng = np.random.default_rng([seed, max_nms, 24])
    n = max_nms + 12
    x = np.arange(n) * 40.0
    s = np.sort(ps._distinct_scores(rng, n))[::-1]
    cls = np.concatenate([np.zeros(max_nms), 1 + rng.integers(0, 2, 12)])
    p = rng.permutation(n)
    return _scene(np.stack([x, 0 * x, x + 20, 0 * x + 20], 1)[p], s[p], cls[p], ps._rows(rng, n))


def no_class(scene, c):
    """`scene` without its candidates of class c"""
    m = scene["cls"] != c
    return _scene(scene["box"][m], scene["score"][m], scene["cls"][m], scene["rows"][m])


# ------------------------------------------------------------------------------------------------ head-logit scenes (k_decode_filter_ml)
PLANT_OBJ, PLANT_ON, PLANT_OFF = 4.0, 3.0, -9.0      # objectness 0.982; class confidence 0.935 / 0.00012: on either side of every conf_thres in [0.001, 0.9]


def planted_rows(gi):
    """(image, level, y, x, anchor) -> number of classes planted ON, for GRIDS[gi]: with nc > 1 rows with 0, 1, 2 and all nc classes passing, in level 0 of image 0;
    with one class one row that passes (the single row of the 1 x 1 grid: its image is not empty)"""
    nl, na, no, shapes, B = ps.GRIDS[gi]
    nc = no - 5
    if nc < 2:
        return {(0, 0, 0, 0, 0): 1}
    return {(0, 0, 0, 0, 0): 0, (0, 0, 0, 1, 0): 1, (0, 0, 1, 0, na - 1): 2, (0, 0, 1, 1, 0): nc}


def conf64(h, na, no):
    """float64 objectness (B, ny, nx, na) and per-class confidence (B, ny, nx, na, nc) of a level's logits"""
    v = h.reshape(h.shape[:3] + (na, no)).astype(np.float64)
    obj = 1.0 / (1.0 + np.exp(-v[..., 4]))
    return obj, 1.0 / (1.0 + np.exp(-v[..., 5:])) * obj[..., None]


@functools.lru_cache(maxsize=None)
def ml_scene(gi, conf_thres, obj_logit=None):
    """post_scenes.decode_scene(gi, conf_thres) with (a) NO objectness and NO per-class confidence within BAND of conf_thres (decode_scene clears the band for the best
    class alone): the class logits of such a row are drawn again, at most 200 times; (b) for nc > 1 the rows of planted_rows(gi): objectness logit PLANT_OBJ, k class
    logits at PLANT_ON -- bit-equal logits: the row's k candidates tie in score and come out in class order -- and the others at PLANT_OFF."""
    base = ps.decode_scene(gi, conf_thres, obj_logit=obj_logit)
    nl, na, no, shapes, B = ps.GRIDS[gi]
    nc = no - 5
    rng = np.random.default_rng([gi, int(round(conf_thres * 1e4)), 25])
    heads = [h.copy() for h in base["heads"]]
    for (b, l, y, x, an), k in planted_rows(gi).items():
        v = heads[l].reshape(heads[l].shape[:3] + (na, no))
        on = rng.choice(nc, k, replace=False)
        v[b, y, x, an, 4] = PLANT_OBJ
        v[b, y, x, an, 5:] = PLANT_OFF
        v[b, y, x, an, 5 + on] = PLANT_ON
    for h in heads:
        v = h.reshape(h.shape[:3] + (na, no))
        for _ in range(200):
            obj, conf = conf64(h, na, no)
            bad = (np.abs(conf - conf_thres) < ps.BAND).any(-1)
            assert not (np.abs(obj - conf_thres) < ps.BAND).any()          # (decode_scene's own condition)
            if not bad.any():
                break
            v[bad, 5:] = (rng.standard_normal((int(bad.sum()), nc)) * 1.5).astype(np.float32)
        else:
            raise AssertionError("could not clear the band around conf_thres")
    out = dict(base)
    out["heads"] = [np.ascontiguousarray(h) for h in heads]
    return out


def thread_order_rows(scene, level=0):
    """the anchor rows of one image's level in the order k_decode_filter(_ml)'s threads take them: x fastest, then anchor, then y"""
    na = scene["na"]
    ny, nx = scene["shapes"][level]
    row0 = sum(na * a * b for a, b in scene["shapes"][:level])
    r = np.arange(na * ny * nx)
    x, an, y = r % nx, (r // nx) % na, r // (nx * na)
    return row0 + (an * ny + y) * nx + x


def straddle_cap(scene, conf_thres, lo=64):
    """-> (cap, the first `cap` (row, class) pairs of image 0 in reservation order): the smallest cap >= lo that falls strictly INSIDE the reservation of one row of image
    0's level 0.  That level's rows of image 0 belong to one wave (asserted), whose reservations are handed out in lane order by the wave's scan: the pairs below cap are
    then determined -- the rows in thread order, each row's classes ascending."""
    order = thread_order_rows(scene, 0)
    assert len(order) <= 64
    c = candidates(decode(scene)[0], conf_thres, multi_label=True)
    pairs, ends = [], []
    for r in order:
        m = c["rows"] == r
        pairs += [(int(r), int(k)) for k in c["cls"][m]]
        ends.append(len(pairs))
    for cap in range(lo, len(pairs)):
        if cap not in ends:
            return cap, pairs[:cap]
    raise AssertionError("no row of level 0 straddles a cap >= %d" % lo)
