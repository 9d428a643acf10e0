"""Seeded scenes and the reference walk for the post-processing chain of csrc/y7t_post.hip (k_decode_filter -> k_rank_sort -> k_nms_keep behind
y7t_det_postprocess).  Plain helpers shared by tests/test_post_scenes.py (CPU: every scene meets its stated conditions under the oracle alone, so no GPU
test passes vacuously) and tests/test_postprocess_gpu.py (the kernels against the reference walk).  numpy only at import time.

A candidate scene is a dict of ONE image's candidate arrays in SLOT order, the order the decode's atomicAdd hands slots out in:
    box (n, 4) float32 xyxy | score (n,) float32 | cls (n,) float32 | rows (n,) int32 anchor rows -- unique, a random permutation (slot order != row order)"""
import functools

import numpy as np

MAX_WH = np.float32(4096)          # class offset of non_max_suppression (utils/general.py:618)
ROW_SPACE = 102000                 # anchor rows are drawn from [0, ROW_SPACE): the row count of yolov7-w6 at 1280 x 1280
F32 = np.float32


# ------------------------------------------------------------------------------------------------ workspace layout
def _rup(n):
    return (n + 255) // 256 * 256


def ws_layout(B, cap, max_nms=30000):
    """byte layout of y7t_det_postprocess' workspace (include/y7t.h; Detector.candidate_arrays mirrors its head): name -> (offset, bytes), each array
    256-byte aligned, + "total" = y7t_det_postprocess_workspace_bytes(B, cap, max_nms).  Callers may write cbox / cscore / ccls / cidx / count (head == NULL);
    nsorted / sbox / sorder / lb are the chain's own scratch."""
    mcap = min(cap, max_nms)
    lay, o = {}, 0
    for name, nbytes in (("cbox", B * cap * 16), ("cscore", B * cap * 4), ("ccls", B * cap * 4), ("cidx", B * cap * 4), ("count", B * 4), ("nsorted", B * 4),
                         ("sbox", B * mcap * 16), ("sorder", B * mcap * 4), ("lb", B * 5 * 4)):
        lay[name] = (o, nbytes)
        o += _rup(nbytes)
    lay["total"] = o + 256
    return lay


CAND_FIELDS = (("cbox", np.float32, 4), ("cscore", np.float32, 1), ("ccls", np.float32, 1), ("cidx", np.int32, 1))
SENTINEL = 0xA5                    # byte pattern of everything a scene does not define (as a float ~ -2.9e-16, as an int < 0: nothing a kernel may read as a candidate)


def pack_candidates(scenes, cap, counts=None, max_nms=30000):
    """the head of a workspace (cbox .. count, up to the start of nsorted) with `scenes` planted, image b's n_b candidates in slots [0, n_b) and SENTINEL bytes everywhere
    else -- the slots past n_b and the padding behind each array included.  counts: what to write into `count` instead of the n_b (overflow: > cap).  -> uint8 array"""
    B = len(scenes)
    lay = ws_layout(B, cap, max_nms)
    buf = np.full(lay["nsorted"][0], SENTINEL, np.uint8)
    for name, dtype, width in CAND_FIELDS:
        o, nbytes = lay[name]
        view = buf[o:o + nbytes].view(dtype).reshape(B, cap, width)
        for b, s in enumerate(scenes):
            n = len(s["score"])
            assert n <= cap
            view[b, :n] = np.asarray({"cbox": s["box"], "cscore": s["score"], "ccls": s["cls"], "cidx": s["rows"]}[name]).reshape(n, width)
    o, nbytes = lay["count"]
    buf[o:o + nbytes].view(np.int32)[:] = [len(s["score"]) for s in scenes] if counts is None else counts
    return buf


def unpack_candidates(buf, B, cap, max_nms=30000):
    """-> (cbox (B, cap, 4), cscore (B, cap), ccls (B, cap), cidx (B, cap), count (B,)) views of a workspace's bytes (numpy uint8)"""
    lay = ws_layout(B, cap, max_nms)
    out = []
    for name, dtype, width in CAND_FIELDS:
        o, nbytes = lay[name]
        v = buf[o:o + nbytes].view(dtype)
        out.append(v.reshape(B, cap, 4) if width == 4 else v.reshape(B, cap))
    o, nbytes = lay["count"]
    return tuple(out) + (buf[o:o + nbytes].view(np.int32),)


# ------------------------------------------------------------------------------------------------ the reference walk
def reference_walk(scene, iou_thres=0.45, max_nms=30000, max_det=300):
    """oracle.detector_torch.nms_rows on arrays, with both limits as arguments: sort by (score desc, anchor row asc), cut to max_nms, greedy NMS
    (oracle.cnative.nms) on the class-offset float32 boxes, cut to max_det.  -> the kept candidate SLOTS in output order (scene["rows"][...] are the kept anchor rows)"""
    from oracle import cnative
    box, s, c, rows = scene["box"], scene["score"], scene["cls"], scene["rows"]
    if not len(s):
        return np.zeros(0, np.int64)
    order = np.lexsort((rows, -s.astype(np.float64)))[:max_nms]
    k = cnative.nms((box + c[:, None] * MAX_WH).astype(np.float32)[order], s[order], float(F32(iou_thres)))[:max_det]
    return order[k]


def expected_rows(scene, slots, lb=(1.0, 0.0, 0.0, 4096.0, 4096.0)):
    """the (len(slots), 6) float32 rows the chain must write for the kept `slots` under letterbox parameters (gain, pad_w, pad_h, H0, W0): scale_coords + clip + round
    (utils/general.py:319-340, tracker/track.py:240) as ONE float32 expression per coordinate -- (x - pad) / gain, clip, round half to even -- then score and class"""
    gain, padw, padh, H0, W0 = (F32(v) for v in lb)
    b = scene["box"][slots].astype(np.float32)
    out = np.zeros((len(slots), 6), np.float32)
    for j, (pad, hi) in enumerate(((padw, W0), (padh, H0), (padw, W0), (padh, H0))):
        out[:, j] = np.rint(np.clip((b[:, j] - pad) / gain, F32(0), hi))
    out[:, 4], out[:, 5] = scene["score"][slots], scene["cls"][slots]
    return out


def prefix(scene, n):
    """the first n slots of a scene (what the chain sees of it when `count` or `cap` is n)"""
    return {k: v[:n] for k, v in scene.items()}


def suppressed_by_any_better_box(scene, iou_thres=0.45):
    """the WRONG rule -- a candidate dies when ANY better-ranked box of its class overlaps it, kept or not -- as a count of survivors (the greedy walk only lets KEPT boxes suppress)"""
    order = np.lexsort((scene["rows"], -scene["score"].astype(np.float64)))
    b = (scene["box"] + scene["cls"][:, None] * MAX_WH).astype(np.float64)[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), 0, None)
    h = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), 0, None)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (area[:, None] + area[None, :] - inter)
    better = np.tril(np.ones_like(iou, bool), -1)              # [i, j]: j ranks before i
    return int((~((iou > iou_thres) & better).any(1)).sum())


# ------------------------------------------------------------------------------------------------ candidate scenes
def _distinct_scores(rng, n):
    """n pairwise different float32 scores in (0.01, 0.99), in random order"""
    s = ((rng.permutation(n) + 1.0) / (n + 1.0) * 0.98 + 0.01).astype(np.float32)
    assert len(np.unique(s)) == n
    return s


def _rows(rng, n):
    return rng.choice(ROW_SPACE, n, replace=False).astype(np.int32)


def _scene(box, score, cls, rows):
    s = {"box": np.array(box, np.float32), "score": np.array(score, np.float32), "cls": np.array(cls, np.float32), "rows": np.array(rows, np.int32)}
    assert s["box"].shape == (len(s["score"]), 4) and len(np.unique(s["rows"])) == len(s["rows"]) == len(s["cls"]) == len(s["score"])
    for v in s.values():
        v.flags.writeable = False          # scenes are cached and shared between tests
    return s


@functools.lru_cache(maxsize=None)
def clustered(n, seed=0, n_clusters=40, jitter=0.08, nc=3):
    """n candidates around `n_clusters` boxes (40 ... 200 px, each of one class) on a 1280-px canvas: centres moved by jitter x side, sides scaled by 1 + jitter x N(0, 1).
    Most candidates of a cluster overlap its best one above 0.45; some do not and survive, so that the keep list depends on the ORDER of the walk."""
    rng = np.random.default_rng([seed, n, 1])
    ctr, wh, ccls = rng.uniform(100, 1180, (n_clusters, 2)), rng.uniform(40, 200, (n_clusters, 2)), rng.integers(0, nc, n_clusters)
    k = rng.integers(0, n_clusters, n)
    c = ctr[k] + jitter * wh[k] * rng.standard_normal((n, 2))
    s = np.maximum(wh[k] * (1.0 + jitter * rng.standard_normal((n, 2))), 1.0)
    return _scene(np.concatenate([c - s / 2, c + s / 2], 1), _distinct_scores(rng, n), ccls[k], _rows(rng, n))


BOUNDARY_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000)      # around the wave (64), the sort chunk (256) and twice / four times it


@functools.lru_cache(maxsize=None)
def separated(n=1000, seed=1, nc=10, canvas=130.0):
    """n boxes of 20 ... 60 px in nc classes with their centres scattered over `canvas` px: most are separate from every better box of their class (IoU <= 0.45), so far
    more than max_det = 300 survive the NMS, and enough are suppressed that the kept ones are not simply the first max_det of the sorted list"""
    rng = np.random.default_rng([seed, n, 2])
    c, s = rng.uniform(0, canvas, (n, 2)), rng.uniform(20, 60, (n, 2))
    return _scene(np.concatenate([c - s / 2, c + s / 2], 1), _distinct_scores(rng, n), rng.integers(0, nc, n), _rows(rng, n))


@functools.lru_cache(maxsize=None)
def chain(order="descending", n=300, seed=2):
    """boxes [10 i, 0, 10 i + 30, 30] of one class: neighbours overlap at IoU exactly 0.5, next-but-one at 0.2.  Scores run down the chain ("descending"), up it
    ("ascending") or are shuffled ("permuted").  Walked greedily at 0.45 every second box of a run survives; a rule that lets suppressed boxes suppress keeps one."""
    rng = np.random.default_rng([seed, n, 3])
    i = np.arange(n, dtype=np.float64)
    box = np.stack([10 * i, 0 * i, 10 * i + 30, 0 * i + 30], 1)
    s = np.sort(_distinct_scores(rng, n))[::-1]
    s = {"descending": s, "ascending": s[::-1], "permuted": s[rng.permutation(n)]}[order]
    p = rng.permutation(n)                                     # slot order is neither chain order nor score order
    return _scene(box[p], s[p], np.zeros(n), _rows(rng, n))


@functools.lru_cache(maxsize=None)
def tight_cluster(n=512, seed=3, jitter=0.03):
    """n candidates of one class, all within 3 % of one 200-px box: whichever is best suppresses every other one"""
    rng = np.random.default_rng([seed, n, 4])
    c = 600.0 + jitter * 200.0 * rng.standard_normal((n, 2))
    s = 200.0 * (1.0 + jitter * rng.standard_normal((n, 2)))
    return _scene(np.concatenate([c - s / 2, c + s / 2], 1), _distinct_scores(rng, n), np.zeros(n), _rows(rng, n))


@functools.lru_cache(maxsize=None)
def ties(n=320, seed=4, group=8):
    """n disjoint 20-px boxes on a 40-px lattice (nothing suppresses anything) whose scores come in groups of `group` bit-identical values: the output order inside a
    group is ascending anchor row, and with n > 300 the max_det cut falls inside a group"""
    rng = np.random.default_rng([seed, n, 5])
    i = rng.permutation(n)
    x, y = (i % 30) * 40.0, (i // 30) * 40.0
    s = np.repeat(_distinct_scores(rng, n // group), group)
    return _scene(np.stack([x, y, x + 20, y + 20], 1), s[rng.permutation(n)], rng.integers(0, 2, n), _rows(rng, n))


@functools.lru_cache(maxsize=None)
def duplicates(groups=8, copies=8, seed=5):
    """`groups` disjoint boxes with fractional coordinates, each `copies` times bit-identically, one class, distinct scores: IoU of two copies is exactly 1"""
    rng = np.random.default_rng([seed, groups, 6])
    n = groups * copies
    x = np.repeat(np.arange(groups) * 100.0 + rng.uniform(0, 9, groups), copies)
    box = np.stack([x, x * 0 + 3.25, x + 50.7, x * 0 + 61.5], 1)[rng.permutation(n)]
    return _scene(box, _distinct_scores(rng, n), np.zeros(n), _rows(rng, n))


@functools.lru_cache(maxsize=None)
def touching():
    """one class, scores descending: A, B touch along an edge (zero intersection), C overlaps B by half a pixel (IoU 0.025), D is far away"""
    box = [[0, 0, 10, 10], [10, 0, 20, 10], [19.5, 0, 30, 10], [100, 100, 110, 110]]
    return _scene(box, [0.9, 0.8, 0.7, 0.6], np.zeros(4), [40, 30, 20, 10])


@functools.lru_cache(maxsize=None)
def exact_half():
    """[0, 0, 4, 4] and [0, 0, 4, 2] of one class: intersection 8, union 16, IoU exactly 0.5 in float32"""
    return _scene([[0, 0, 4, 4], [0, 0, 4, 2]], [0.9, 0.8], np.zeros(2), [7, 3])


@functools.lru_cache(maxsize=None)
def class_offsets(n=600, seed=6, nc=80):
    """80 classes, fractional coordinates up to 1280: above class 63 the offset box + cls x 4096 lies past 2^18, where float32 keeps 1/32 px, so the sum is rounded and
    overlaps are decided on the ROUNDED boxes.  Plus: one box repeated bit-identically in 12 classes (nothing suppresses across classes), one zero-area box, one 4000-px box."""
    rng = np.random.default_rng([seed, n, 7])
    base = clustered(n - 14, seed=seed, n_clusters=60, jitter=0.1, nc=nc)       # (a cluster is of one class: its candidates do compete)
    box, cls = base["box"], base["cls"]
    extra_box = [[300.3, 200.7, 380.1, 290.9]] * 12 + [[640.5, 640.5, 640.5, 700.25], [-1000.5, -1000.5, 3000.25, 3000.25]]
    extra_cls = list(range(60, 72)) + [79, 79]
    p = rng.permutation(n)
    return _scene(np.concatenate([box, np.array(extra_box, np.float32)])[p], _distinct_scores(rng, n), np.concatenate([cls, np.array(extra_cls, np.float32)])[p], _rows(rng, n))


@functools.lru_cache(maxsize=None)
def rescale_scene(n=280, seed=7):
    """boxes for the scale_coords / clip / round tail, well separated so that nearly all are kept: odd-integer and half-integer coordinates (x.5 after a gain of 2 or 1: round
    half to even decides), fractional ones, and boxes that reach past each edge and every corner of the frame"""
    rng = np.random.default_rng([seed, n, 8])
    i = np.arange(n)
    x, y = (i % 20) * 60.0 + 5 + (i // 7) % 4, (i // 20) * 60.0 + 5 + (i // 5) % 4      # (corners of both parities: after a gain of 2, x.5 with even and odd floors)
    wh = rng.integers(10, 25, (n, 2)) * 2 + 1.0                 # odd sides from odd corners: even far corners ... mixed below
    box = np.stack([x, y, x + wh[:, 0], y + wh[:, 1]], 1)
    box[i % 4 == 1] += 0.5                                      # half-integer coordinates
    box[i % 4 == 2] += rng.uniform(0, 1, (int((i % 4 == 2).sum()), 4))      # fractional coordinates
    outside = np.array([[-30.5, 40, 20, 80], [40, -30.5, 80, 20], [1250, 40, 1400.5, 80], [40, 1250, 80, 1400.5], [-50, -50, 30, 30], [1200, 1200, 2000, 2000],
                        [-50, 1200, 30, 2000], [1200, -50, 2000, 30], [-100, -100, 3000, 3000]])
    box = np.concatenate([box, outside])
    m = len(box)
    p = rng.permutation(m)
    return _scene(box[p], _distinct_scores(rng, m), (np.arange(m) % 7)[p], _rows(rng, m))


# ------------------------------------------------------------------------------------------------ head-logit scenes (k_decode_filter)
# (nl, na, no, [(ny, nx) per level], B)
GRIDS = ((1, 1, 6, ((1, 1),), 1),
         (2, 3, 6, ((3, 5), (2, 3)), 3),                         # one class (the MOT17 configuration), non-square maps
         (4, 3, 15, ((8, 10), (4, 5), (2, 3), (1, 2)), 2),
         (3, 2, 85, ((6, 4), (3, 2), (2, 1)), 2))
BAND = 1e-4      # no objectness / confidence within BAND of conf_thres: three orders above the few-ulp error of a float32 expf + division, so membership is unambiguous


def _sig64(x):
    return 1.0 / (1.0 + np.exp(-x.astype(np.float64)))


def scores64(heads, na, no):
    """float64 objectness and best-class confidence of every anchor of every level: list of ((B, ny, nx, na) obj, (B, ny, nx, na) conf)"""
    out = []
    for h in heads:
        v = h.reshape(h.shape[:3] + (na, no))
        obj = _sig64(v[..., 4])
        out.append((obj, (_sig64(v[..., 5:]) * obj[..., None]).max(-1)))
    return out


@functools.lru_cache(maxsize=None)
def decode_scene(gi, conf_thres, seed=0, obj_logit=None):
    """Detect head logits for GRIDS[gi]: N(0, 1.5), the objectness shifted so that about a third of the anchors pass the candidate filter at conf_thres (obj_logit: every
    objectness logit at that value instead), arbitrary positive strides and anchors.  A row whose float64 objectness or confidence falls within BAND of conf_thres is
    drawn again.  -> dict heads [(B, ny, nx, na * no) float32 NHWC per level], strides (nl,), anchors (nl, na, 2), nl, na, no, B, A (anchor rows per image)"""
    nl, na, no, shapes, B = GRIDS[gi]
    rng = np.random.default_rng([seed, gi, int(round(conf_thres * 1e4)), 9])
    strides = rng.uniform(4, 40, nl).astype(np.float32)
    anchors = rng.uniform(5, 120, (nl, na, 2)).astype(np.float32)
    raw = [(rng.standard_normal((B, ny, nx, na, no)) * 1.5) for ny, nx in shapes]
    A = sum(na * ny * nx for ny, nx in shapes)
    if obj_logit is not None:
        shift = None
    else:
        z4 = np.concatenate([r[..., 4].ravel() for r in raw])
        cls = np.concatenate([_sig64(r[..., 5:]).max(-1).ravel() for r in raw])
        want = -(-len(z4) // 3)
        lo, hi = -30.0, 30.0
        for _ in range(60):                                    # the pass count is monotone in the shift
            mid = (lo + hi) / 2
            obj = _sig64(z4 + mid)
            lo, hi = (lo, mid) if ((obj > conf_thres) & (obj * cls > conf_thres)).sum() >= want else (mid, hi)
        shift = hi
    heads = []
    for r in raw:
        r[..., 4] = obj_logit if shift is None else r[..., 4] + shift
        h = r.astype(np.float32)
        for _ in range(200):
            obj, conf = scores64([h.reshape(h.shape[:3] + (na * no,))], na, no)[0]
            bad = (np.abs(obj - conf_thres) < BAND) | (np.abs(conf - conf_thres) < BAND)
            if not bad.any():
                break
            fresh = rng.standard_normal((int(bad.sum()), no)) * 1.5
            fresh[:, 4] = obj_logit if shift is None else fresh[:, 4] + shift
            h[bad] = fresh.astype(np.float32)
        else:
            raise AssertionError("could not clear the band around conf_thres")
        heads.append(np.ascontiguousarray(h.reshape(h.shape[:3] + (na * no,))))
    return {"heads": heads, "strides": strides, "anchors": anchors, "nl": nl, "na": na, "no": no, "B": B, "A": A, "shapes": shapes}


def decode_reference(scene, conf_thres):
    """the oracle's Detect decode (oracle.detector_torch.decode_level per level, the stride passed explicitly) and candidate filter (oracle.detector_torch.candidates) of a
    head-logit scene -> per image: dict anchor row -> (xyxy float32, conf, cls, per-class confidences)"""
    import torch
    from oracle import detector_torch as dt
    na, no = scene["na"], scene["no"]
    z = []
    for h, st, an in zip(scene["heads"], scene["strides"], scene["anchors"]):
        B, ny, nx, _ = h.shape
        x = torch.from_numpy(h.reshape(B, ny, nx, na, no)).permute(0, 3, 1, 2, 4).contiguous()          # the reference's (bs, na, ny, nx, no) view
        z.append(dt.decode_level(x, torch.from_numpy(an), float(st)))
    dec = torch.cat(z, 1)
    return [dt.candidates(dec[b], conf_thres) for b in range(scene["B"])]
