"""tests/map_scenes.py -- TEST INFRASTRUCTURE ONLY: the seeded cases of the mAP tests (tests/test_map_cpu.py, tests/test_map_gpu.py) and of the recorder
tests/golden/make_golden_map.py.  Matching cases are batches (predictions in network pixels, normalised targets, the letterbox rows); compute cases are stored rows
(tp, conf, class) with the targets per class."""
import numpy as np
import torch

from tests import map_np

MAX_DET = 300
NIOU = 10


# ---------------------------------------------------------------------------------------------
# matching cases: dict(hw, lb (B, 5) f32, preds [B x (P, 6) f32 torch], targets (L, 6) f32 torch, nc)
# ---------------------------------------------------------------------------------------------
def _lb_square(B, size):
    return np.tile(np.array([[1.0, 0.0, 0.0, size, size]], np.float32), (B, 1))


def _image(rng, P, T, size, ncls, b):
    """T random targets, P predictions: jittered copies of targets first (several a target), then strays (the caller fills the confidences in)"""
    cls = rng.integers(0, ncls, T).astype(np.float32)
    wh = rng.uniform(0.04, 0.3, (T, 2))
    c = rng.uniform(0.1, 0.9, (T, 2))
    tg = np.concatenate([np.full((T, 1), b), cls[:, None], c, wh], 1).astype(np.float32)
    rows = []
    for p in range(P):
        if T and p < 0.8 * P:
            t = int(rng.integers(0, T))
            box = np.array([c[t, 0] - wh[t, 0] / 2, c[t, 1] - wh[t, 1] / 2, c[t, 0] + wh[t, 0] / 2, c[t, 1] + wh[t, 1] / 2]) * size
            box += rng.normal(0, 0.06 * size * float(wh[t].mean()), 4)
            k = cls[t] if rng.random() < 0.85 else float(rng.integers(0, ncls))
        else:
            xy = rng.uniform(0, 0.8 * size, 2)
            box = np.concatenate([xy, xy + rng.uniform(0.04, 0.3, 2) * size])
            k = float(rng.integers(0, ncls))
        rows.append([box[0], box[1], box[2], box[3], 0.0, k])
    pred = np.array(rows, np.float32).reshape(-1, 6)
    return pred, tg


def _batch(seed, shapes, size=640, ncls=4):
    rng = np.random.default_rng(9000 + seed)
    preds, tgs = [], []
    n_pool = max(4000, sum(P for P, _ in shapes))
    pool, used = (rng.permutation(n_pool) + 1) / (n_pool + 1.0), 0      # confidences distinct over the whole batch
    for b, (P, T) in enumerate(shapes):
        p, t = _image(rng, P, T, size, ncls, b)
        p[:, 4] = np.sort(pool[used:used + P])[::-1]
        used += P
        preds.append(torch.from_numpy(p))
        tgs.append(t)
    return dict(hw=(size, size), lb=_lb_square(len(shapes), size), preds=preds, targets=torch.from_numpy(np.concatenate(tgs, 0).astype(np.float32).reshape(-1, 6)),
                nc=max(ncls, 2))


def _two_claim():
    """predictions 0 and 1 both take target 0 (IoU 0.81 and 0.68); prediction 1's second-best, target 1, is at IoU 0.56 > 0.5 and must not be handed to it; prediction
    2 takes target 1"""
    size = 640
    tg = np.array([[0, 1, 0.25, 0.25, 0.3125, 0.3125], [0, 1, 0.3125, 0.25, 0.3125, 0.3125]], np.float32)      # boxes (60, 60, 260, 260) and (100, 60, 300, 260)
    pred = np.array([[62, 62, 250, 262, 0.9, 1], [78, 60, 278, 260, 0.8, 1], [104, 64, 298, 256, 0.7, 1]], np.float32)
    return dict(hw=(size, size), lb=_lb_square(1, size), preds=[torch.from_numpy(pred)], targets=torch.from_numpy(tg), nc=2)


def _other_class():
    """prediction 0 (class 0) lies on a class-1 target; its best same-class target is a poor match; prediction 1 has no target of its class at all"""
    size = 640
    tg = np.array([[0, 1, 0.25, 0.25, 0.25, 0.25], [0, 0, 0.5, 0.5, 0.25, 0.25]], np.float32)
    pred = np.array([[80, 80, 240, 240, 0.9, 0], [80, 80, 240, 240, 0.8, 2], [240, 240, 400, 400, 0.7, 0]], np.float32)
    return dict(hw=(size, size), lb=_lb_square(1, size), preds=[torch.from_numpy(pred)], targets=torch.from_numpy(tg), nc=3)


def _ulp():
    """per threshold k three (target, prediction) pairs whose float32 IoU is the float just below iouv[k], iouv[k] itself and the float just above.  Every pair has
    its own class and its own row band of a 1024 x 1024 image (gain 1, no pad): the target is wt x 1, the prediction w x 1 inside it, so that the IoU is about w / wt;
    w is searched among the neighbours of wt v, over a few wt, until torch's box_iou gives exactly the wanted float"""
    size = 1024
    thr = map_np.iouv().numpy()
    tg, pred = [], []
    for k in range(NIOU):
        for step in (-1, 0, 1):
            want = thr[k] if step == 0 else np.nextafter(thr[k], np.float32(2.0 * step), dtype=np.float32)
            j = len(tg)
            found = None
            for wt in (512, 768, 640, 896):      # (the sum of the two areas rounds: not every float is reached from every target width)
                tb = torch.tensor([[0.0, 2.0 * j, float(wt), 2.0 * j + 1.0]])
                w = np.float32(wt) * want
                for _ in range(40):
                    w = np.nextafter(w, np.float32(0), dtype=np.float32)
                for _ in range(81):
                    pb = torch.tensor([[0.0, 2.0 * j, float(w), 2.0 * j + 1.0]])
                    if np.float32(map_np.box_iou(pb, tb)[0, 0].item()) == want:
                        found = (wt, float(w))
                        break
                    w = np.nextafter(w, np.float32(2048), dtype=np.float32)
                if found:
                    break
            assert found is not None, (k, step)
            tg.append(np.array([0, j, found[0] / 2.0 / size, (2 * j + 0.5) / size, float(found[0]) / size, 1.0 / size], np.float32))
            pred.append([0.0, 2.0 * j, found[1], 2.0 * j + 1.0, 0.0, j])
    pred = np.array(pred, np.float32)
    pred[:, 4] = 0.99 - 0.01 * np.arange(len(pred), dtype=np.float32)
    return dict(hw=(size, size), lb=_lb_square(1, size), preds=[torch.from_numpy(pred)], targets=torch.from_numpy(np.array(tg, np.float32)), nc=len(tg))


def _clamp():
    """a 500 x 1000 image letterboxed into 384 x 640 (gain 0.64, 32 rows of pad above and below): targets and predictions that reach into the pad and past the sides"""
    H, W = 384, 640
    lb = np.array([[0.64, 0.0, 32.0, 500.0, 1000.0]], np.float32)
    tg = np.array([[0, 0, 0.05, 0.12, 0.2, 0.2], [0, 0, 0.97, 0.5, 0.12, 0.3], [0, 1, 0.5, 0.93, 0.3, 0.2], [0, 1, 0.5, 0.5, 0.2, 0.2]], np.float32)
    pred = np.array([[-20, 10, 95, 84, 0.9, 0], [580, 130, 660, 250, 0.85, 0], [230, 320, 420, 400, 0.8, 1], [258, 155, 380, 231, 0.75, 1], [-5, -5, 30, 30, 0.6, 1]],
                    np.float32)
    return dict(hw=(H, W), lb=lb, preds=[torch.from_numpy(pred)], targets=torch.from_numpy(tg), nc=2)


MATCH_CASES = {
    "p0_t3": lambda: _batch(1, [(0, 3)]),
    "p5_t0": lambda: _batch(2, [(5, 0)]),
    "empty": lambda: _batch(3, [(0, 0)]),
    "p1_t1": lambda: _batch(4, [(1, 1)], ncls=1),
    "p65_t3": lambda: _batch(5, [(65, 3)], ncls=2),
    "p300_t70": lambda: _batch(6, [(300, 70)]),
    "two_claim": _two_claim,
    "other_class": _other_class,
    "ulp": _ulp,
    "clamp": _clamp,
    "batch5": lambda: _batch(7, [(40, 9), (0, 4), (17, 0), (300, 30), (3, 2)]),
}


def split(case, lo, hi):
    """images [lo, hi) of a case as a case of their own"""
    t = case["targets"]
    sel = (t[:, 0] >= lo) & (t[:, 0] < hi)
    t2 = t[sel].clone()
    t2[:, 0] -= lo
    return dict(hw=case["hw"], lb=case["lb"][lo:hi], preds=case["preds"][lo:hi], targets=t2, nc=case["nc"])


def raw_args(case, max_det=MAX_DET, seed=0):
    """-> the arrays y7t_map_update takes: dets (B, max_det, 6) whose box columns are poison (only conf and cls may be read), ndets, keep, cbox (B, cap, 4) with the
    boxes at shuffled candidate slots, targets grouped by image, offsets"""
    B = len(case["preds"])
    cap = max([len(p) for p in case["preds"]] + [1]) + 7
    rng = np.random.default_rng(77 + seed)
    dets = np.full((B, max_det, 6), -1e4, np.float32)
    keep = np.full((B, max_det), -5, np.int32)
    cbox = rng.uniform(0, 50, (B, cap, 4)).astype(np.float32)
    nd = np.zeros(B, np.int32)
    for b, p in enumerate(case["preds"]):
        p = p.numpy()
        n = len(p)
        slots = rng.permutation(cap)[:n]
        cbox[b, slots] = p[:, :4]
        keep[b, :n] = slots
        dets[b, :n, 4:] = p[:, 4:]
        nd[b] = n
    t = case["targets"].numpy().reshape(-1, 6)
    off = np.searchsorted(t[:, 0], np.arange(B + 1), side="left").astype(np.int32)
    return dict(dets=dets, ndets=nd, keep=keep, cbox=cbox, targets=t, toff=off, hw=case["hw"], lb=case["lb"], iouv=map_np.iouv().numpy())


def expected_stats(case, fn=None):
    """the case through the literal loop -> (correct, conf, cls int32, nt (nc,))"""
    cor, conf, cls, tcls = map_np.batch_stats(case["preds"], case["targets"], case["hw"], case["lb"], fn or map_np.image_stats)
    nt = np.bincount(np.array(tcls, np.int64), minlength=case["nc"]) if len(tcls) else np.zeros(case["nc"], np.int64)
    return cor, conf.astype(np.float32), cls.astype(np.int32), nt.astype(np.int64)


# ---------------------------------------------------------------------------------------------
# compute cases: dict(tp (N, 10) bool, conf (N,) f32, cls (N,) int32, nt (nc,) int64, nc)
# ---------------------------------------------------------------------------------------------
def _rows(seed, N, nt, pred_classes=None, distinct=True, hit=0.6):
    """N rows over the classes `pred_classes` (default: the classes with targets); tp nested over the thresholds, at most nt[c] true per class and threshold"""
    rng = np.random.default_rng(12000 + seed)
    nt = np.asarray(nt, np.int64)
    nc = len(nt)
    pc = np.asarray(pred_classes if pred_classes is not None else np.nonzero(nt)[0], np.int64)
    cls = pc[rng.integers(0, len(pc), N)].astype(np.int32) if N else np.zeros(0, np.int32)
    if distinct:
        conf = ((rng.permutation(max(N, 1))[:N] + 1) / np.float64(N + 1)).astype(np.float32)
        assert len(np.unique(conf)) == N
    else:
        conf = (rng.integers(1, 12, N) / 12.0).astype(np.float32)
    level = np.where(rng.random(N) < hit, rng.integers(1, NIOU + 1, N), 0)      # thresholds 0 .. level - 1 are passed
    tp = np.arange(NIOU)[None, :] < level[:, None]
    for c in range(nc):      # no more true positives than targets
        idx = np.nonzero(cls == c)[0]
        hits = idx[tp[idx, 0]]      # (nested: a row true at any threshold is true at threshold 0)
        tp[hits[int(nt[c]):]] = False
    return dict(tp=tp, conf=conf, cls=cls, nt=nt, nc=nc)


def _nl(n_l):
    return _rows(100 + n_l, 3 * n_l + 2, [n_l], hit=0.8)


COMPUTE_CASES = {
    "class_gaps": lambda: _rows(1, 60, [7, 5, 0, 0], pred_classes=[0, 2]),
    "one_row": lambda: _rows(2, 1, [0, 3], pred_classes=[1], hit=1.0),
    "rows_1": lambda: _rows(3, 1, [2, 2, 2]),
    "rows_255": lambda: _rows(4, 255, [40, 90, 30]),
    "rows_256": lambda: _rows(5, 256, [40, 90, 30]),
    "rows_257": lambda: _rows(6, 257, [40, 90, 30]),
    "rows_70000": lambda: _rows(7, 70000, [9000, 15000, 4000]),
    "nc80": lambda: _rows(8, 3000, [0 if c == 37 else 5 + (c * 7) % 23 for c in range(80)]),
    "nc300": lambda: _rows(9, 2000, [0 if c % 5 == 4 else 3 + c % 11 for c in range(300)]),
}
for _n in (1, 2, 4, 5, 10, 20, 25, 50, 100):
    COMPUTE_CASES["nl_%d" % _n] = (lambda n: (lambda: _nl(n)))(_n)
EQUAL_CONF_CASE = lambda: _rows(50, 900, [60, 45, 0, 80], pred_classes=[0, 1, 2, 3], distinct=False)


def target_cls_of(nt):
    return np.repeat(np.arange(len(nt)), nt).astype(np.float64)


def masks(tp):
    return (tp.astype(np.int32) << np.arange(NIOU, dtype=np.int32)).sum(1).astype(np.int32)


def expected_compute(case, ap_per_class=None):
    """-> dict(p, r, ap, f1, classes) of map_np.ap_per_class (or the function given) over the case"""
    f = ap_per_class or map_np.ap_per_class
    p, r, ap, f1, classes = f(case["tp"], case["conf"], case["cls"].astype(np.float32), target_cls_of(case["nt"]))
    return dict(p=p, r=r, ap=ap, f1=f1, classes=np.asarray(classes, np.int32))
