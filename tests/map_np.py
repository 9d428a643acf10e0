"""tests/map_np.py -- TEST INFRASTRUCTURE ONLY: the NumPy / torch statement of the detector's mAP evaluation (DESIGN.md section 4 "mAP evaluation"), against which the
host build and the device kernels of csrc/y7t_map.h are checked.

  image_stats     the per-image statistics as the reference's test loop forms them, literally: a Python loop over target classes and a set of detected targets
  image_stats_rule  the parallel restatement the kernels implement (best same-class target, claim, first claimant in row order)
  ap_per_class    the reference's per-class AP with ONE change: np.argsort(-conf, kind='stable'), so that equal confidences keep their arrival order
  metrics         mp, mr, map50, map and the per-class maps from those arrays

float32 torch for the boxes (so that every operation rounds as the reference's does), float64 NumPy for the curves."""
import numpy as np
import torch

NIOU = 10


def iouv():
    return torch.linspace(0.5, 0.95, NIOU)


def xywh2xyxy(x):
    y = x.clone()
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def scale_coords(coords, lb):
    """in place, with ratio_pad: lb = (gain, padx, pady, h0, w0) as float32"""
    gain, padx, pady, h0, w0 = (float(v) for v in lb)
    coords[:, [0, 2]] -= padx
    coords[:, [1, 3]] -= pady
    coords[:, :4] /= gain
    coords[:, 0].clamp_(0, w0)
    coords[:, 1].clamp_(0, h0)
    coords[:, 2].clamp_(0, w0)
    coords[:, 3].clamp_(0, h0)
    return coords


def box_iou(box1, box2):
    def area(b):
        return (b[2] - b[0]) * (b[3] - b[1])
    a1, a2 = area(box1.T), area(box2.T)
    inter = (torch.min(box1[:, None, 2:], box2[:, 2:]) - torch.max(box1[:, None, :2], box2[:, :2])).clamp(0).prod(2)
    return inter / (a1[:, None] + a2 - inter)


def native_boxes(pred, labels, hw, lb):
    """pred (P, 6) [xyxy in network pixels, conf, cls], labels (T, 5) [cls, xywh normalised] -> (predn boxes (P, 4), tbox (T, 4)) in native pixels"""
    H, W = hw
    predn = pred[:, :4].clone().float()
    if len(predn):
        scale_coords(predn, lb)
    lab = labels.clone().float()
    lab[:, 1:5] *= torch.tensor([W, H, W, H], dtype=torch.float32)
    tbox = xywh2xyxy(lab[:, 1:5])
    if len(tbox):
        scale_coords(tbox, lb)
    return predn, tbox


def image_stats(pred, labels, hw, lb, box_iou_fn=box_iou):
    """one image, literally -> correct (P, 10) bool.  pred (P, 6) torch float32, labels (T, 5) torch float32"""
    thr = iouv()
    P, nl = len(pred), len(labels)
    correct = torch.zeros(P, NIOU, dtype=torch.bool)
    if not P or not nl:
        return correct
    predn, tbox = native_boxes(pred, labels, hw, lb)
    detected = []
    tcls = labels[:, 0]
    for cls in torch.unique(tcls):
        ti = (cls == tcls).nonzero(as_tuple=False).view(-1)
        pi = (cls == pred[:, 5]).nonzero(as_tuple=False).view(-1)
        if pi.shape[0]:
            ious, i = box_iou_fn(predn[pi], tbox[ti]).max(1)
            seen = set()
            for j in (ious > thr[0]).nonzero(as_tuple=False):
                d = ti[i[j]]
                if d.item() not in seen:
                    seen.add(d.item())
                    detected.append(d)
                    correct[pi[j]] = ious[j] > thr
                    if len(detected) == nl:
                        break
    return correct


def image_stats_rule(pred, labels, hw, lb):
    """the same, as the kernels state it"""
    thr = iouv().numpy()
    P, nl = len(pred), len(labels)
    correct = np.zeros((P, NIOU), bool)
    if not P or not nl:
        return torch.from_numpy(correct)
    predn, tbox = native_boxes(pred, labels, hw, lb)
    iou = box_iou(predn, tbox).numpy()
    same = pred[:, 5].numpy()[:, None] == labels[:, 0].numpy()[None, :]
    claimed = set()
    for p in range(P):
        cand = np.nonzero(same[p])[0]
        if not len(cand):
            continue
        t = cand[np.argmax(iou[p, cand])]      # (the first of equal maxima)
        if iou[p, t] > thr[0] and t not in claimed:
            claimed.add(t)
            correct[p] = iou[p, t] > thr
    return torch.from_numpy(correct)


def batch_stats(preds, targets, hw, lbs, fn=image_stats):
    """preds: list of (P_b, 6); targets (L, 6) [image, cls, xywh] -> (correct (N, 10) bool, conf (N,) f32, cls (N,) f32, tcls list), rows in image order"""
    cor, conf, cls, tcls = [], [], [], []
    for b, pred in enumerate(preds):
        labels = targets[targets[:, 0] == b, 1:]
        tcls += labels[:, 0].tolist()
        cor.append(fn(pred, labels, hw, lbs[b]).numpy())
        conf.append(pred[:, 4].numpy())
        cls.append(pred[:, 5].numpy())
    return (np.concatenate(cor, 0) if cor else np.zeros((0, NIOU), bool), np.concatenate(conf) if conf else np.zeros(0, np.float32),
            np.concatenate(cls) if cls else np.zeros(0, np.float32), tcls)


def compute_ap(recall, precision):
    mrec = np.concatenate(([0.], recall, [recall[-1] + 0.01]))
    mpre = np.concatenate(([1.], precision, [0.]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    y = np.interp(x, mrec, mpre)
    return ((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0).sum()      # np.trapz(y, x)


def ap_curves(tp, conf, pred_cls, target_cls):
    """-> (ap (nu, 10), p (nu, 1000), r (nu, 1000), unique classes) with the stable order"""
    i = np.argsort(-conf, kind='stable')
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes = np.unique(target_cls)
    nu = unique_classes.shape[0]
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nu, tp.shape[1])), np.zeros((nu, 1000)), np.zeros((nu, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = (target_cls == c).sum()
        if i.sum() == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + 1e-16)
        r[ci] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j])
    return ap, p, r, unique_classes.astype('int32')


def f1_pick(p, r):
    """(p, r) curves (nu, 1000) -> (p, r, f1 at the arg-max of the mean F1, that index), in NumPy's own order"""
    f1 = 2 * p * r / (p + r + 1e-16)
    i = f1.mean(0).argmax() if len(f1) else 0
    return p[:, i], r[:, i], f1[:, i], int(i)


def ap_per_class(tp, conf, pred_cls, target_cls):
    ap, p, r, classes = ap_curves(tp, conf, pred_cls, target_cls)
    p, r, f1, _ = f1_pick(p, r)
    return p, r, ap, f1, classes


def metrics(p, r, ap, ap_class, nc):
    """-> (mp, mr, map50, map), maps (nc,)"""
    if not len(ap_class):
        return (0.0, 0.0, 0.0, 0.0), np.zeros(nc)
    ap50, apm = ap[:, 0], ap.mean(1)
    mp, mr, map50, map_ = p.mean(), r.mean(), ap50.mean(), apm.mean()
    maps = np.zeros(nc) + map_
    for i, c in enumerate(ap_class):
        maps[c] = apm[i]
    return (mp, mr, map50, map_), maps
