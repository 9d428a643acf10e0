"""mAP evaluation of the detector on the device: what the reference's test.py does with a checkpoint (DESIGN.md section 4 "mAP evaluation").

The per-image statistics (test.py:126-209) and ap_per_class / compute_ap (utils/metrics.py:18-106) run in liby7t.so (y7t_map_update, y7t_map_compute;
csrc/y7t_map.h): no prediction row reaches the host.  What comes back from a compute is ap (nc, 10), the precision and recall curves (nc, 1000), the targets per
class and the classes that have targets; f1, the arg-max of its mean, mp, mr, map50 and map are host arithmetic on those arrays in NumPy's own order.

    python -m yolov7_tracker_amd.detector.evaluate --weights random:yolov7-tiny --data synthetic:8:40 --img-size 320 --batch-size 4
    python -m yolov7_tracker_amd.detector.evaluate --weights yolov7.pt --cfg yolov7 --data data/coco.yaml --img-size 640 --batch-size 32

Not built: the confusion matrix and the plots, --save-json / pycocotools, --save-txt / --save-hybrid and NMS `labels=`, single_cls, compute_loss, a
multi-GPU gather of the statistics.
"""
import argparse
import ctypes
import glob
import math
import os
import time

import numpy as np
import torch

from .. import _lib
from . import model as _model

NIOU = 10
MAX_PLANS = 4      # input sizes whose plans (arena, weights, post-processing sets) evaluate() keeps alive while it walks rect batches of many shapes


def finish(ap, p, r, classes):
    """device outputs -> what ap_per_class returns: (p, r, ap, f1, ap_class) at the arg-max of the mean F1 over the classes that have targets"""
    classes = np.asarray(classes, np.int64)
    ap, p, r = ap[classes], p[classes], r[classes]
    f1 = 2 * p * r / (p + r + 1e-16)
    i = f1.mean(0).argmax() if len(classes) else 0
    return p[:, i], r[:, i], ap, f1[:, i], classes.astype('int32')


def summarize(p, r, ap, ap_class, nc):
    """-> (mp, mr, map50, map), maps (nc,) as test.py:221-223, 281-283"""
    if not len(ap_class):
        return (0.0, 0.0, 0.0, 0.0), np.zeros(nc)
    ap50, apm = ap[:, 0], ap.mean(1)
    mp, mr, map50, map_ = p.mean(), r.mean(), ap50.mean(), apm.mean()
    maps = np.zeros(nc) + map_
    for i, c in enumerate(ap_class):
        maps[c] = apm[i]
    return (mp, mr, map50, map_), maps


def letterbox_rows(shapes, B, hw):
    """shapes[b]: (h0, w0), or test.py's ((h0, w0), ((rh, rw), (padx, pady))) -> (B, 5) float32 rows (gain, padx, pady, h0, w0): scale_coords' ratio_pad when given"""
    H, W = hw
    lb = np.zeros((B, 5), np.float32)
    for b in range(B):
        s = (H, W) if shapes is None else shapes[b]
        if len(s) == 2 and not np.isscalar(s[0]):
            (h0, w0), (ratio, pad) = s
            lb[b] = (ratio[0], pad[0], pad[1], h0, w0)
        else:
            h0, w0 = s[:2]
            gain = min(H / h0, W / w0)
            lb[b] = (gain, (W - w0 * gain) / 2, (H - h0 * gain) / 2, h0, w0)
    return lb


def group_targets(targets, B):
    """(L, 6) [image, class, x, y, w, h] -> (float32 rows grouped by image in their order, (B + 1) int32 offsets)"""
    t = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 6)
    img = t[:, 0].astype(np.int64)
    if len(t) and ((img < 0) | (img >= B)).any():
        raise ValueError("a target names image %d of a batch of %d" % (int(img[(img < 0) | (img >= B)][0]), B))
    if len(t) > 1 and (np.diff(img) < 0).any():
        t = t[np.argsort(img, kind="stable")]
        img = t[:, 0].astype(np.int64)
    off = np.searchsorted(img, np.arange(B + 1), side="left").astype(np.int32)
    return t, off


class DeviceMAP:
    """The statistics of an evaluation run, on the device.  update() is one asynchronous call per batch; compute() is the only read-back.
    cap_rows: the most prediction rows the run may store (300 an image at most); about 48 bytes of device memory a row."""

    def __init__(self, nc, cap_rows, conf_thres=0.001, iou_thres=0.65):
        _lib.require_gpu()
        self._L = _lib.load()
        self.nc, self.cap_rows = int(nc), int(cap_rows)
        self.conf_thres, self.iou_thres = float(conf_thres), float(iou_thres)
        n = int(self._L.y7t_map_bytes(self.cap_rows, self.nc))
        if n == 0:
            raise ValueError("DeviceMAP: cap_rows=%d, nc=%d out of range" % (self.cap_rows, self.nc))
        self.state = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.iouv = torch.linspace(0.5, 0.95, NIOU).cuda()
        off = (ctypes.c_size_t * 4)()
        _lib.check(self._L.y7t_map_layout(self.cap_rows, self.nc, off))
        self._off = dict(zip(("nt", "conf", "cls", "correct"), (int(v) for v in off)))
        self.reset()

    def reset(self):
        _lib.check(self._L.y7t_map_init(_lib.ptr(self.state), self.state.numel(), self.cap_rows, self.nc, _lib.stream_ptr()))

    def __del__(self):
        try:
            self._L.y7t_map_release(_lib.ptr(self.state))
        except Exception:
            pass

    # -- views of the state (tests, inspection: each is a device tensor, reading it is the caller's synchronisation) --
    def header(self):
        """int32 device view: [rows, images seen, status, ...]"""
        return self.state[:256].view(torch.int32)

    def rows(self):
        """-> (conf (n,) float32, cls (n,) int32, correct (n, 10) bool, nt (nc,) int64) on the host"""
        n = int(self.header()[0].item())
        v = lambda k, dt: self.state[self._off[k]:self._off[k] + 4 * self.cap_rows].view(dt)[:n].cpu().numpy()
        mask = v("correct", torch.int32)
        nt = self.state[self._off["nt"]:self._off["nt"] + 8 * self.nc].view(torch.int64).cpu().numpy()
        return v("conf", torch.float32), v("cls", torch.int32), ((mask[:, None] >> np.arange(NIOU)) & 1).astype(bool), nt

    def _set_of(self, detector, dets):
        for ps, cap in [(ps, detector.max_cand) for ps in detector.plan.post] + [(a, a.cap) for a in detector._aug.values()]:
            if ps.dets.data_ptr() == dets.data_ptr():
                return ps, cap
        raise _lib.Y7TError("DeviceMAP.update: these detections are not the output of this detector's current post-processing sets")

    def update(self, detector, out_or_dets, targets, shapes=None, img_shape=None):
        """One batch.  out_or_dets: the HeadOutput / AugmentedOutput of a forward -- it is post-processed here at (conf_thres, iou_thres), multi-label as test.py:122
        where the forward allows it (per-class scores exist: a plain, un-fused forward), the best-class form otherwise -- or the (dets, ndets) a
        Detector.postprocess of this detector just returned (then img_shape = the batch's (H, W)).  targets: (L, 6) [image, class, x, y, w, h] normalised to the
        letterboxed batch, as the reference's loader gives them.  shapes[b]: test.py's ((h0, w0), ((rh, rw), (padx, pady))) or (h0, w0); None: the batch's own
        size.  The boxes matched are the candidates' un-rounded ones, gathered by `keep` on the device.  Asynchronous; -> (dets, ndets)."""
        if isinstance(out_or_dets, _model.HeadOutput):
            out = out_or_dets
            aug = isinstance(out, _model.AugmentedOutput)
            ml = (not aug) and out.fused is None
            conf = out.fused if out.fused is not None else self.conf_thres
            dets, nd = detector.postprocess(out, conf, self.iou_thres, None, multi_label=ml)
            B, hw = out.B, out.img_shape
        else:
            dets, nd = out_or_dets
            if img_shape is None:
                raise ValueError("DeviceMAP.update((dets, ndets), ...) needs img_shape=(H, W) of the batch")
            hw = tuple(img_shape)
            B = len(shapes) if shapes is not None else int(nd.shape[0])
        ps, cap = self._set_of(detector, dets)
        t, off = group_targets(targets, B)
        lb = letterbox_rows(shapes, B, hw)
        # one small upload: [targets | offsets | lb], 256-byte aligned pieces
        rup = lambda n: (n + 255) // 256 * 256
        o1 = rup(max(t.nbytes, 4)); o2 = o1 + rup(off.nbytes)
        host = np.zeros(o2 + rup(lb.nbytes), np.uint8)
        host[:t.nbytes] = t.view(np.uint8).reshape(-1)
        host[o1:o1 + off.nbytes] = off.view(np.uint8)
        host[o2:o2 + lb.nbytes] = lb.view(np.uint8).reshape(-1)
        dev = torch.from_numpy(host).pin_memory().cuda(non_blocking=True)
        self.update_arrays(dets, nd, ps.keep, ps.ws, cap, cap, B, dev[:o1], dev[o1:o2], hw, dev[o2:])
        self._upload_keep = dev      # (alive until the next update's launches are behind this one's on the stream)
        return dets, nd

    def update_arrays(self, dets, ndets, keep, cand_boxes, cand_rows, cand_stride, B, targets, target_offsets, hw, lb):
        """y7t_map_update on device tensors, as include/y7t.h lays them out"""
        _lib.check(self._L.y7t_map_update(_lib.ptr(self.state), _lib.ptr(dets), _lib.ptr(ndets), _lib.ptr(keep), _lib.ptr(cand_boxes), int(cand_rows), int(cand_stride),
                                          int(B), int(dets.shape[1]), _lib.ptr(targets), _lib.ptr(target_offsets), int(hw[0]), int(hw[1]), _lib.ptr(lb),
                                          _lib.ptr(self.iouv), _lib.stream_ptr()))

    def compute_raw(self):
        """-> dict(ap (nc, 10), p, r (nc, 1000), nt (nc,), classes, rows, seen, status): the device outputs on the host"""
        ap = torch.empty((self.nc, NIOU), dtype=torch.float64, device="cuda")
        p = torch.empty((self.nc, 1000), dtype=torch.float64, device="cuda")
        r = torch.empty((self.nc, 1000), dtype=torch.float64, device="cuda")
        nt = torch.empty(self.nc, dtype=torch.int64, device="cuda")
        cl = torch.empty(self.nc, dtype=torch.int32, device="cuda")
        info = torch.empty(4, dtype=torch.int32, device="cuda")
        _lib.check(self._L.y7t_map_compute(_lib.ptr(self.state), _lib.ptr(ap), _lib.ptr(p), _lib.ptr(r), _lib.ptr(nt), _lib.ptr(cl), _lib.ptr(info), _lib.stream_ptr()))
        info = info.cpu().numpy()
        return dict(ap=ap.cpu().numpy(), p=p.cpu().numpy(), r=r.cpu().numpy(), nt=nt.cpu().numpy(), classes=cl.cpu().numpy()[:int(info[3])], rows=int(info[0]),
                    seen=int(info[1]), status=int(info[2]))

    def compute(self):
        """-> (p, r, ap, f1, ap_class, nt) -- ap_per_class's tuple over everything stored so far, plus the targets per class.  Raises when an update overflowed
        cap_rows: the statistics would be those of a part of the run."""
        raw = self.compute_raw()
        if raw["status"] & 1:
            raise _lib.Y7TError("DeviceMAP: an update passed cap_rows=%d and stored nothing; size the state for the run" % self.cap_rows)
        self.seen = raw["seen"]
        return finish(raw["ap"], raw["p"], raw["r"], raw["classes"]) + (raw["nt"],)


# ---- data ----
def synthetic_batches(n_images=8, n_obj=40, size=320, batch_size=4, seq_idx=0):
    """frames and labels of synth.make_frames' scene, batched as test.py's loader hands them over: (img uint8 (B, 3, H, W) RGB, targets (L, 6), paths, shapes)"""
    from .. import synth
    frames = synth.make_frames(n_images, n_obj, size, seq_idx)
    labels = synth.make_frame_labels(n_images, n_obj, size, seq_idx)
    for i in range(0, n_images, batch_size):
        fr = frames[i:i + batch_size]
        img = torch.from_numpy(np.ascontiguousarray(fr[..., ::-1].transpose(0, 3, 1, 2)))
        t = [np.concatenate([np.full((len(l), 1), b, np.float32), l], 1) for b, l in enumerate(labels[i:i + batch_size])]
        shapes = [((size, size), ((1.0, 1.0), (0.0, 0.0)))] * len(fr)
        yield img, torch.from_numpy(np.concatenate(t, 0)), ["synthetic_%06d" % (i + b) for b in range(len(fr))], shapes


IMG_FORMATS = ('bmp', 'jpg', 'jpeg', 'png', 'tif', 'tiff', 'dng', 'webp', 'mpo')


def list_images(path):
    """a directory (searched recursively) or a list file whose relative lines are taken from the file's folder, as utils/datasets.py:366-380"""
    out = []
    for p in (path if isinstance(path, list) else [path]):
        if os.path.isdir(p):
            out += glob.glob(os.path.join(p, "**", "*.*"), recursive=True)
        elif os.path.isfile(p):
            parent = os.path.dirname(os.path.abspath(p)) + os.sep
            with open(p) as f:
                out += [x.replace("./", parent, 1) if x.startswith("./") else x for x in f.read().strip().splitlines()]
        else:
            raise FileNotFoundError("%s does not exist" % p)
    return sorted(x for x in out if x.split(".")[-1].lower() in IMG_FORMATS)


def label_path(img_path):
    sa, sb = os.sep + "images" + os.sep, os.sep + "labels" + os.sep
    return "txt".join(img_path.replace(sa, sb, 1).rsplit(img_path.split(".")[-1], 1))


def rect_batch_shapes(hw0, img_size, batch_size, stride, pad=0.5):
    """utils/datasets.py:413-438 (rect=True): hw0 (n, 2) native (h, w) -> (order by aspect ratio, batch index of every sorted image, (nb, 2) batch (H, W))"""
    hw0 = np.asarray(hw0, np.float64)
    ar = hw0[:, 0] / hw0[:, 1]
    order = ar.argsort()
    ar = ar[order]
    bi = np.floor(np.arange(len(ar)) / batch_size).astype(int)
    shapes = []
    for i in range(bi[-1] + 1):
        ari = ar[bi == i]
        mini, maxi = ari.min(), ari.max()
        shapes.append([maxi, 1] if maxi < 1 else ([1, 1 / mini] if mini > 1 else [1, 1]))
    return order, bi, np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride


def yaml_batches(data, task="val", img_size=640, batch_size=32, stride=32):
    """the reference's loader for test.py (rect=True, pad=0.5, no augmentation) over a data dict: images decoded with PIL, the long side resized to img_size,
    letterboxed to the batch's shape (scaleup off), labels moved with the image.  Yields (img uint8 (B, 3, H, W) RGB, targets (L, 6), paths, shapes)."""
    from PIL import Image
    from ..tracker.tracker_dataloader import _resize_linear, letterbox
    files = list_images(data[task])
    if not files:
        raise FileNotFoundError("no images under %r" % (data[task],))
    sizes = []
    for f in files:
        with Image.open(f) as im:
            sizes.append((im.size[1], im.size[0]))
    order, bi, batch_shapes = rect_batch_shapes(sizes, img_size, batch_size, stride)
    files = [files[i] for i in order]
    for k in range(bi[-1] + 1):
        idx = np.nonzero(bi == k)[0]
        H, W = (int(v) for v in batch_shapes[k])
        imgs, tg, shapes = [], [], []
        for b, i in enumerate(idx):
            img = np.asarray(Image.open(files[i]).convert("RGB"))[:, :, ::-1]      # BGR like cv2.imread
            h0, w0 = img.shape[:2]
            r = img_size / max(h0, w0)
            if r != 1:
                img = _resize_linear(img, int(h0 * r), int(w0 * r))
            h, w = img.shape[:2]
            img, ratio, pad = letterbox(img, (H, W), auto=False, scaleup=False)
            lp = label_path(files[i])
            lab = np.zeros((0, 5), np.float32)
            if os.path.isfile(lp):
                with open(lp) as f:
                    rows = [x.split() for x in f.read().strip().splitlines() if x.strip()]
                if rows:
                    lab = np.unique(np.array(rows, np.float32).reshape(-1, 5), axis=0)
            if len(lab):      # normalised xywh of the native image -> pixels of the letterboxed one -> normalised xywh of it (utils/datasets.py:583-612)
                x = lab[:, 1:].copy()
                x1 = ratio[0] * w * (x[:, 0] - x[:, 2] / 2) + pad[0]
                y1 = ratio[1] * h * (x[:, 1] - x[:, 3] / 2) + pad[1]
                x2 = ratio[0] * w * (x[:, 0] + x[:, 2] / 2) + pad[0]
                y2 = ratio[1] * h * (x[:, 1] + x[:, 3] / 2) + pad[1]
                lab[:, 1] = (x1 + x2) / 2 / img.shape[1]
                lab[:, 2] = (y1 + y2) / 2 / img.shape[0]
                lab[:, 3] = (x2 - x1) / img.shape[1]
                lab[:, 4] = (y2 - y1) / img.shape[0]
            imgs.append(np.ascontiguousarray(img[:, :, ::-1].transpose(2, 0, 1)))
            tg.append(np.concatenate([np.full((len(lab), 1), b, np.float32), lab], 1))
            shapes.append(((h0, w0), ((h / h0, w / w0), pad)))
        yield torch.from_numpy(np.stack(imgs)), torch.from_numpy(np.concatenate(tg, 0)), [files[i] for i in idx], shapes


def _bound_plans(det, limit=MAX_PLANS):
    """keep at most `limit` input sizes alive in the detector: the oldest plans other than the current one are destroyed, with the augmented sets of their size"""
    if len(det._plans) <= limit:
        return
    torch.cuda.synchronize()      # (nothing of a plan may still be in flight when its arena goes)
    for hw in list(det._plans):
        if len(det._plans) <= limit:
            break
        plan = det._plans[hw]
        if plan is det.plan:
            continue
        _lib.check(det._L.y7t_det_destroy(plan.handle))
        del det._plans[hw]
        for key in [k for k in det._aug if k[0] == hw or hw in k[1]]:
            del det._aug[key]


def evaluate(detector, batches, nc=None, conf_thres=0.001, iou_thres=0.65, augment=False, verbose=False, names=None, cap_rows=None, dmap=None, update=True,
             print_fn=print, max_plans=MAX_PLANS):
    """test.py's test() for a Detector: -> (mp, mr, map50, map, 0, 0, 0), maps, t.  The loss terms are zero: no loss is computed.  batches yields test.py's
    (img, targets, paths, shapes), img uint8 or float (B, 3, H, W) RGB.  Multi-label NMS as test.py:122 on a plain forward, the best-class form under augment.
    t = (forward, NMS + statistics, total) milliseconds an image from stream events (no synchronisation inside the loop), then the batch's size.
    update=False runs the loop without the statistics call (timing: scripts/time_map.py).  Rect batches of many shapes: at most `max_plans` plans stay alive."""
    nc = int(nc if nc is not None else detector.spec["nc"])
    names = names if names is not None else detector.names
    batches = iter(batches)
    first = next(batches, None)
    if first is None:
        raise ValueError("evaluate: no batches")
    if dmap is None:
        dmap = DeviceMAP(nc, cap_rows if cap_rows is not None else 1 << 20, conf_thres, iou_thres)
    else:
        dmap.reset()
    ev, seen, bs, hw = [], 0, first[0].shape[0], tuple(first[0].shape[2:])
    import itertools
    t_wall = time.time()
    for img, targets, paths, shapes in itertools.chain([first], batches):
        if img.dtype == torch.uint8:
            img = img.cuda(non_blocking=True).float() / 255.0
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        out = detector.forward_augment(img, conf_thres=conf_thres) if augment else detector.forward(img)
        e[1].record()
        if update:
            dmap.update(detector, out, targets, shapes)
        else:
            detector.postprocess(out, conf_thres, iou_thres, None, multi_label=not augment)
        e[2].record()
        ev.append(e)
        seen += img.shape[0]
        _bound_plans(detector, max_plans)
    torch.cuda.synchronize()
    t_wall = time.time() - t_wall
    t0 = sum(e[0].elapsed_time(e[1]) for e in ev)
    t1 = sum(e[1].elapsed_time(e[2]) for e in ev)
    if update:
        p, r, ap, f1, ap_class, nt = dmap.compute()
    else:
        p = r = f1 = np.zeros(0); ap = np.zeros((0, NIOU)); ap_class = np.zeros(0, 'int32'); nt = np.zeros(nc, np.int64)
    (mp, mr, map50, map_), maps = summarize(p, r, ap, ap_class, nc)
    pf = '%20s' + '%12i' * 2 + '%12.3g' * 4
    print_fn(('%20s' + '%12s' * 6) % ('Class', 'Images', 'Labels', 'P', 'R', 'mAP@.5', 'mAP@.5:.95'))
    print_fn(pf % ('all', seen, nt.sum(), mp, mr, map50, map_))
    if (verbose or nc < 50) and nc > 1:
        for i, c in enumerate(ap_class):
            print_fn(pf % (names[c], seen, nt[c], p[i], r[i], ap[i, 0], ap[i].mean()))
    t = tuple(x / max(seen, 1) for x in (t0, t1, t0 + t1)) + (hw[0], hw[1], bs)
    print_fn('Speed: %.1f/%.1f/%.1f ms inference/NMS/total per %gx%g image at batch-size %g' % t)
    evaluate.last = dict(seen=seen, wall_s=t_wall, nt=nt, ap_class=ap_class, p=p, r=r, ap=ap, f1=f1, dmap=dmap)      # (the state stays readable: DeviceMAP.rows)
    return (mp, mr, map50, map_, 0.0, 0.0, 0.0), maps, t


def parse_synthetic(spec):
    parts = spec.split(":")
    return (int(parts[1]) if len(parts) > 1 and parts[1] else 8), (int(parts[2]) if len(parts) > 2 and parts[2] else 40)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m yolov7_tracker_amd.detector.evaluate", description="mAP of a detector checkpoint, as the reference's test.py")
    ap.add_argument('--weights', nargs='+', type=str, default=['yolov7.pt'], help="model.pt path, or random:<arch>[:seed]")
    ap.add_argument('--cfg', type=str, default=None, help="model yaml or arch name, for a state-dict checkpoint")
    ap.add_argument('--data', type=str, default='data/coco.yaml', help="data yaml, or synthetic[:images[:objects]]")
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--img-size', type=int, default=640)
    ap.add_argument('--conf-thres', type=float, default=0.001)
    ap.add_argument('--iou-thres', type=float, default=0.65)
    ap.add_argument('--task', default='val', help="val, test or train: the key of the data yaml")
    ap.add_argument('--augment', action='store_true', help="augmented inference (best-class NMS over the union of the passes)")
    ap.add_argument('--verbose', action='store_true', help="report mAP by class")
    ap.add_argument('--cap-rows', type=int, default=0, help="prediction rows the device state holds (default: 300 an image)")
    ap.add_argument('--plant-objectness', type=int, default=0, help="random weights only: shift the Detect biases so that about this many anchors pass (Detector.plant_objectness_bias)")
    opt = ap.parse_args(argv)
    torch.cuda.set_device(0)
    if opt.data.startswith("synthetic"):
        n_img, n_obj = parse_synthetic(opt.data)
        nc, names = 80, None
        spec, sd, seed = _model.load_checkpoint(opt.weights, opt.cfg, nc)
        size = opt.img_size
        mk = lambda: synthetic_batches(n_img, n_obj, size, opt.batch_size)
        n_total = n_img
    else:
        import yaml
        with open(opt.data) as f:
            data = yaml.safe_load(f)
        nc, names = int(data['nc']), data.get('names')
        spec, sd, seed = _model.load_checkpoint(opt.weights, opt.cfg, nc)
        gs = int(max(8 * 2 ** (len(spec["anchors"]) - 1), 32))
        size = int(math.ceil(opt.img_size / gs) * gs)      # check_img_size
        mk = lambda: yaml_batches(data, opt.task, size, opt.batch_size, gs)
        n_total = len(list_images(data[opt.task]))
    first = next(iter(mk()))
    det = _model.Detector(spec, sd, img_size=tuple(first[0].shape[2:]), max_batch=opt.batch_size, seed=seed)
    if opt.plant_objectness:
        det.plant_objectness_bias(first[0][:1].float() / 255.0, target=opt.plant_objectness)
    res = evaluate(det, mk(), nc, opt.conf_thres, opt.iou_thres, opt.augment, opt.verbose, names, opt.cap_rows or 300 * n_total)
    return res


if __name__ == "__main__":
    main()
