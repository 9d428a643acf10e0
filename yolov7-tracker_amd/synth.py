"""Deterministic synthetic workloads for the tracking hot path.

No dataset or trained checkpoint ships with the reference, so every parity test and
benchmark in this repo runs on seeded synthetic sequences:

* `make_detections` -- ground-truth rectangles moving with constant velocity + jitter,
  emitted at the tracker's `(N, 6)` seam `[x1, y1, x2, y2, conf, cls]` exactly as
  `post_process_v7` hands them over (integer-rounded corners, float32;
  /root/reference/tracker/track.py:234-244).
* `make_frames` -- uint8 BGR frames of VisDrone-like shape for the detector.
* `make_camera_frames` -- uint8 BGR frames of an analytic textured scene under a moving camera, with the planted
  per-frame Euclidean warps (the camera-motion estimate's input and ground truth).
"""
import numpy as np

BASE_SEED = 20260924


def _tracks(rng, n_obj, size):
    w = np.clip(rng.lognormal(np.log(30.0), 0.5, n_obj), 8, 300)
    h = np.clip(rng.lognormal(np.log(30.0), 0.5, n_obj) * 1.6, 8, 300)
    cx = rng.uniform(0.05 * size, 0.95 * size, n_obj)
    cy = rng.uniform(0.05 * size, 0.95 * size, n_obj)
    vx = rng.normal(0, 2.0, n_obj)
    vy = rng.normal(0, 2.0, n_obj)
    cls = rng.integers(0, 10, n_obj)
    conf0 = rng.uniform(0.1, 0.95, n_obj)
    return cx, cy, w, h, vx, vy, cls, conf0


_FEAT_DIM = 128


def make_detections(n_frames=100, n_obj=80, size=1280, seq_idx=0, miss=0.10, fp=0.05, conf_jitter=0.05, ground_truth=None, bounce=False):
    """-> list of float32 (N_t, 6) arrays, one per frame.  `ground_truth`: a list that receives, per frame, the float64
    (n, 7) rows `[id (1-based), x, y, w, h, cls, detected]` of the true rectangles (clipped to the image; objects that left it
    are dropped) -- what make_ground_truth returns.  bounce=True: objects are reflected at the image border instead of leaving
    (long sequences keep ~n_obj objects per frame: bench.py; the default keeps the generator the golden sequences were recorded
    with: there the constant-velocity objects drift out, ~27 of 80 left after 800 frames)."""
    rng = np.random.default_rng(BASE_SEED + seq_idx)
    cx, cy, w, h, vx, vy, cls, conf0 = _tracks(rng, n_obj, size)
    out = []
    for _ in range(n_frames):
        cx = cx + vx
        cy = cy + vy
        if bounce:
            for c, v in ((cx, vx), (cy, vy)):
                lo, hi = c < 0.02 * size, c > 0.98 * size
                v[lo] = np.abs(v[lo])
                v[hi] = -np.abs(v[hi])
        if ground_truth is not None:
            gx1, gy1 = np.clip(cx - w / 2, 0, size), np.clip(cy - h / 2, 0, size)
            gx2, gy2 = np.clip(cx + w / 2, 0, size), np.clip(cy + h / 2, 0, size)
            vis = (gx2 - gx1 >= 2) & (gy2 - gy1 >= 2)
            gt_rows = np.stack([np.arange(1, n_obj + 1, dtype=np.float64), gx1, gy1, gx2 - gx1, gy2 - gy1, cls.astype(np.float64),
                                np.zeros(n_obj)], 1)
        jx = rng.normal(0, 0.5, n_obj)
        jy = rng.normal(0, 0.5, n_obj)
        keep = rng.random(n_obj) >= miss
        x1 = cx + jx - w / 2
        y1 = cy + jy - h / 2
        x2 = x1 + w
        y2 = y1 + h
        conf = np.clip(conf0 + rng.normal(0, conf_jitter, n_obj), 0.02, 0.99)
        rows = np.stack([x1, y1, x2, y2, conf, cls.astype(np.float64)], 1)[keep]
        if ground_truth is not None:
            gt_rows[:, 6] = keep
            ground_truth.append(gt_rows[vis])
        n_fp = rng.binomial(n_obj, fp)
        if n_fp:
            fw = np.clip(rng.lognormal(np.log(30.0), 0.5, n_fp), 8, 300)
            fh = np.clip(rng.lognormal(np.log(30.0), 0.5, n_fp) * 1.6, 8, 300)
            fx = rng.uniform(0, size - 8, n_fp)
            fy = rng.uniform(0, size - 8, n_fp)
            fr = np.stack([fx, fy, fx + fw, fy + fh, rng.uniform(0.1, 0.95, n_fp),
                           rng.integers(0, 10, n_fp).astype(np.float64)], 1)
            rows = np.concatenate([rows, fr], 0)
        rows[:, :4] = np.clip(np.round(rows[:, :4]), 0, size)
        ok = (rows[:, 2] - rows[:, 0] >= 2) & (rows[:, 3] - rows[:, 1] >= 2)
        rows = rows[ok]
        # reject exact duplicate boxes so assignment optima stay unique
        _, first = np.unique(rows[:, :4], axis=0, return_index=True)
        rows = rows[np.sort(first)]
        # the detector hands rows over sorted by confidence (NMS output order)
        rows = rows[np.argsort(-rows[:, 4], kind="stable")]
        out.append(rows.astype(np.float32))
    return out



def make_features(boxes, seed=0, dim=_FEAT_DIM):
    """Deterministic stand-in for a ReID embedding at DeepSORT's `get_feature(tlbrs, ori_img)` seam (tracker/deepsort.py:19-41; no
    ReID checkpoint ships with the reference, weights/ckpt.t7): a fixed random projection of what stays constant for an object in
    these scenes -- its box width and height -- through a few non-linear terms to a unit vector of dimension `dim` (128), float32.
    boxes: (N, >=4) [x1, y1, x2, y2, ...]."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(len(boxes), -1)
    rng = np.random.default_rng(BASE_SEED + 1000 + seed)
    proj = rng.normal(0, 1, (6, dim)).astype(np.float32)
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    code = np.stack([w / 32.0, h / 32.0, np.sqrt(np.maximum(w * h, 0)) / 32.0, w / np.maximum(h, 1.0), np.sin(w / 7.0), np.cos(h / 9.0)], 1).astype(np.float32)
    f = code @ proj
    return (f / np.maximum(np.linalg.norm(f, axis=1, keepdims=True), 1e-12)).astype(np.float32)


def make_identity_features(n_frames=60, n_obj=60, size=1280, seq_idx=0, dim=128, noise=0.15, **kw):
    """A scene whose appearance features IDENTIFY the object (what a ReID network delivers): -> (dets, feature_fn).  Every detection of object k
    gets unit(base_k + noise * N(0, 1)), false positives a random unit vector; feature_fn(boxes) looks the vectors up by the box (the seam
    DeepSORT.get_feature(tlbrs, ori_img) only sees boxes).  With such features a detection is an appearance candidate of ONE track, which is
    when the matching cascade's levels do not compete for detections."""
    gt = []
    dets = make_detections(n_frames, n_obj, size, seq_idx, ground_truth=gt, **kw)
    rng = np.random.default_rng(BASE_SEED + 2000 + seq_idx)
    base = rng.normal(0, 1, (n_obj + 1, dim)).astype(np.float32)
    table = {}
    for d, g in zip(dets, gt):
        f = rng.normal(0, 1, (len(d), dim)).astype(np.float32)
        if len(g) and len(d):
            gc = np.stack([g[:, 1] + g[:, 3] / 2, g[:, 2] + g[:, 4] / 2], 1)
            dc = np.stack([(d[:, 0] + d[:, 2]) / 2, (d[:, 1] + d[:, 3]) / 2], 1)
            dist = np.abs(dc[:, None, :] - gc[None, :, :]).max(2)
            j = dist.argmin(1)
            hit = dist[np.arange(len(d)), j] < 4.0
            f[hit] = base[g[j[hit], 0].astype(int)] + np.float32(noise) * f[hit]
        f = (f / np.maximum(np.linalg.norm(f, axis=1, keepdims=True), 1e-12)).astype(np.float32)
        for row, v in zip(d, f):
            table[tuple(float(x) for x in row[:4])] = v

    def feature_fn(boxes):
        boxes = np.asarray(boxes, dtype=np.float32).reshape(len(boxes), -1)
        return np.stack([table[tuple(float(x) for x in b[:4])] for b in boxes]) if len(boxes) else np.zeros((0, dim), np.float32)
    return dets, feature_fn


def make_ground_truth(n_frames=100, n_obj=80, size=1280, seq_idx=0, **kw):
    """ground truth of the sequence make_detections(...) observes: per frame float64 (n, 7) `[id, x, y, w, h, cls, detected]`"""
    gt = []
    make_detections(n_frames, n_obj, size, seq_idx, ground_truth=gt, **kw)
    return gt


def write_mot_gt(path, gt, single_class=True):
    """MOTChallenge gt.txt: frame,id,x,y,w,h,conf(1 = evaluate),class,visibility (class 1 = pedestrian when single_class)"""
    with open(path, "w") as f:
        for t, rows in enumerate(gt):
            for r in rows:
                f.write("%d,%d,%.2f,%.2f,%.2f,%.2f,1,%d,1.0\n" % (t + 1, int(r[0]), r[1], r[2], r[3], r[4], 1 if single_class else int(r[5]) + 1))


def make_frames(n_frames=4, n_obj=80, size=1280, seq_idx=0):
    """-> uint8 (n_frames, size, size, 3) BGR frames: smooth background + moving filled rectangles."""
    rng = np.random.default_rng(BASE_SEED + 1000 + seq_idx)
    cx, cy, w, h, vx, vy, cls, _ = _tracks(rng, n_obj, size)
    colors = rng.integers(0, 256, (n_obj, 3))
    coarse = rng.integers(60, 200, (40, 40, 3)).astype(np.float32)
    rep = size // 40 + 1
    bg = np.kron(coarse, np.ones((rep, rep, 1), np.float32))[:size, :size]
    # cheap separable box blur to make it low-frequency
    k = max(rep // 2, 1)
    bg = (bg + np.roll(bg, k, 0) + np.roll(bg, -k, 0) + np.roll(bg, k, 1) + np.roll(bg, -k, 1)) / 5.0
    frames = np.empty((n_frames, size, size, 3), np.uint8)
    for t in range(n_frames):
        cx = cx + vx
        cy = cy + vy
        img = bg.copy()
        for i in range(n_obj):
            x1 = int(np.clip(cx[i] - w[i] / 2, 0, size - 1))
            y1 = int(np.clip(cy[i] - h[i] / 2, 0, size - 1))
            x2 = int(np.clip(cx[i] + w[i] / 2, x1 + 1, size))
            y2 = int(np.clip(cy[i] + h[i] / 2, y1 + 1, size))
            img[y1:y2, x1:x2] = colors[i]
        frames[t] = img.astype(np.uint8)
    return frames


def make_frame_labels(n_frames=4, n_obj=80, size=1280, seq_idx=0):
    """the rectangles make_frames(...) paints, as detector labels: per frame float32 (n, 5) rows [class, x, y, w, h], centre and size normalised by `size`
    (the reference's label files), for the rectangles of which at least 2 x 2 pixels lie inside the frame"""
    rng = np.random.default_rng(BASE_SEED + 1000 + seq_idx)
    cx, cy, w, h, vx, vy, cls, _ = _tracks(rng, n_obj, size)
    out = []
    for _ in range(n_frames):
        cx = cx + vx
        cy = cy + vy
        x1, y1 = np.clip(cx - w / 2, 0, size), np.clip(cy - h / 2, 0, size)
        x2, y2 = np.clip(cx + w / 2, 0, size), np.clip(cy + h / 2, 0, size)
        vis = (x2 - x1 >= 2) & (y2 - y1 >= 2)
        rows = np.stack([cls.astype(np.float64), (x1 + x2) / 2 / size, (y1 + y2) / 2 / size, (x2 - x1) / size, (y2 - y1) / size], 1)[vis]
        out.append(rows.astype(np.float32))
    return out


def make_warps(n_frames=100, seq_idx=0, rot=0.002, shift=2.0):
    """-> (n_frames, 2, 3) float64 camera-motion matrices near the identity (what BoT-SORT's GMC.apply would estimate from
    ORB matches, /root/reference/tracker/botsort.py:13-248 -- the estimation itself is OpenCV and out of scope)."""
    rng = np.random.default_rng(BASE_SEED + 5000 + seq_idx)
    H = np.zeros((n_frames, 2, 3))
    H[:, :2, :2] = np.eye(2) + rng.normal(0, rot, (n_frames, 2, 2))
    H[:, :, 2] = rng.normal(0, shift, (n_frames, 2))
    return H


# ---- frames under a moving camera (the input of the camera-motion estimate, tracker/gmc.py) ----
_BG_TERMS = 12


def camera_background(x, y, seq_idx=0):
    """-> (..., 3) float64 BGR levels of the analytic scene of sequence `seq_idx` at the (real-valued) scene coordinates x, y: 128 plus a seeded sum of
    12 sinusoids with wavelengths of 8 - 200 px, mixed differently into the three channels.  Analytic, so a frame under any warp is EVALUATED, never
    interpolated."""
    rng = np.random.default_rng(BASE_SEED + 7000 + seq_idx)
    lam = np.exp(rng.uniform(np.log(8.0), np.log(200.0), _BG_TERMS))
    phi = rng.uniform(0.0, np.pi, _BG_TERMS)
    psi = rng.uniform(0.0, 2.0 * np.pi, _BG_TERMS)
    mix = rng.uniform(0.5, 1.0, (3, _BG_TERMS)) * np.sqrt(lam / lam.max())[None, :]      # longer waves carry more contrast, like natural footage
    mix *= 90.0 / mix.sum(axis=1, keepdims=True)                                          # |level - 128| <= 90: no clipping
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.full(x.shape + (3,), 128.0)
    for k in range(_BG_TERMS):
        wave = np.sin((2.0 * np.pi / lam[k]) * (x * np.cos(phi[k]) + y * np.sin(phi[k])) + psi[k])
        out += wave[..., None] * mix[:, k]
    return out


def euclidean_warp(theta, tx, ty):
    """-> (2, 3) float64 [[cos, -sin, tx], [sin, cos, ty]]"""
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty]], np.float64)


def render_camera_frame(size, pose, seq_idx=0):
    """-> uint8 (H, W, 3) BGR frame whose pixel X shows the scene at pose @ [X, 1] (pose: (2, 3)); size = side or (H, W); levels rounded half up"""
    H, W = (size, size) if np.isscalar(size) else (int(size[0]), int(size[1]))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    sx = pose[0, 0] * xs + pose[0, 1] * ys + pose[0, 2]
    sy = pose[1, 0] * xs + pose[1, 1] * ys + pose[1, 2]
    return np.clip(np.floor(camera_background(sx, sy, seq_idx) + 0.5), 0, 255).astype(np.uint8)


def make_camera_frames(n_frames=8, size=1280, seq_idx=0, rot=0.004, shift=1.5):
    """-> (frames uint8 (n_frames, H, W, 3) BGR, warps float64 (n_frames, 2, 3)): the analytic scene of camera_background seen by a camera that moves by a
    seeded Euclidean step per frame (rotation ~ N(0, rot) rad, translation ~ N(0, shift) px, clipped at 2 sigma).  warps[t] is the PLANTED motion from frame
    t - 1 to frame t in full-resolution pixel coordinates -- frame_t(warps[t] @ [X, 1]) shows what frame_{t-1}(X) shows, which is the matrix GMC.apply
    estimates (template = previous frame) -- and warps[0] is the identity.  size = side or (H, W)."""
    rng = np.random.default_rng(BASE_SEED + 7500 + seq_idx)
    pose = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])      # frame pixel -> scene
    frames, warps = [], np.zeros((n_frames, 2, 3))
    for t in range(n_frames):
        if t == 0:
            step = np.eye(3)
        else:
            th = float(np.clip(rng.normal(0.0, rot), -2 * rot, 2 * rot))
            tr = np.clip(rng.normal(0.0, shift, 2), -2 * shift, 2 * shift)
            step = np.vstack([euclidean_warp(th, tr[0], tr[1]), [0.0, 0.0, 1.0]])
        warps[t] = step[:2]
        pose = pose @ np.linalg.inv(step)                                        # pose_t = pose_{t-1} W_t^-1
        frames.append(render_camera_frame(size, pose[:2], seq_idx))
    return np.stack(frames), warps


# ---- frames with corners (the input of the feature-based estimate, GMC('features')): the sinusoid scene is too smooth for FAST at threshold 20 ----
def corner_scene(x, y, extent, seq_idx=0, per_kilopixel=3.0, sides=(6.0, 28.0)):
    """-> (..., 3) float64 BGR levels at the (real-valued) scene coordinates x, y: camera_background with a seeded set of rotated rectangles of random grey levels
    painted over it in order, their centres spread over extent = (H, W) and a margin around it, `per_kilopixel` of them per 1000 square pixels, half-sides drawn
    from sides / 2.  A point is inside a rectangle by an analytic test at its own coordinates, so a frame under any warp is EVALUATED, never interpolated."""
    H, W = float(extent[0]), float(extent[1])
    rng = np.random.default_rng(BASE_SEED + 7700 + seq_idx)
    margin = 0.06 * max(H, W)
    n = max(4, int(round(per_kilopixel * (H + 2 * margin) * (W + 2 * margin) / 1000.0)))
    cx, cy = rng.uniform(-margin, W + margin, n), rng.uniform(-margin, H + margin, n)
    a, b = rng.uniform(sides[0] / 2, sides[1] / 2, n), rng.uniform(sides[0] / 2, sides[1] / 2, n)
    phi = rng.uniform(0.0, np.pi, n)
    grey = rng.uniform(20.0, 235.0, n)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = camera_background(x, y, seq_idx)
    # a pixel grid under an affine pose (every caller's): a rectangle is tested only in a window of rows and columns that contains it -- the same levels, sooner
    inv = None
    if x.ndim == 2 and x.shape[0] > 1 and x.shape[1] > 1:
        R, C = x.shape[0] - 1, x.shape[1] - 1
        o = np.array([x[0, 0], y[0, 0]])
        M = np.array([[(x[0, C] - o[0]) / C, (x[R, 0] - o[0]) / R], [(y[0, C] - o[1]) / C, (y[R, 0] - o[1]) / R]])      # scene = M (col, row) + o
        if abs(np.linalg.det(M)) > 1e-9 and np.allclose(M @ [C, R] + o, [x[R, C], y[R, C]], rtol=0, atol=1e-6):
            inv = np.linalg.inv(M)
    for k in range(n):
        xs, ys, dst = x, y, out
        if inv is not None:
            c, r = inv @ (np.array([cx[k], cy[k]]) - o)
            reach = np.hypot(a[k], b[k]) * np.abs(inv).sum(1) + 2.0
            c0, c1, r0, r1 = int(max(0, c - reach[0])), int(min(x.shape[1], c + reach[0] + 1)), int(max(0, r - reach[1])), int(min(x.shape[0], r + reach[1] + 1))
            if c0 >= c1 or r0 >= r1:
                continue
            xs, ys, dst = x[r0:r1, c0:c1], y[r0:r1, c0:c1], out[r0:r1, c0:c1]
        dx, dy = xs - cx[k], ys - cy[k]
        inside = (np.abs(dx * np.cos(phi[k]) + dy * np.sin(phi[k])) <= a[k]) & (np.abs(dy * np.cos(phi[k]) - dx * np.sin(phi[k])) <= b[k])
        dst[inside] = grey[k]
    return out


def make_corner_frames(n_frames=8, size=1280, seq_idx=0, rot=0.004, shift=1.5, steps=None, **scene):
    """make_camera_frames over corner_scene: -> (frames uint8 (n_frames, H, W, 3) BGR, warps float64 (n_frames, 2, 3)), warps[t] the PLANTED motion from frame
    t - 1 to frame t in full-resolution pixels, warps[0] the identity.  steps: the (theta, tx, ty) of frames 1 .. n_frames - 1, instead of the seeded draw."""
    H, W = (size, size) if np.isscalar(size) else (int(size[0]), int(size[1]))
    rng = np.random.default_rng(BASE_SEED + 7800 + seq_idx)
    pose = np.eye(3)                                                             # frame pixel -> scene
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    frames, warps = [], np.zeros((n_frames, 2, 3))
    for t in range(n_frames):
        if t == 0:
            step = np.eye(3)
        elif steps is not None:
            step = np.vstack([euclidean_warp(*steps[t - 1]), [0.0, 0.0, 1.0]])
        else:
            th = float(np.clip(rng.normal(0.0, rot), -2 * rot, 2 * rot))
            tr = np.clip(rng.normal(0.0, shift, 2), -2 * shift, 2 * shift)
            step = np.vstack([euclidean_warp(th, tr[0], tr[1]), [0.0, 0.0, 1.0]])
        warps[t] = step[:2]
        pose = pose @ np.linalg.inv(step)                                        # pose_t = pose_{t-1} W_t^-1
        sx = pose[0, 0] * xs + pose[0, 1] * ys + pose[0, 2]
        sy = pose[1, 0] * xs + pose[1, 1] * ys + pose[1, 2]
        frames.append(np.clip(np.floor(corner_scene(sx, sy, (H, W), seq_idx, **scene) + 0.5), 0, 255).astype(np.uint8))
    return np.stack(frames), warps


# ---- the Deep Hungarian Net of DeepMOT (/root/reference/tracker/deepmot.py:10-140, class Munkrs) ----
def dhn_tensor_shapes():
    """-> [(name, shape)]: the 38 tensors of Munkrs(element_dim=1, hidden_dim=256, target_size=1, bidirectional=True).state_dict(), in its order
    (4,093,825 values): two 2-layer bidirectional GRUs (input widths 1 and 512, hidden 256; gate rows r, z, n) and three linear layers"""
    out = []
    for gru, first in (("lstm_row", 1), ("lstm_col", 512)):
        for layer in (0, 1):
            for suffix in ("", "_reverse"):
                width = first if layer == 0 else 512
                out += [("%s.weight_ih_l%d%s" % (gru, layer, suffix), (768, width)), ("%s.weight_hh_l%d%s" % (gru, layer, suffix), (768, 256)),
                        ("%s.bias_ih_l%d%s" % (gru, layer, suffix), (768,)), ("%s.bias_hh_l%d%s" % (gru, layer, suffix), (768,))]
    for i, (fin, fout) in enumerate(((512, 256), (256, 64), (64, 1)), 1):
        out += [("hidden2tag_%d.weight" % i, (fout, fin)), ("hidden2tag_%d.bias" % i, (fout,))]
    return out


def make_dhn_weights(seed=0, scale=1.0):
    """seeded weights of the Deep Hungarian Net (no DHN.pth ships with the reference) -> {name: float32 array} in state_dict() order.  One
    numpy.random.RandomState(seed), tensor by tensor: uniform(-scale / sqrt(fan), +scale / sqrt(fan)) with fan = 256 for every GRU tensor, in_features for a
    linear layer's weight and its bias.  scale = 1 (PyTorch's own initialisation range) makes the network nearly constant; scale >= 3 spreads its output."""
    rng = np.random.RandomState(int(seed))
    out = {}
    for name, shape in dhn_tensor_shapes():
        fan = 256 if name.startswith("lstm_") else {"1": 512, "2": 256, "3": 64}[name.split(".")[0][-1]]
        bound = float(scale) / np.sqrt(float(fan))
        out[name] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    return out


# ---- AFLink, the appearance-free link model of StrongSORT++ (the reference's tracker/reid_models/AFLink.py, class PostLinker) ----
def aflink_tensor_shapes():
    """-> [(name, shape)]: the 74 float tensors of PostLinker().state_dict(), in its order, without the num_batches_tracked entries (1,075,266 values): two temporal
    modules of four blocks (a (7,1) convolution and the BatchNorms bnf, bnx, bny of the three columns), two fusion blocks ((1,3) convolution, BatchNorm), a classifier"""
    out = []
    for mod in ("TemporalModule_1", "TemporalModule_2"):
        for k, (cin, cout) in enumerate(((1, 32), (32, 64), (64, 128), (128, 256))):
            out.append(("%s.%d.conv.weight" % (mod, k), (cout, cin, 7, 1)))
            for bn in ("bnf", "bnx", "bny"):
                out += [("%s.%d.%s.%s" % (mod, k, bn, t), (cout,)) for t in ("weight", "bias", "running_mean", "running_var")]
    for mod in ("FusionBlock_1", "FusionBlock_2"):
        out.append((mod + ".conv.weight", (256, 256, 1, 3)))
        out += [("%s.bn.%s" % (mod, t), (256,)) for t in ("weight", "bias", "running_mean", "running_var")]
    out += [("classifier.fc1.weight", (128, 512)), ("classifier.fc1.bias", (128,)), ("classifier.fc2.weight", (2, 128)), ("classifier.fc2.bias", (2,))]
    return out


def aflink_transform(former, latter):
    """the pair transform (DESIGN.md section 4 "AFLink"): former, latter (n, 3) float64 [frame, x, y] -> two (30, 3) float32 blocks"""
    a, b = np.zeros((30, 3)), np.zeros((30, 3))
    fa, lb = np.asarray(former, np.float64)[-30:], np.asarray(latter, np.float64)[:30]
    a[30 - len(fa):] = fa
    b[:len(lb)] = lb
    both = np.concatenate([a, b], 0)
    mn, mx = both.min(0), both.max(0)
    sub, div = (mx + mn) / 2, (mx - mn) / 2 + 1e-5
    return ((a - sub) / div).astype(np.float32), ((b - sub) / div).astype(np.float32)


AFLINK_PAIR_LENGTHS = (1, 2, 29, 30, 31, 60)


def make_aflink_tracklet_pairs(n=256, seed=0):
    """seeded synthetic (former, latter) tracklet pairs, [frame, x, y] float64 rows: lengths among 1, 2, 29, 30, 31, 60, gaps 0..29, the latter either the same
    object moving on or another object nearby; pair 0 is a single-row pair and pair 1 has a constant x column"""
    rng = np.random.RandomState(1000 + int(seed))
    out = []
    for k in range(n):
        la, lb = (1, 1) if k == 0 else (AFLINK_PAIR_LENGTHS[rng.randint(6)], AFLINK_PAIR_LENGTHS[rng.randint(6)])
        gap = int(rng.randint(0, 30))
        f0 = int(rng.randint(1, 500))
        pos, vel = rng.uniform(50, 1200, 2), rng.uniform(-6, 6, 2)
        fa = np.arange(f0, f0 + la, dtype=np.float64)
        fb = np.arange(f0 + la - 1 + gap, f0 + la - 1 + gap + lb, dtype=np.float64)
        pa = pos + (fa - f0)[:, None] * vel + rng.normal(0, 1.0, (la, 2))
        if rng.rand() < 0.5:
            pb = pos + (fb - f0)[:, None] * vel + rng.normal(0, 1.0, (lb, 2))
        else:
            pb = pa[-1] + rng.uniform(-60, 60, 2) + (fb - fb[0])[:, None] * rng.uniform(-6, 6, 2) + rng.normal(0, 1.0, (lb, 2))
        if k == 1:
            pa[:, 0] = 640.0
            pb[:, 0] = 640.0
        out.append((np.column_stack([fa, pa]), np.column_stack([fb, pb])))
    return out


def make_aflink_pairs(n=256, seed=0):
    """-> x1, x2 (n, 30, 3) float32: make_aflink_tracklet_pairs through aflink_transform"""
    blocks = [aflink_transform(a, b) for a, b in make_aflink_tracklet_pairs(n, seed)]
    return np.stack([x[0] for x in blocks]), np.stack([x[1] for x in blocks])


def aflink_forward_np(weights, x1, x2, dtype=np.float64):
    """PostLinker.forward in eval mode from the tensors by name, NumPy: x1, x2 (P, 30, 3) -> the two logits (P, 2)"""
    w = {k: np.asarray(v, dtype) for k, v in weights.items()}

    def bn(x, p):
        return (x - w[p + ".running_mean"]) / np.sqrt(w[p + ".running_var"] + dtype(1e-5)) * w[p + ".weight"] + w[p + ".bias"]

    feats = []
    for b, x in ((1, x1), (2, x2)):
        h = np.asarray(x, dtype)[..., None]                                   # [P][rows][3][channels]
        for k in range(4):
            p = "TemporalModule_%d.%d" % (b, k)
            cw = w[p + ".conv.weight"][:, :, :, 0]                            # [cout][cin][7]
            rows = h.shape[1] - 6
            y = sum(h[:, t:t + rows] @ cw[:, :, t].T for t in range(7))
            y = np.stack([bn(y[:, :, c], "%s.%s" % (p, name)) for c, name in enumerate(("bnf", "bnx", "bny"))], 2)
            h = np.maximum(y, 0)
        fw = w["FusionBlock_%d.conv.weight" % b][:, :, 0, :]                   # [cout][cin][3]
        y = sum(h[:, :, c] @ fw[:, :, c].T for c in range(3))
        feats.append(np.maximum(bn(y, "FusionBlock_%d.bn" % b), 0).mean(1))
    v = np.concatenate(feats, 1)
    hid = np.maximum(v @ w["classifier.fc1.weight"].T + w["classifier.fc1.bias"], 0)
    return hid @ w["classifier.fc2.weight"].T + w["classifier.fc2.bias"]


def make_aflink_weights(seed=0, gain=1.5, accept=0.15):
    """seeded weights of PostLinker (no AFLink_epoch20.pth ships with the reference) -> {name: float32 array} in state_dict() order.  One
    numpy.random.RandomState(seed), tensor by tensor: convolution and linear weights He-normal (std sqrt(2 / fan_in)) times `gain`; BatchNorm weight and running_var
    uniform(0.8, 1.2), bias and running_mean normal(0, 0.1), different for bnf, bnx, bny; fc1.bias zero; fc2.bias = [0, b] with b (rounded to 1e-3) such that about
    `accept` of make_aflink_pairs(256, seed) score above 0.95.  PyTorch's own initialisation makes the score constant (0.48); gain 1.5 spreads it over 0..1."""
    key = (int(seed), float(gain), float(accept))
    if key in _AFLINK_WEIGHTS:      # (the calibration evaluates the network 256 times: once per process and recipe)
        return {k: v.copy() for k, v in _AFLINK_WEIGHTS[key].items()}
    rng = np.random.RandomState(int(seed))
    out = {}
    for name, shape in aflink_tensor_shapes():
        if name.endswith("conv.weight") or name in ("classifier.fc1.weight", "classifier.fc2.weight"):
            fan = int(np.prod(shape[1:]))
            out[name] = (rng.standard_normal(shape) * (float(gain) * np.sqrt(2.0 / fan))).astype(np.float32)
        elif name.startswith("classifier"):
            out[name] = np.zeros(shape, np.float32)
        elif name.endswith((".weight", ".running_var")):
            out[name] = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        else:
            out[name] = rng.normal(0.0, 0.1, shape).astype(np.float32)
    x1, x2 = make_aflink_pairs(256, seed)
    lg = aflink_forward_np(out, x1, x2)
    # score > 0.95  <=>  l1 + b - l0 > log(19)
    b = np.log(19.0) - np.quantile(lg[:, 1] - lg[:, 0], 1.0 - float(accept))
    out["classifier.fc2.bias"] = np.array([0.0, np.round(b, 3)], np.float32)
    _AFLINK_WEIGHTS[key] = {k: v.copy() for k, v in out.items()}
    return out


_AFLINK_WEIGHTS = {}
