"""Association ops with the reference's signatures (/root/reference/tracker/matching.py:30-82),
computed on the MI355X by liby7t.so: `iou_distance` (IoU with the +1 pixel convention of
cython_bbox.bbox_overlaps) and `linear_assignment` (lap.lapjv(extend_cost=True, cost_limit=t)); UAVMOT's structure cost
(matching.py:284-388) with `structure_similarity_distance` on the device; `embedding_distance` (matching.py:84-103) on the track views' vectors; DeepMOT's `ecu_iou_distance` (matching.py:129-162)."""
import math

import numpy as np
import torch

from .. import _lib


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def ious(atlbrs, btlbrs):
    """matching.py:44-61 -> (N, M) float64 IoU."""
    return 1.0 - _cost(atlbrs, btlbrs) if (len(atlbrs) and len(btlbrs)) else np.zeros((len(atlbrs), len(btlbrs)))


def _cost(atlbrs, btlbrs):
    _lib.require_gpu()
    a = _dev(np.asarray(atlbrs, dtype=np.float64).reshape(-1, 4), np.float64)
    b = _dev(np.asarray(btlbrs, dtype=np.float64).reshape(-1, 4), np.float64)
    n, m = a.shape[0], b.shape[0]
    out = torch.empty((n, m), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().y7t_iou_cost_f64(_lib.ptr(a), n, _lib.ptr(b), m, _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu().numpy()


def iou_distance(atracks, btracks):
    """matching.py:64-82: lists of tracks (objects with .tlbr) or of tlbr arrays -> (N, M) float64 cost."""
    if (len(atracks) > 0 and isinstance(atracks[0], np.ndarray)) or (len(btracks) > 0 and isinstance(btracks[0], np.ndarray)):
        atlbrs, btlbrs = atracks, btracks
    else:
        atlbrs = [t.tlbr for t in atracks]
        btlbrs = [t.tlbr for t in btracks]
    if len(atlbrs) == 0 or len(btlbrs) == 0:
        return np.zeros((len(atlbrs), len(btlbrs)), dtype=np.float64)
    return _cost(atlbrs, btlbrs)


def ecu_iou_distance(tracks, detections, img0_shape):
    """matching.py:129-162 (DeepMOT): 0.5 * ((1 - exp(-5 * centre distance / image diagonal)) + iou_distance) -> (N, M) float64.  The centres are taken in the
    boxes' own dtypes (a detection's tlwh is float32, a predicted track's float64), their differences in float64, as numpy evaluates the reference's lines.
    Host arithmetic beside the device IoU, for code written against the reference's matching module; the fused device step computes the same per pair
    (csrc/y7t_track_deepmot.h: y7t_dm_ecu_iou)."""
    cost_matrix = np.zeros((len(tracks), len(detections)), dtype=np.float64)
    if cost_matrix.size == 0:
        return cost_matrix
    det_bbox = np.asarray([det.tlwh for det in detections])
    trk_bbox = np.asarray([trk.tlwh for trk in tracks])
    det_cx, det_cy = det_bbox[:, 0] + 0.5 * det_bbox[:, 2], det_bbox[:, 1] + 0.5 * det_bbox[:, 3]
    trk_cx, trk_cy = trk_bbox[:, 0] + 0.5 * trk_bbox[:, 2], trk_bbox[:, 1] + 0.5 * trk_bbox[:, 3]
    ecu_dist = np.asarray([np.sqrt((det_cx - trk_cx[i]) ** 2 + (det_cy - trk_cy[i]) ** 2) for i in range(len(tracks))])
    norm_factor = float((img0_shape[0] ** 2 + img0_shape[1] ** 2) ** 0.5)
    ecu_dist = 1. - np.exp(-5 * ecu_dist / norm_factor)
    return 0.5 * (ecu_dist + iou_distance(tracks, detections))


def cal_cosine_distance(mat1, mat2):
    """matching.py:165-178: the rows divided by their norms, then mat1 . mat2^T (in the arrays' own dtype)"""
    mat1 = mat1 / np.linalg.norm(mat1, axis=1, keepdims=True)
    mat2 = mat2 / np.linalg.norm(mat2, axis=1, keepdims=True)
    return np.dot(mat1, mat2.T)


def embedding_distance(tracks, detections, metric='cosine'):
    """matching.py:84-103: the appearance distance of features[-1] of both sides, cast to float64 -> (N, M) float64.  'euclidean' (StrongSORT):
    np.maximum(0.0, cdist) -- per pair one sequential float64 chain d = u[k] - v[k]; s += d * d over k, then sqrt, which is what scipy's cdist computes
    and what the device step's k_ss_appearance restates; 'cosine': 1 - cal_cosine_distance.  Host arithmetic on the (host-side) vectors of the track
    views, for code written against the reference's matching module; the fused device step does not go through it."""
    cost_matrix = np.zeros((len(tracks), len(detections)), dtype=np.float64)
    if cost_matrix.size == 0:
        return cost_matrix
    det_features = np.asarray([track.features[-1] for track in detections], dtype=np.float64)
    track_features = np.asarray([track.features[-1] for track in tracks], dtype=np.float64)
    if metric == 'euclidean':
        s = np.zeros_like(cost_matrix)
        for k in range(track_features.shape[1]):      # (scipy's chain, a k at a time for every pair: numpy fuses nothing)
            d = track_features[:, k, None] - det_features[None, :, k]
            s += d * d
        cost_matrix = np.maximum(0.0, np.sqrt(s))
    elif metric == 'cosine':
        cost_matrix = 1. - cal_cosine_distance(track_features, det_features)
    else:
        raise NotImplementedError
    return cost_matrix


def buffered_iou_distance(atracks, btracks, level=1):
    """matching.py:391-407 (C-BIoU): the tracks' motion states against the detections' buffered boxes, both as tlbr in their own dtype
    (tlwh2tlbr of the C_BIoUSTrack objects), -> (N, M) float64 cost 1 - IoU.  level 1: motion_state1 / buffer_bbox1, level 2: motion_state2 / buffer_bbox2."""
    assert level in [1, 2], 'level must be 1 or 2'
    if level == 1:
        atlbrs = [track.tlwh2tlbr(track.motion_state1) for track in atracks]
        btlbrs = [det.tlwh2tlbr(det.buffer_bbox1) for det in btracks]
    else:
        atlbrs = [track.tlwh2tlbr(track.motion_state2) for track in atracks]
        btlbrs = [det.tlwh2tlbr(det.buffer_bbox2) for det in btracks]
    if len(atlbrs) == 0 or len(btlbrs) == 0:
        return np.ones((len(atlbrs), len(btlbrs)), dtype=np.float64)
    return _cost(atlbrs, btlbrs)


def lapjv_device(cost, cost_limit):
    """-> (opt, x, y) like lap.lapjv(cost, extend_cost=True, cost_limit=cost_limit)."""
    _lib.require_gpu()
    L = _lib.load()
    c = _dev(cost, np.float64)
    n, m = c.shape
    x = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    y = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
    opt = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(int(L.y7t_lapjv_workspace_bytes(n, m)), 8), dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_lapjv_f64(_lib.ptr(c), n, m, float(cost_limit), _lib.ptr(x), _lib.ptr(y), _lib.ptr(opt), _lib.ptr(ws),
                               _lib.stream_ptr()))
    return float(opt.item()), x[:n].cpu().numpy().astype(np.int64), y[:m].cpu().numpy().astype(np.int64)


def lapjv_host(cost, cost_limit):
    """the same for a numpy cost matrix through the library's host-pointer entry (y7t_lapjv_f64_host: staging buffers owned by the library, one call,
    one synchronisation) -- what matching.linear_assignment uses, since the reference calls it with numpy arrays"""
    _lib.require_gpu()
    L = _lib.load()
    c = np.ascontiguousarray(cost, dtype=np.float64)
    n, m = c.shape
    x, y, opt = np.empty(max(n, 1), np.int32), np.empty(max(m, 1), np.int32), np.zeros(1, np.float64)
    _lib.check(L.y7t_lapjv_f64_host(c.ctypes.data, n, m, float(cost_limit), x.ctypes.data, y.ctypes.data, opt.ctypes.data, _lib.stream_ptr()))
    return float(opt[0]), x[:n].astype(np.int64), y[:m].astype(np.int64)


def linear_assignment(cost_matrix, thresh):
    """matching.py:30-41 -> (matches (K,2) int, unmatched_a, unmatched_b)."""
    on_device = torch.is_tensor(cost_matrix) and cost_matrix.device.type == "cuda"      # (the reference only ever passes numpy; a device cost stays there)
    if not on_device:
        cost_matrix = np.asarray(cost_matrix.cpu() if torch.is_tensor(cost_matrix) else cost_matrix)
    if (cost_matrix.numel() if on_device else cost_matrix.size) == 0:
        return np.empty((0, 2), dtype=int), tuple(range(cost_matrix.shape[0])), tuple(range(cost_matrix.shape[1]))
    if on_device:
        _, x, y = lapjv_device(cost_matrix, thresh)
    else:
        _, x, y = lapjv_host(cost_matrix, thresh)
    matches = np.asarray([[ix, mx] for ix, mx in enumerate(x) if mx >= 0])
    return matches, np.where(x < 0)[0], np.where(y < 0)[0]


# ---- UAVMOT's structure cost (matching.py:284-388) ----
def local_relation_fuse_motion(cost_matrix, tracks, detections, only_position=False, lambda_=0.98):
    """matching.py:284-311: lambda_ * cost + (1 - lambda_) * structure_similarity_distance(tracks, detections)"""
    if cost_matrix.size == 0:
        return cost_matrix
    structure_distance = structure_similarity_distance(tracks, detections)
    return lambda_ * cost_matrix + (1 - lambda_) * structure_distance


def structure_similarity_distance(tracks, detections):
    """matching.py:312-319 -> (N, M) float64 max(0, cosine distance) of the structure vectors of the tracks (mean[0:2]) and of the detections
    (get_xy()), computed on the device (y7t_structure_distance_f64).  The detections' centres must be float32 (AMF_STrack detections: get_xy() of
    a float32 tlwh) and the tracks' float64 (means after multi_predict), the dtypes of the reference's one call site (uavmot.py:189)."""
    txy, dxy = _track_xy(tracks), _det_xy(detections)
    if txy.dtype != np.float64 or dxy.dtype != np.float32:
        raise ValueError("structure_similarity_distance: float64 track means and float32 detection centres (got %s / %s)" % (txy.dtype, dxy.dtype))
    n, m = txy.shape[0], dxy.shape[0]
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.float64)
    _lib.require_gpu()
    a, b = _dev(txy, np.float64), _dev(dxy, np.float64)
    out = torch.empty((n, m), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().y7t_structure_distance_f64(_lib.ptr(a), n, _lib.ptr(b), m, _lib.ptr(out), _lib.stream_ptr()))
    return out.cpu().numpy()


def angle(v1, v2):
    """matching.py:321-342: the included angle of two offsets, from their atan2 angles truncated to whole degrees"""
    angle1 = int(math.atan2(v1[1], v1[0]) * 180 / math.pi)
    angle2 = int(math.atan2(v2[1], v2[0]) * 180 / math.pi)
    if angle1 * angle2 >= 0:
        return abs(angle1 - angle2)
    included_angle = abs(angle1) + abs(angle2)
    if included_angle > 180:
        included_angle = 360 - included_angle
    return included_angle


def structure_representation(tracks, mode='trcak'):
    """matching.py:344-388 -> (N, 3) float64 [max, min, included angle] of every element's neighbours at 0 < distance < 400 (tracks: mean[0:2];
    mode == "detection": get_xy())"""
    xy = _det_xy(tracks) if mode == "detection" else _track_xy(tracks)
    return _structure_vectors(xy)


def _track_xy(tracks):
    return np.asarray([t.mean[0:2] for t in tracks]).reshape(-1, 2)


def _det_xy(detections):
    return np.asarray([d.get_xy() for d in detections]).reshape(-1, 2)


def _structure_vectors(xy, dtype=None):
    """structure_representation of a (N, 2) array of centres, in the reference's arithmetic (its dtype; np.linalg.norm for the distances)"""
    xy = np.asarray(xy, dtype=dtype)
    rows = []
    for a in range(xy.shape[0]):
        length, index = [], []
        for b in range(xy.shape[0]):
            pp = [np.linalg.norm(np.array(xy[a, 0] - xy[b, 0])), np.linalg.norm(np.array(xy[a, 1] - xy[b, 1]))]
            lgt = np.linalg.norm(pp)
            if 0 < lgt < 400:
                length.append(lgt)
                index.append(b)
        if not length:
            rows.append([0.0001, 0.0001, 0.0001])
            continue
        mx, mn = max(length), min(length)
        if mx == mn:
            rows.append([mx, mn, 0.0001])
            continue
        v1 = xy[index[length.index(mx)]] - xy[a]
        v2 = xy[index[length.index(mn)]] - xy[a]
        rows.append([mx, mn, angle(v1, v2)])
    return np.asarray(rows)


def _structure_cosine(track_vec, det_vec):
    """np.maximum(0, cdist(T, D, "cosine")) restated elementwise (unfused left-to-right sums, the cosine clipped to [-1, 1]) -- what the device computes"""
    u, v = np.asarray(track_vec, np.float64)[:, None, :], np.asarray(det_vec, np.float64)[None, :, :]
    dot = u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]
    uu = u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1] + u[..., 2] * u[..., 2]
    vv = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    return np.maximum(0.0, 1.0 - np.clip(dot / (np.sqrt(uu) * np.sqrt(vv)), -1.0, 1.0))
