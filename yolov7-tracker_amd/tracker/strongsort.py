"""StrongSORT (/root/reference/tracker/strongsort.py:20-250) on the device track pool: the NSA Kalman filter, camera-motion compensation of the
pool before the prediction, one smoothed appearance vector per track and the fused cost gamma * IoU distance + (1 - gamma) * Euclidean appearance
distance for the first and the unconfirmed association.  A frame is three launches of liby7t.so (y7t_tracker_step_strongsort;
csrc/y7t_track_strongsort.h): the appearance distances, the step, the queued vector updates.

The reference's quirks are kept: the second association's unmatched indices, which point into the still-Tracked leftovers of the first, are applied
to strack_pool (strongsort.py:195-198); re_activate keeps the appearance vector; a new track starts with the detection's raw vector.

Seams, as in the reference: `get_feature(tlbrs, ori_img) -> (N, D)` (strongsort.py:66-89: crops resized to width 256, height 128 -> OSNet x0.25) and
the camera motion, shaped like BoTSORT's: `update(dets, img, warp=H)` or `tracker.ECC = object with apply(raw_frame, detections) -> (2, 3)` (or a (6,)
CUDA tensor, which goes to the step without a host copy).  The ECC estimation itself (findTransformECC, botsort.py:78-109) is tracker/gmc.py:
`tracker.ECC = GMC('ecc')`; `ECC` is None by default, as before.  matching_thresh, num_of_budget, use_AFLink and use_GSI are never
read by the reference and do nothing here either."""
import ctypes
import os

import numpy as np
import torch

from .. import _lib
from .botsort import _device_warp
from .basetrack import BaseTracker, STrack, TrackState, _PoolTrack, joint_stracks, sub_stracks, remove_duplicate_stracks  # noqa: F401

REID_SIZE = (256, 128)      # (W, H): cv2.resize(..., dsize=(256, 128)), strongsort.py:56


class _SSPoolTrack(_PoolTrack):
    """View of one slot of a StrongSORT device pool: `features` is the list with the track's one smoothed float32 vector, read from the feature state."""

    @property
    def features(self):
        v = self._pool._vector(self._slot, self.track_id)
        return [] if v is None else [v]

    @features.setter
    def features(self, value):      # (the views are built with an empty list)
        pass

    @property
    def smooth_feat(self):
        f = self.features
        return f[0] if f else None

    @property
    def has_feature(self):
        return bool(self.features)

    @has_feature.setter
    def has_feature(self, value):
        pass


class StrongSORT(BaseTracker):
    """strongsort.py:20-250.  opts: conf_thresh, track_buffer, kalman_format (default / strongsort; tracker/track.py sets strongsort), img_size,
    reid_model_path (+ the optional capacities of BaseTracker)."""
    _KIND = 6  # Y7T_TRACKER_STRONGSORT
    _VIEW = _SSPoolTrack

    def __init__(self, opts, frame_rate=30, gamma=0.1, use_ECC=True, use_AFLink=True, use_GSI=True, num_of_budget=20, reid_model=None, *args, **kwargs):
        if getattr(opts, "kalman_format", "default") not in ("default", "strongsort"):
            raise NotImplementedError("StrongSORT fuses the IoU of xyah means (strongsort.py:150): kalman_format default / strongsort")
        super().__init__(opts, frame_rate=frame_rate)
        self.gamma = float(gamma)
        self.reid_model = reid_model if reid_model is not None else getattr(opts, "reid_model", None)
        path = getattr(opts, "reid_model_path", None)
        if self.reid_model is None and isinstance(path, str) and path.startswith("random"):
            # "random[:osnet]" -- seeded random weights, like DeepSORT's (no checkpoint ships with the reference)
            from .reid import ReIDExtractor
            arch = path.partition(":")[2] or "osnet"
            if arch != "osnet":
                raise ValueError("reid_model_path %r: random or random:osnet (strongsort.py:26: osnet_x0_25)" % (path,))
            self.reid_model = ReIDExtractor(None, arch="osnet", size=REID_SIZE, max_crops=128)
        elif self.reid_model is None and path and os.path.isfile(str(path)):      # strongsort.py:29: load_pretrained_weights(self.reid_model, opts.reid_model_path)
            from .reid import ReIDExtractor
            self.reid_model = ReIDExtractor.from_checkpoint(path, size=REID_SIZE, max_crops=128)
        self.use_ECC = use_ECC
        self.ECC = None                               # optional object with apply(raw_frame, detections) -> (2, 3) matrix
        self.use_AFLink, self.use_GSI, self.num_of_budget = use_AFLink, use_GSI, num_of_budget      # (dead flags of the reference)
        self.matching_thresh = min(0.3, getattr(self.opts, "iou_thresh", 0.5) - 0.2)
        self._warp = torch.zeros(6, dtype=torch.float64, device="cuda")
        self._feat = None           # feature state, allocated when the feature dimension is known
        self._feat_dim = 0
        self._feat_used = False     # a frame with appearance vectors has been stepped (from then on the width is fixed)
        self._vec_cache = None

    _warned = False

    def get_feature(self, tlbrs, ori_img):
        """strongsort.py:66-89: crops of the boxes -> self.reid_model(crops) -> (N, D) raw (unnormalised) features"""
        if self.reid_model is None:
            raise _lib.Y7TError("StrongSORT needs appearance features: pass reid_model=<callable(list of crops) -> (N, D)> (e.g. "
                                "yolov7_tracker_amd.tracker.reid.ReIDExtractor(size=(256, 128))) or override get_feature")
        if hasattr(self.reid_model, "features_for_boxes"):      # device extractor: crop + resize + normalise on the GPU
            return self.reid_model.features_for_boxes(ori_img, tlbrs)
        if isinstance(ori_img, torch.Tensor):
            ori_img = ori_img.cpu().numpy()
        crops = []
        for tlbr in tlbrs:
            x1, y1, x2, y2 = (int(v) for v in tlbr)
            crops.append(ori_img[y1:y2, x1:x2])
        return self.reid_model(crops) if crops else np.zeros((0, max(self._feat_dim, 1)), np.float32)

    def _ensure_feature_state(self, dim):
        """the per-slot vectors + the frame's appearance matrix, sized for `dim`-wide embeddings; a state sized on a guess before any detection
        passed det_thresh (no track exists yet) is re-made when the real width shows up, as DeepSORT's"""
        if self._feat is None or (int(dim) != self._feat_dim and not self._feat_used):
            self._feat_dim = int(dim)
            nb = int(self._L.y7t_strongsort_feature_bytes(self.cap_t, self.cap_d, self._feat_dim))
            self._feat = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            _lib.check(self._L.y7t_strongsort_init(_lib.ptr(self._feat), nb, self.cap_t, self.cap_d, self._feat_dim, self.gamma, _lib.stream_ptr()))
        elif int(dim) != self._feat_dim:
            raise ValueError("feature dimension changed from %d to %d" % (self._feat_dim, int(dim)))

    def _check_feats(self, feats_dev, n):
        """what the device step dereferences: n rows of `_feat_dim` contiguous float32 on the GPU"""
        if not isinstance(feats_dev, torch.Tensor) or feats_dev.dim() != 2:
            raise _lib.Y7TError("StrongSORT: features must be an (n, D) tensor")
        if feats_dev.shape[0] < n:
            raise _lib.Y7TError("StrongSORT: %d feature rows for %d detections" % (feats_dev.shape[0], n))
        return feats_dev.to(device="cuda", dtype=torch.float32).contiguous()

    def _step(self, d, n, feats, warp, out):
        if out is None:
            optr, cptr = _lib.ptr(self._out), self._count_ptr
        else:
            optr, cptr = _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + self.cap_t * 8 * 8)
        self._det_keep = (d, feats, warp)
        _lib.check(self._L.y7t_tracker_step_strongsort(_lib.ptr(self._state), _lib.ptr(self._feat), _lib.ptr(d), n, _lib.ptr(feats), optr, self.cap_t, cptr,
                                                       self.threads, _lib.ptr(warp), _lib.stream_ptr()))
        self.frame_id += 1
        self._snap_cache = None
        self._vec_cache = None

    def _launch(self, det_dev, feats_dev=None, warp=None, out=None, **kw):
        """enqueue one frame without a host round trip (pipelines): det_dev (n, 6) float32 and feats_dev (n, D) float32 DEVICE tensors (rows at or
        below det_thresh are ignored by the step), warp a (6,) float64 device tensor or None, out like BaseTracker._launch.  det_dev None: the
        predict-only step of update_without_detection (basetrack.py:489-537), the same for every tracker."""
        if det_dev is None:
            self._vec_cache = None
            return super()._launch(None, out=out, **kw)
        if feats_dev is None:
            raise _lib.Y7TError("StrongSORT._launch needs the detections' appearance features (use update() for the get_feature seam)")
        d = det_dev.reshape(-1, 6)
        n = d.shape[0]
        if n > self.cap_d:
            raise _lib.Y7TError("%d detections exceed the pool capacity max_dets=%d" % (n, self.cap_d))
        d = d.to(device="cuda", dtype=torch.float32).contiguous()
        feats_dev = self._check_feats(feats_dev, n)
        self._ensure_feature_state(feats_dev.shape[1])
        self._feat_used = self._feat_used or n > 0
        self._step(d, n, feats_dev, warp, out)

    def update(self, det_results, ori_img=None, warp=None):
        """(N,6) [x1,y1,x2,y2,conf,cls] + the frame -> list of tracks (strongsort.py:91-250)"""
        if isinstance(det_results, torch.Tensor):
            det_host = det_results.detach().cpu().numpy()
        else:
            det_host = np.asarray(det_results)
        det_host = np.ascontiguousarray(det_host, dtype=np.float32).reshape(-1, 6)
        n = det_host.shape[0]
        if n > self.cap_d:
            raise _lib.Y7TError("%d detections exceed the pool capacity max_dets=%d" % (n, self.cap_d))
        keep = det_host[:, 4] > np.float32(self.det_thresh)            # strongsort.py:110: only these get features
        feats = None
        if keep.any():
            feats = self.get_feature(det_host[keep, :4], ori_img)
            if not isinstance(feats, torch.Tensor):
                feats = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32))
            feats = self._check_feats(feats, int(keep.sum()))
            self._ensure_feature_state(feats.shape[1])
            self._feat_used = True
        elif self._feat is None:        # nothing above det_thresh yet: the extractor's width if it states one, else a placeholder that the first real frame replaces
            self._ensure_feature_state(getattr(self.reid_model, "feat_dim", None) or self._feat_dim or 128)
        if warp is None and self.use_ECC and self.ECC is not None:
            warp = self.ECC.apply(ori_img, det_results)
        if warp is None and self.use_ECC and not StrongSORT._warned:
            import warnings
            warnings.warn("StrongSORT: use_ECC is set but no camera-motion matrix was supplied (update(..., warp=H) or tracker.ECC = object with "
                          "apply(raw_frame, detections), e.g. tracker/gmc.py's GMC('ecc')): the reference estimates one per frame with OpenCV (botsort.py:13-248); "
                          "running WITHOUT compensation, results on moving-camera footage will differ from the reference", RuntimeWarning)
            StrongSORT._warned = True
        w = None
        if warp is not None and self.use_ECC:
            w = _device_warp(warp, self._warp)
        d = torch.from_numpy(det_host).cuda()
        allf = torch.zeros((max(n, 1), self._feat_dim), dtype=torch.float32, device="cuda")
        if feats is not None:
            allf[torch.from_numpy(np.nonzero(keep)[0]).cuda()] = feats
        self._step(d, n, allf, w, None)
        rows = self._collect()
        st = self._feature_status()
        if st:
            raise _lib.Y7TError("StrongSORT feature state overflow (status %d): the feature state is smaller than the pool" % st)
        return rows

    def update_without_detection(self, det_results=None, ori_img=None):
        self._vec_cache = None
        return super().update_without_detection(det_results, ori_img)

    def _feature_status(self):
        return int(self._feat[20:24].view(torch.int32).item())           # Y7TSsHdr.status

    # -- host views of the feature state ---------------------------------------------------------
    def _vectors(self):
        """(cap_t, D) float32 host copy of the slots' vectors (cached until the next step)"""
        if self._vec_cache is None and self._feat is not None:
            off = 64                                                     # the vectors follow the 64-byte header (y7t_ss_layout)
            raw = self._feat[off:off + 4 * self.cap_t * self._feat_dim].cpu().numpy()
            self._vec_cache = raw.view(np.float32).reshape(self.cap_t, self._feat_dim)
        return self._vec_cache

    def _vector(self, slot, track_id):
        if self._feat is None or not self._feat_used or self._snapshot()["tid"][slot] != track_id:
            return None
        return self._vectors()[slot].copy()

    def _views(self, list_name, n_name):
        return [_SSPoolTrack(t._pool, t._slot, t.track_id, t._tlwh_now, t.cls, t.score) for t in super()._views(list_name, n_name)]
