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
import numpy as np
import torch

from .. import _lib
from .appearance import AppearanceTracker, OneVectorViews, osnet_family_archs, _VectorPoolTrack as _SSPoolTrack  # noqa: F401
from .botsort import _device_warp
from .basetrack import STrack, TrackState, _PoolTrack, joint_stracks, sub_stracks, remove_duplicate_stracks  # noqa: F401

REID_SIZE = (256, 128)      # (W, H): cv2.resize(..., dsize=(256, 128)), strongsort.py:56


class StrongSORT(OneVectorViews, AppearanceTracker):
    """strongsort.py:20-250.  opts: conf_thresh, track_buffer, kalman_format (default / strongsort; tracker/track.py sets strongsort), img_size,
    reid_model_path (+ the optional capacities of BaseTracker)."""
    _KIND = 6  # Y7T_TRACKER_STRONGSORT
    _KALMAN_NOTE = "fuses the IoU of xyah means (strongsort.py:150)"
    _REID_ARCHS = dict({"osnet": dict(size=REID_SIZE, max_crops=128)}, **osnet_family_archs(size=REID_SIZE, max_crops=128))
    _REID_ARCH_NOTE = "random or random:osnet (strongsort.py:26: osnet_x0_25), or random:osnet_x0_25 / _x0_5 / _x0_75 / _x1_0 / osnet_ibn_x1_0 (the general fp16 path)"
    _REID_CKPT = dict(size=REID_SIZE, max_crops=128)
    _REID_HINT = "ReIDExtractor(size=(256, 128))"
    _OVERFLOW_NOTE = ": the feature state is smaller than the pool"

    def __init__(self, opts, frame_rate=30, gamma=0.1, use_ECC=True, use_AFLink=True, use_GSI=True, num_of_budget=20, reid_model=None, *args, **kwargs):
        super().__init__(opts, frame_rate=frame_rate, reid_model=reid_model)
        self.gamma = float(gamma)
        self.use_ECC = use_ECC
        self.ECC = None                               # optional object with apply(raw_frame, detections) -> (2, 3) matrix
        self.use_AFLink, self.use_GSI, self.num_of_budget = use_AFLink, use_GSI, num_of_budget      # (dead flags of the reference)
        self.matching_thresh = min(0.3, getattr(self.opts, "iou_thresh", 0.5) - 0.2)
        self._warp = torch.zeros(6, dtype=torch.float64, device="cuda")
        self._vec_cache = None

    _warned = False

    def _feature_bytes(self, dim):
        return self._L.y7t_strongsort_feature_bytes(self.cap_t, self.cap_d, dim)

    def _feature_init(self, nbytes):      # one smoothed vector per slot + the frame's appearance matrix
        return self._L.y7t_strongsort_init(_lib.ptr(self._feat), nbytes, self.cap_t, self.cap_d, self._feat_dim, self.gamma, _lib.stream_ptr())

    def _step(self, d, n, feats, warp, out):
        optr, cptr = self._out_ptrs(out)
        self._det_keep = (d, feats, warp)
        _lib.check(self._L.y7t_tracker_step_strongsort(_lib.ptr(self._state), _lib.ptr(self._feat), _lib.ptr(d), n, _lib.ptr(feats), optr, self.cap_t, cptr,
                                                       self.threads, _lib.ptr(warp), _lib.stream_ptr()))
        self.frame_id += 1
        self._snap_cache = None
        self._vec_cache = None

    def _launch(self, det_dev, feats_dev=None, warp=None, out=None, **kw):
        if det_dev is None:      # (the predict-only step applies no camera motion)
            self._vec_cache, warp = None, None
        return super()._launch(det_dev, feats_dev, warp=warp, out=out, **kw)

    def _frame_warp(self, warp, ori_img, det_results):
        if warp is None and self.use_ECC and self.ECC is not None:
            warp = self.ECC.apply(ori_img, det_results)
        if warp is None and self.use_ECC and not StrongSORT._warned:
            import warnings
            warnings.warn("StrongSORT: use_ECC is set but no camera-motion matrix was supplied (update(..., warp=H) or tracker.ECC = object with "
                          "apply(raw_frame, detections), e.g. tracker/gmc.py's GMC('ecc')): the reference estimates one per frame with OpenCV (botsort.py:13-248); "
                          "running WITHOUT compensation, results on moving-camera footage will differ from the reference", RuntimeWarning)
            StrongSORT._warned = True
        return _device_warp(warp, self._warp) if warp is not None and self.use_ECC else None
