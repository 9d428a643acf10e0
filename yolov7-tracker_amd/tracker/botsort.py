"""BoT-SORT state path (/root/reference/tracker/botsort.py:250-493) on the device pool: xywh Kalman filter
(BoTSORTKalmanFilter, kalman_filter.py:414-605), camera-motion compensation of the predicted tracks (multi_gmc,
botsort.py:250-269) and BoT-SORT's association variant -- including its two quirks (every unmatched pool track, not only the
Tracked ones, goes to the low-score association, botsort.py:411; new tracks are spawned from the detections left after the
FIRST association, botsort.py:462-466).

The appearance branch (`use_apperance_model`, equations 12-13 of the BoT-SORT paper: the first and the unconfirmed association solve min(IoU distance, App) with
App = 0.5 * cosine distance of the track's smoothed vector and the detection's, set to 1 where the IoU distance exceeds theta_iou = 0.5 or App exceeds theta_emb
= 0.25) is off by default, as in the reference; `BoTSORT(opts, use_apperance_model=True, reid_model=None)` returns a BoTSORTReID, which runs it on the device
(y7t_tracker_step_botsort_reid; csrc/y7t_track_botsort_reid.h): cosines are taken only for the pairs at or under theta_iou, which the step finds in its own pair
pass.  Features enter at `get_feature(tlbrs, ori_img) -> (N, D)` (botsort.py:291-311: the DeepSORT Net on 128 x 64 crops; tracker/appearance.py) for the
detections with score >= conf_thresh.

The camera-motion ESTIMATION (`GMC`, botsort.py:13-248) is tracker/gmc.py for method 'ecc' (findTransformECC as HIP kernels) and for method 'features' (applyFeaures, botsort.py:111-235,
under a specification of our own); OpenCV's own ORB / SIFT and the GMC files stay out of scope.  The 2x3 warp of a frame is an input: `update(dets, img, warp=H)` or `tracker.gmc = callable(raw_frame, detections) -> H`, e.g. `GMC('ecc').apply_device`, whose (6,) float64
DEVICE tensor goes to the step without a host copy.  `tracker.gmc` is None by default, as before."""
import numpy as np
import torch

from .. import _lib
from .appearance import AppearanceTracker, OneVectorViews, osnet_family_archs
from .basetrack import BaseTracker, STrack, TrackState, joint_stracks, sub_stracks  # noqa: F401


def _device_warp(warp, buf):
    """the frame's 2x3 matrix as a (6,) float64 device tensor: an estimator's CUDA tensor as it is (no host copy), anything else through `buf`"""
    if isinstance(warp, torch.Tensor) and warp.is_cuda:
        return warp.to(torch.float64).reshape(6).contiguous()
    if isinstance(warp, torch.Tensor):
        warp = warp.detach().numpy()
    buf.copy_(torch.as_tensor(np.ascontiguousarray(warp, dtype=np.float64).reshape(6)), non_blocking=True)
    return buf


class BoTSORT(BaseTracker):
    _KIND = 2  # Y7T_TRACKER_BOTSORT

    def __new__(cls, opts=None, *args, use_apperance_model=False, **kwargs):
        if use_apperance_model and cls is BoTSORT:      # the appearance branch is a tracker kind of its own: its class, constructed here (no __init__ of this class runs)
            return BoTSORTReID(opts, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, opts, frame_rate=30, gamma=0.02, use_GMC=True, *args, **kwargs):
        if getattr(opts, "kalman_format", "botsort") != "botsort":
            opts.kalman_format = "botsort"          # tracker/track.py:68-69 forces it for this tracker
        super().__init__(opts, frame_rate=frame_rate)
        self.use_apperance_model = False
        self.gamma = gamma
        self.low_conf_thresh = max(0.15, self.opts.conf_thresh - 0.3)
        self.filter_small_area = False
        self.use_GMC = use_GMC
        self.gmc = None                              # optional callable(raw_frame, detections) -> (2, 3) matrix
        self.theta_iou, self.theta_emb = 0.5, 0.25
        self._warp = torch.zeros(6, dtype=torch.float64, device="cuda")

    _warned = False

    def update(self, det_results, ori_img=None, warp=None):
        if warp is None and self.use_GMC and self.gmc is not None:
            warp = self.gmc(ori_img, det_results)
        if warp is None and self.use_GMC and not BoTSORT._warned:
            import warnings
            warnings.warn("BoTSORT: use_GMC is set but no camera-motion matrix was supplied (update(..., warp=H) or tracker.gmc = callable): "
                          "the reference estimates one per frame with OpenCV (botsort.py:13-248; tracker.gmc = GMC('ecc').apply_device does it here); running WITHOUT "
                          "compensation, results on moving-camera footage will differ from the reference", RuntimeWarning)
            BoTSORT._warned = True
        w = None
        if warp is not None and self.use_GMC:
            w = self._warp_keep = _device_warp(warp, self._warp)      # (alive until the step has run)
        self._launch(det_results, warp=w)
        return self._collect()


class BoTSORTReID(OneVectorViews, AppearanceTracker):
    """botsort.py:272-493 with use_apperance_model = True.  opts: conf_thresh, track_buffer, img_size, reid_model_path (+ the optional capacities of BaseTracker);
    kalman_format is botsort (track.py:68-69).  Camera motion as for BoTSORT: `update(dets, img, warp=H)` or `tracker.gmc = callable(raw_frame, detections) -> H`."""
    _KIND = 8  # Y7T_TRACKER_BOTSORT_REID
    _KALMAN_FORMATS = ("botsort",)
    _KALMAN_NOTE = "runs the xywh filter (track.py:68-69)"
    _FEATURE_AT_THRESHOLD = True      # botsort.py:339: det_results[:, 4] >= self.det_thresh
    _REID_ARCHS = dict({"deepsort": dict(max_crops=128), "osnet": dict(max_crops=512)}, **osnet_family_archs(max_crops=128))      # botsort.py:3,278: Extractor = the DeepSORT Net on 128 x 64 crops
    _REID_ARCH_NOTE = "random, random:deepsort, random:osnet or random:osnet_x0_25 / _x0_5 / _x0_75 / _x1_0 / osnet_ibn_x1_0 (the general fp16 path)"
    _REID_HINT = "ReIDExtractor(arch='deepsort')"
    _OVERFLOW_NOTE = (": bit 2 = the feature state is smaller than the pool, 4 = an appearance vector with zero or non-finite norm (the reference hands NaN costs "
                      "to lapjv; the frame was not stepped), 16 = more queued vectors than the list holds, 32 = more pairs at or under theta_iou than the pair table holds")

    def __init__(self, opts, frame_rate=30, gamma=0.02, use_GMC=True, reid_model=None, *args, **kwargs):
        if getattr(opts, "kalman_format", "botsort") != "botsort":
            opts.kalman_format = "botsort"          # tracker/track.py:68-69 forces it for this tracker
        super().__init__(opts, frame_rate=frame_rate, reid_model=reid_model)
        self.use_apperance_model = True
        self.gamma = gamma
        self.low_conf_thresh = max(0.15, self.opts.conf_thresh - 0.3)
        self.filter_small_area = False
        self.use_GMC = use_GMC
        self.gmc = None                              # optional callable(raw_frame, detections) -> (2, 3) matrix
        self.theta_iou, self.theta_emb = 0.5, 0.25
        self._warp = torch.zeros(6, dtype=torch.float64, device="cuda")
        self._vec_cache = None

    def _feature_bytes(self, dim):
        return self._L.y7t_botsort_reid_feature_bytes(self.cap_t, self.cap_d, dim)

    def _feature_init(self, nbytes):      # one smoothed vector per slot, the frame's normalised rows, the pair table
        return self._L.y7t_botsort_reid_init(_lib.ptr(self._feat), nbytes, self.cap_t, self.cap_d, self._feat_dim, self.theta_iou, self.theta_emb, _lib.stream_ptr())

    def _step(self, d, n, feats, warp, out):
        optr, cptr = self._out_ptrs(out)
        self._det_keep = (d, feats, warp)
        _lib.check(self._L.y7t_tracker_step_botsort_reid(_lib.ptr(self._state), _lib.ptr(self._feat), _lib.ptr(d), n, _lib.ptr(feats), optr, self.cap_t, cptr,
                                                         self.threads, _lib.ptr(warp), _lib.stream_ptr()))
        self.frame_id += 1
        self._snap_cache = None
        self._vec_cache = None

    def _launch(self, det_dev, feats_dev=None, warp=None, out=None, **kw):
        if det_dev is None:      # (the predict-only step applies no camera motion)
            self._vec_cache, warp = None, None
        return super()._launch(det_dev, feats_dev, warp=warp, out=out, **kw)

    def _frame_warp(self, warp, ori_img, det_results):
        if warp is None and self.use_GMC and self.gmc is not None:
            warp = self.gmc(ori_img, det_results)
        return _device_warp(warp, self._warp) if warp is not None and self.use_GMC else None

    def cosine_count(self):
        """how many cosines the last frame's step evaluated (the pairs at or under theta_iou of its two fused associations) and how many of them theta_emb sent to 1"""
        h = self._feat[:64].view(torch.int32).cpu()
        return int(h[7]), int(h[12])
