"""DeepSORT (/root/reference/tracker/deepsort.py:10-227) on the device track pool: the matching cascade over the gated appearance
cost (nearest cosine distance to a track's last 100 appearance vectors, Mahalanobis gate on the predicted Kalman state), the IoU
fallbacks and the list bookkeeping run in liby7t.so (y7t_tracker_step_deepsort; csrc/y7t_track_deepsort.h).

Appearance features enter at the reference's own seam, `get_feature(tlbrs, ori_img) -> (N, D)` (deepsort.py:19-41; tracker/appearance.py).
The reference hard-wires `Extractor(opts.reid_model_path)` with weights/ckpt.t7, which does not ship with it."""
from .. import _lib
from .appearance import AppearanceTracker, osnet_family_archs

STORE_FEATURES_BUDGET = 100     # STrack.__init__ store_features_budget (basetrack.py:76)


class DeepSORT(AppearanceTracker):
    _KIND = 3  # Y7T_TRACKER_DEEPSORT
    _KALMAN_NOTE = "gates on xyah measurements (deepsort.py:59)"
    _REID_ARCHS = dict({"osnet": dict(max_crops=512), "deepsort": dict(max_crops=128)}, **osnet_family_archs(max_crops=128))
    _REID_ARCH_NOTE = "random, random:osnet, random:deepsort or random:osnet_x0_25 / _x0_5 / _x0_75 / _x1_0 / osnet_ibn_x1_0 (the general fp16 path)"
    _REID_HINT = "ReIDExtractor"

    def __init__(self, opts, frame_rate=30, gamma=0.02, reid_model=None, *args, **kwargs):
        super().__init__(opts, frame_rate=frame_rate, reid_model=reid_model)
        self.gamma = gamma
        self.filter_small_area = False

    def _feature_bytes(self, dim):
        return self._L.y7t_deepsort_feature_bytes(self.cap_t, self.cap_d, dim, STORE_FEATURES_BUDGET)

    def _feature_init(self, nbytes):      # the per-slot rings of the last STORE_FEATURES_BUDGET vectors
        return self._L.y7t_deepsort_init(_lib.ptr(self._feat), nbytes, self.cap_t, self.cap_d, self._feat_dim, STORE_FEATURES_BUDGET, _lib.stream_ptr())

    def _step(self, d, n, feats, warp, out):      # (no camera-motion compensation in deepsort.py: warp is not read)
        optr, cptr = self._out_ptrs(out)
        self._det_keep = (d, feats)
        _lib.check(self._L.y7t_tracker_step_deepsort(_lib.ptr(self._state), _lib.ptr(self._feat), self.cap_t, _lib.ptr(d), n, _lib.ptr(feats),
                                                     optr, self.cap_t, cptr, self.threads, _lib.stream_ptr()))
        self.frame_id += 1
        self._snap_cache = None
