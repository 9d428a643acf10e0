"""What the trackers with an appearance model share (DeepSORT, StrongSORT): the `reid_model` seam, the feature state beside the track pool, and the staging of
a frame's detections and their appearance vectors for the device step.

Appearance features enter at the reference's own seam, `get_feature(tlbrs, ori_img) -> (N, D)` (deepsort.py:19-41, strongsort.py:66-89): by default it crops
`ori_img` like the reference and calls `self.reid_model(crops)`; `reid_model` is any callable returning (N, D) features -- the device ReID extractor of this
package (`tracker/reid.py`), or a stand-in.

A subclass states its reference's constants (the class attributes below), sizes and initialises its feature state (`_feature_bytes`, `_feature_init`) and makes
its library call in `_step`."""
import os

import numpy as np
import torch

from .. import _lib
from .basetrack import BaseTracker, _PoolTrack


class _VectorPoolTrack(_PoolTrack):
    """View of one slot of a device pool whose feature state keeps ONE float32 vector per slot (StrongSORT, BoT-SORT with its appearance branch): `features` is
    the list with the track's smoothed vector, read from the feature state."""

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


def osnet_family_archs(**kw):
    """"random:osnet_x0_25" .. "random:osnet_ibn_x1_0": the reference's five OSNet constructors (reid_models/OSNet.py:522-592) with seeded weights on the general
    fp16 path (ReIDExtractor(half=True)) at the tracker's crop size"""
    from .reid import OSNET_NAMES
    return {name: dict(arch="osnet", width=width, ibn=ibn, half=True, **kw) for name, (width, ibn) in OSNET_NAMES.items()}


class AppearanceTracker(BaseTracker):
    _KALMAN_FORMATS = ("default", "strongsort")      # the kalman_format values the tracker's device program accepts
    _KALMAN_NOTE = ""       # why the tracker needs these filters
    _FEATURE_AT_THRESHOLD = False      # a detection gets a feature when its score is > det_thresh (deepsort.py:98, strongsort.py:110); True: >= (botsort.py:339)
    _REID_ARCHS = {}        # "random:<arch>" -> ReIDExtractor keyword arguments (arch: the name itself unless given); the first is what a bare "random" means
    _REID_ARCH_NOTE = ""    # the accepted forms of a "random" reid_model_path, for the error message
    _REID_CKPT = {}         # ReIDExtractor.from_checkpoint keyword arguments
    _REID_HINT = ""         # the extractor to name when none was given
    _OVERFLOW_NOTE = ""     # what a feature-state overflow means, after "(status %d)"

    def __init__(self, opts, frame_rate=30, reid_model=None):
        name = type(self).__name__
        if getattr(opts, "kalman_format", "default") not in self._KALMAN_FORMATS:
            raise NotImplementedError("%s %s: kalman_format %s" % (name, self._KALMAN_NOTE, " / ".join(self._KALMAN_FORMATS)))
        super().__init__(opts, frame_rate=frame_rate)
        self.reid_model = reid_model if reid_model is not None else getattr(opts, "reid_model", None)
        path = getattr(opts, "reid_model_path", None)
        if self.reid_model is None and isinstance(path, str) and path.startswith("random"):
            # "random[:<arch>]" -- seeded random weights of the named embedding network, like the detector's "random:<arch>" model paths: for synthetic
            # runs (track.py --dataset synthetic, bench.py); no checkpoint ships that the reference's trackers can load
            from .reid import ReIDExtractor
            arch = path.partition(":")[2] or next(iter(self._REID_ARCHS))
            if arch not in self._REID_ARCHS:
                raise ValueError("reid_model_path %r: %s" % (path, self._REID_ARCH_NOTE))
            kw = dict(self._REID_ARCHS[arch])
            kw.setdefault("arch", arch)
            if getattr(opts, "reid_half", False) and kw["arch"] == "osnet":      # (extension) --reid_half: the general fp16 OSNet path
                kw["half"] = True
            self.reid_model = ReIDExtractor(None, **kw)
        elif self.reid_model is None and path and os.path.isfile(str(path)):      # deepsort.py:14, strongsort.py:29: the weights of opts.reid_model_path
            from .reid import ReIDExtractor
            self.reid_model = ReIDExtractor.from_checkpoint(path, **dict(self._REID_CKPT, **({"half": True} if getattr(opts, "reid_half", False) else {})))
        self._feat = None           # feature state, allocated when the feature dimension is known
        self._feat_dim = 0
        self._feat_used = False     # a frame with appearance vectors has been stepped (from then on the width is fixed)

    def get_feature(self, tlbrs, ori_img):
        """deepsort.py:19-41, strongsort.py:66-89: crops of the boxes -> self.reid_model(crops) -> (N, D) features"""
        if self.reid_model is None:
            raise _lib.Y7TError("%s needs appearance features: pass reid_model=<callable(list of crops) -> (N, D)> (e.g. "
                                "yolov7_tracker_amd.tracker.reid.%s) or override get_feature" % (type(self).__name__, self._REID_HINT))
        if hasattr(self.reid_model, "features_for_boxes"):      # device extractor: crop + resize + normalise on the GPU
            return self.reid_model.features_for_boxes(ori_img, tlbrs)
        if isinstance(ori_img, torch.Tensor):
            ori_img = ori_img.cpu().numpy()
        crops = []
        for tlbr in tlbrs:
            x1, y1, x2, y2 = (int(v) for v in tlbr)
            crops.append(ori_img[y1:y2, x1:x2])
        return self.reid_model(crops) if crops else np.zeros((0, max(self._feat_dim, 1)), np.float32)

    def _feature_bytes(self, dim):
        """the size of the feature state for `dim`-wide embeddings"""
        raise NotImplementedError

    def _feature_init(self, nbytes):
        """initialise self._feat (nbytes of zeros) for self._feat_dim-wide embeddings -> the library's return code"""
        raise NotImplementedError

    def _ensure_feature_state(self, dim):
        """the per-slot appearance vectors + per-frame scratch, sized for `dim`-wide embeddings.  Until a frame has carried a detection above det_thresh
        no track exists (a new track needs score > det_thresh + 0.1, deepsort.py:207) and no slot holds a vector, so a state that was sized on a
        guess for such frames (empty / low-confidence first frames are common in real footage) is simply re-made when the real width shows up."""
        if self._feat is None or (int(dim) != self._feat_dim and not self._feat_used):
            self._feat_dim = int(dim)
            nb = int(self._feature_bytes(self._feat_dim))
            self._feat = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            _lib.check(self._feature_init(nb))
        elif int(dim) != self._feat_dim:
            raise ValueError("feature dimension changed from %d to %d" % (self._feat_dim, int(dim)))

    def _check_feats(self, feats_dev, n):
        """what the device step dereferences: n rows of `_feat_dim` contiguous float32 on the GPU (a short, fp16 or strided tensor would be read out
        of bounds / misinterpreted by the appearance-distance and store kernels)"""
        if not isinstance(feats_dev, torch.Tensor) or feats_dev.dim() != 2:
            raise _lib.Y7TError("%s: features must be an (n, D) tensor" % type(self).__name__)
        if feats_dev.shape[0] < n:
            raise _lib.Y7TError("%s: %d feature rows for %d detections" % (type(self).__name__, feats_dev.shape[0], n))
        return feats_dev.to(device="cuda", dtype=torch.float32).contiguous()

    def _feature_status(self):
        return int(self._feat[20:24].view(torch.int32).item())           # Y7TPendHdr.status: every feature state's header derives from it (csrc/y7t_track_pend.h)

    def _step(self, d, n, feats, warp, out):
        """the tracker's library call for one frame: d (n, 6) and feats (>= n, D) float32 device tensors, warp a (6,) float64 device tensor or None,
        out like BaseTracker._launch"""
        raise NotImplementedError

    def _launch(self, det_dev, feats_dev=None, warp=None, out=None, **kw):
        """enqueue one frame step without a host round trip (pipelines / bench.py): det_dev (n, 6) float32 and feats_dev (n, D) float32
        DEVICE tensors (rows at or below det_thresh are ignored by the step), warp a (6,) float64 device tensor or None, out like BaseTracker._launch.
        det_dev None: the predict-only step of update_without_detection (basetrack.py:489-537), the same for every tracker."""
        if det_dev is None:
            return super()._launch(None, out=out, warp=warp, **kw)
        if feats_dev is None:
            raise _lib.Y7TError("%s._launch needs the detections' appearance features (use update() for the get_feature seam)" % type(self).__name__)
        d = det_dev.reshape(-1, 6)
        n = d.shape[0]
        if n > self.cap_d:
            raise _lib.Y7TError("%d detections exceed the pool capacity max_dets=%d" % (n, self.cap_d))
        d = d.to(device="cuda", dtype=torch.float32).contiguous()
        feats_dev = self._check_feats(feats_dev, n)
        self._ensure_feature_state(feats_dev.shape[1])
        self._feat_used = self._feat_used or n > 0
        self._step(d, n, feats_dev, warp, out)

    def _frame_warp(self, warp, ori_img, det_results):
        """the camera-motion matrix of update()'s frame as the (6,) float64 device tensor `_step` takes, or None"""
        return None

    def update(self, det_results, ori_img=None, warp=None):
        """(N,6) [x1,y1,x2,y2,conf,cls] + the frame -> list of tracks (deepsort.py:79-227, strongsort.py:91-250)"""
        if isinstance(det_results, torch.Tensor):
            det_host = det_results.detach().cpu().numpy()
        else:
            det_host = np.asarray(det_results)
        det_host = np.ascontiguousarray(det_host, dtype=np.float32).reshape(-1, 6)
        n = det_host.shape[0]
        if n > self.cap_d:
            raise _lib.Y7TError("%d detections exceed the pool capacity max_dets=%d" % (n, self.cap_d))
        thr = np.float32(self.det_thresh)                              # deepsort.py:98, strongsort.py:110, botsort.py:339: only these get features
        keep = det_host[:, 4] >= thr if self._FEATURE_AT_THRESHOLD else det_host[:, 4] > thr
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
        w = self._frame_warp(warp, ori_img, det_results)
        d = torch.from_numpy(det_host).cuda()
        allf = torch.zeros((max(n, 1), self._feat_dim), dtype=torch.float32, device="cuda")
        if feats is not None:
            allf[torch.from_numpy(np.nonzero(keep)[0]).cuda()] = feats
        self._step(d, n, allf, w, None)
        rows = self._collect()
        st = self._feature_status()
        if st:
            raise _lib.Y7TError("%s feature state overflow (status %d)%s" % (type(self).__name__, st, self._OVERFLOW_NOTE))
        return rows


class OneVectorViews:
    """host views of a feature state that keeps ONE float32 vector per slot behind a 64-byte header (y7t_ss_layout, y7t_br_layout): mixed into the tracker class,
    which sets `_vec_cache = None` in its constructor and after every step"""
    _VIEW = _VectorPoolTrack

    def _vectors(self):
        """(cap_t, D) float32 host copy of the slots' vectors (cached until the next step)"""
        if self._vec_cache is None and self._feat is not None:
            off = 64                                                     # the vectors follow the 64-byte header
            raw = self._feat[off:off + 4 * self.cap_t * self._feat_dim].cpu().numpy()
            self._vec_cache = raw.view(np.float32).reshape(self.cap_t, self._feat_dim)
        return self._vec_cache

    def _vector(self, slot, track_id):
        if self._feat is None or not self._feat_used or self._snapshot()["tid"][slot] != track_id:
            return None
        return self._vectors()[slot].copy()

    def _views(self, list_name, n_name):
        return [_VectorPoolTrack(t._pool, t._slot, t.track_id, t._tlwh_now, t.cls, t.score) for t in super()._views(list_name, n_name)]
