"""UAVMOT (the reference's tracker/uavmot.py: "MOT Meets Moving UAV", CVPR 2022): ByteTrack whose first association is re-solved with a fused
IoU + structure cost (the "AMF" pass: matching.local_relation_fuse_motion) whenever the plain 0.7 solve matches anything but the single pair (0, 0).
Same plugin surface as the reference; the frame step -- the AMF pass included -- runs as one device kernel of liby7t.so over the tracker's pool
(csrc/y7t_track_step.h: y7t_tracker_step_body_t<true>), like the other trackers of this package.

The reference's quirks are kept: the gate is `matched_pair0.any()` (the single match (0, 0) counts as none), and the second association's unmatched
indices, which point into the still-Tracked leftovers of the first, are applied to strack_pool (uavmot.py:222-225).
"""
import numpy as np

from .basetrack import STrack, BaseTracker, TrackState, _PoolTrack, joint_stracks, sub_stracks, remove_duplicate_stracks  # noqa: F401


class AMF_STrack(STrack):
    """A detection as the reference builds it (uavmot.py:14-66): an STrack with get_xy().  AMF_update / AMF_reactivate are defined there but never
    called; they are not ported."""

    def get_xy(self):
        """xc, yc for the AMF module (matching.structure_representation): tlwh2xywh(tlwh)[:2] -- tl + wh // 2, in the tlwh's dtype (float32)"""
        return self.tlwh2xywh(self.tlwh)[:2]


class _AMFPoolTrack(_PoolTrack):
    """View of one slot of a UAVMOT device pool (a _PoolTrack with get_xy)."""

    def get_xy(self):
        return self.tlwh2xywh(self.tlwh)[:2]


class UAVMOT(BaseTracker):
    """uavmot.py:70-256.  opts: conf_thresh, track_buffer, kalman_format, img_size (+ the optional capacities of BaseTracker)."""
    _KIND = 5  # Y7T_TRACKER_UAVMOT
    _VIEW = _AMFPoolTrack

    def __init__(self, opts, frame_rate=30, gamma=0.1, *args, use_apperance_model=False, **kwargs):
        # the reference sets use_apperance_model = False and constructs an Extractor(opts.reid_model_path) it never calls (uavmot.py:72-74); the
        # appearance path needs weights/ckpt.t7, which the reference does not ship -- nothing is constructed here
        if use_apperance_model:
            raise NotImplementedError("UAVMOT's appearance path needs the DeepSORT ReID weights (ckpt.t7), which the reference does not ship")
        super().__init__(opts, frame_rate=frame_rate)
        self.use_apperance_model = False
        self.gamma = gamma
        self.low_conf_thresh = max(0.15, self.opts.conf_thresh - 0.3)
        self.filter_small_area = False

    def _views(self, list_name, n_name):
        return [_AMFPoolTrack(t._pool, t._slot, t.track_id, t._tlwh_now, t.cls, t.score) for t in super()._views(list_name, n_name)]
