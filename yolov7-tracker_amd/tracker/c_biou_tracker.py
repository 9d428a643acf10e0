"""C-BIoU (the reference's tracker/c_biou_tracker.py: "Hard to Track Objects with Irregular Motions and Similar Appearances? Make It Easier by
Buffering the Matching Space"): no Kalman filter, three IoU associations of buffered boxes.  Same plugin surface as the reference; the frame
step runs as one device kernel of liby7t.so over the tracker's pool (csrc/y7t_track_cbiou.h), like the other trackers of this package.
"""
import copy
from collections import deque

import numpy as np

from .. import _lib
from .basetrack import BaseTrack, BaseTracker, TrackState, joint_stracks, sub_stracks, remove_duplicate_stracks  # noqa: F401


class C_BIoUSTrack(BaseTrack):
    """A detection as the reference builds it (c_biou_tracker.py:17-62): float32 tlwh, its two buffered boxes and the motion states they start.
    Host-side object; the tracks of a C_BIoUTracker are views of its device pool (_C_BIoUPoolTrack)."""
    b1, b2, n = 0.3, 0.5, 5

    def __init__(self, cls, tlwh, score):
        self.cls = cls
        self._tlwh = np.asarray(tlwh, dtype=np.float32)
        self.score = score
        self.is_activated = False
        self.tracklet_len = 0
        self.track_id = None
        self.start_frame = None
        self.frame_id = None
        self.time_since_update = 0
        self.origin_bbox_buffer = deque([self._tlwh])
        self.buffer_bbox1 = self.get_buffer_bbox(level=1)
        self.buffer_bbox2 = self.get_buffer_bbox(level=2)
        self.motion_state1 = self.buffer_bbox1.copy()
        self.motion_state2 = self.buffer_bbox2.copy()

    def get_buffer_bbox(self, level=1, bbox=None):
        """tlwh + [-b*w, -b*h, 2b*w, 2b*h], clamped at 0 (c_biou_tracker.py:48-62; numpy's own promotion decides the dtype)"""
        assert level in [1, 2], 'level must be 1 or 2'
        b = self.b1 if level == 1 else self.b2
        if bbox is None:
            bbox = self._tlwh
        return np.maximum(0.0, bbox + np.array([-b * bbox[2], -b * bbox[3], 2 * b * bbox[2], 2 * b * bbox[3]]))

    @property
    def tlbr(self):
        ret = self.tlwh.copy()
        ret[2:] += ret[:2]
        return ret

    @property
    def tlwh(self):
        return self.origin_bbox_buffer[-1].copy()

    @staticmethod
    def tlbr2tlwh(tlbr):
        result = np.asarray(tlbr).copy()
        result[2] -= result[0]
        result[3] -= result[1]
        return result

    @staticmethod
    def tlwh2tlbr(tlwh):
        result = np.asarray(tlwh).copy()
        if len(result.shape) > 1:
            result[:, 2:] += result[:, :2]
        else:
            result[2:] += result[:2]
        return result

    def __repr__(self):
        return 'OT_{}_({}-{})'.format(self.track_id, self.start_frame, self.end_frame)


def _view_only(self, *a, **k):
    raise _lib.Y7TError("this track is a view of a device track pool: its state changes only inside the tracker's fused step (y7t_tracker_step)")


class _C_BIoUPoolTrack(C_BIoUSTrack):
    """View of one slot of a C-BIoU device pool.  `track_id`, `tlwh`, `cls`, `score` come from the rows the step kernel returned; everything else is
    read back lazily from a snapshot of the pool (the slot's per-track state: csrc/y7t_track_cbiou.h)."""

    def _snap(self, name):
        if self._pool._snapshot()["tid"][self._slot] != self.track_id:
            raise _lib.Y7TError("track %d is no longer in the device pool" % self.track_id)
        return self._pool._snapshot()[name][self._slot]

    def _boxes(self, lo, hi):
        return np.asarray(self._snap("cov")[lo:hi], dtype=self._pool._box_dtype)

    state = property(lambda self: int(self._snap("state")))
    is_activated = property(lambda self: bool(self._snap("act")))
    frame_id = property(lambda self: int(self._snap("frame")))
    start_frame = property(lambda self: int(self._snap("start")))
    time_since_update = property(lambda self: int(self._snap("tsu")))
    tracklet_len = property(lambda self: int(self._snap("len")))
    _tlwh = property(lambda self: self._snap("box").copy())
    motion_state1 = property(lambda self: self._boxes(24, 28))
    motion_state2 = property(lambda self: self._boxes(28, 32))
    buffer_bbox1 = property(lambda self: self._boxes(36, 40))
    buffer_bbox2 = property(lambda self: self._boxes(40, 44))

    @property
    def origin_bbox_buffer(self):
        c = self._snap("cov")
        return deque(np.asarray(c[4 * k:4 * k + 4], dtype=np.float32) for k in range(int(c[32])))

    @property
    def tlwh(self):
        if self._epoch == self._pool.frame_id:
            return self._tlwh_now.astype(np.float32)
        return self._snap("box").copy()

    activate = update = re_activate = mark_lost = mark_removed = _view_only

    @classmethod
    def of_slot(cls, tracker, slot, s):
        """the view of `slot` in the pool snapshot `s` (tracked_stracks / lost_stracks)"""
        o = cls.__new__(cls)
        o.__dict__ = {"_pool": tracker, "_slot": int(slot), "_epoch": tracker.frame_id, "track_id": int(s["tid"][slot]),
                      "_tlwh_now": s["box"][slot].astype(np.float64), "cls": s["cls"][slot], "score": s["score"][slot]}
        return o


class C_BIoUTracker(BaseTracker):
    """c_biou_tracker.py:212-353.  opts: conf_thresh, track_buffer, img_size (+ the optional capacities of BaseTracker); kalman_format is not used."""
    _KIND = 4  # Y7T_TRACKER_C_BIOU
    _VIEW = _C_BIoUPoolTrack

    def __init__(self, opts, frame_rate=30, *args, **kwargs):
        # the reference lets BaseTracker build a Kalman filter and drops it (c_biou_tracker.py:216); the device pool of this tracker has none
        # (the library ignores the Kalman kind), so any kalman_format is accepted
        o = copy.copy(opts)
        o.kalman_format = 'default'
        super().__init__(o, frame_rate=frame_rate)
        self.opts = opts
        self.kalman = None
        # dtype of the buffered boxes and motion states: float32 under numpy >= 2 (NEP 50), float64 under numpy 1.x
        self._box_dtype = np.float32 if self._flags & 1 else np.float64

    def update_without_detection(self, det_results=None, ori_img=None):
        """BaseTracker.update_without_detection (basetrack.py:489-537) predicts the pool with STrack.multi_predict, which reads the Kalman mean a
        C_BIoUSTrack does not have: the reference fails there as soon as the pool (confirmed tracked + lost) holds a track.  With an empty pool the
        frame only advances."""
        s = self._snapshot()
        tracked = s["tracked"][:s["hdr_n_tracked"]]
        if s["hdr_n_lost"] > 0 or bool(np.any(s["act"][tracked])):
            raise NotImplementedError("C-BIoU has no motion model: update_without_detection would predict the pool's tracks with STrack.multi_predict "
                                      "(basetrack.py:489-537), which needs a Kalman mean -- the reference fails here too")
        return super().update_without_detection(det_results, ori_img)

    def _views(self, list_name, n_name):
        s = self._snapshot()
        return [_C_BIoUPoolTrack.of_slot(self, slot, s) for slot in s[list_name][:s[n_name]]]

