"""GPU cases of tests/test_track_cli_reid_family_gpu.py, which runs this file in a process of its own: tracker/track.py with the OSNet family as the appearance network: --reid_model_path random:<one of the reference's five OSNet constructors> selects the
general fp16 path (ReIDExtractor(half=True)) at the tracker's crop size, --reid_half sends random:osnet (or a checkpoint) there too.  yolov7-tiny on a 20-frame
synthetic scene with --synthetic_dets; each run must write results and hand the tracker 512-wide features."""
import os
import warnings

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tracker,path,half_flag,width,ibn,size", [
    ("strongsort", "random:osnet_x0_5", False, 0.5, False, (256, 128)),
    ("deepsort", "random:osnet_ibn_x1_0", False, 1.0, True, (64, 128)),
    ("strongsort", "random:osnet", True, 0.25, False, (256, 128)),
])
def test_track_cli_osnet_family(tmp_path, monkeypatch, tracker, path, half_flag, width, ibn, size):
    from yolov7_tracker_amd.tracker import reid, track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    seen = []
    inner = reid.ReIDExtractor.features_for_boxes

    def spy(self, frame, tlbrs):
        out = inner(self, frame, tlbrs)
        seen.append((tuple(out.shape), self.half, self.fused, self.spec["channels"][0], bool(self.spec.get("ibn")), (self.in_w, self.in_h)))
        return out
    monkeypatch.setattr(reid.ReIDExtractor, "features_for_boxes", spy)
    args = ["--dataset", "synthetic", "--tracker", tracker, "--reid_model_path", path, "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "640",
            "--synthetic_dets", "--synthetic_frames", "20", "--synthetic_objs", "20", "--results_root", str(tmp_path)] + (["--reid_half"] if half_flag else [])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        folder = track.cli(args)
    lines = open(os.path.join(folder, "synthetic-000.txt")).read().splitlines()
    assert len(lines) > 60 and len({ln.split(",")[0] for ln in lines}) >= 19 and all(len(ln.split(",")) == 10 for ln in lines)
    assert seen and all(s[0][1] == 512 and s[1] and not s[2] for s in seen), seen[:2]
    assert seen[0][3] == int(64 * width) and seen[0][4] == ibn and seen[0][5] == size
    assert sum(s[0][0] for s in seen) > 100


def test_unknown_random_arch_is_refused():
    import types
    from yolov7_tracker_amd.tracker.deepsort import DeepSORT
    with pytest.raises(ValueError, match="osnet_ibn_x1_0"):
        DeepSORT(types.SimpleNamespace(conf_thresh=0.05, track_buffer=30, kalman_format="default", img_size=640, iou_thresh=0.5, reid_model_path="random:osnet_x2_0"))
