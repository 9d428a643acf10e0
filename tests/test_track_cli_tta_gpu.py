"""GPU, through the tracker CLI: `--augment` (extension; detect.py / test.py --augment of the reference) routes detection through Detector.forward_augment.  The detector's
REAL augmented decode + NMS output feeds ByteTrack on a short synthetic sequence; the written result file equals the one produced by driving forward_augment +
post_process_v7 + the tracker by hand on the same frames."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--dataset", "synthetic", "--tracker", "bytetrack", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "256", "--synthetic_frames", "6",
        "--synthetic_objs", "20", "--conf_thresh", "0.05", "--min_area", "0"]


def test_track_cli_augment_equals_the_hand_driven_loop(tmp_path, monkeypatch):
    from yolov7_tracker_amd.detector import attempt_load, model
    from yolov7_tracker_amd.tracker import track, tracker_dataloader
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    calls = []
    inner = model.Detector.forward_augment
    monkeypatch.setattr(model.Detector, "forward_augment", lambda self, *a, **k: (calls.append(1), inner(self, *a, **k))[1])
    BaseTrack._count = 0
    folder = track.cli(ARGS + ["--augment", "--classes", "0", "1", "2", "3", "--agnostic_nms", "--results_root", str(tmp_path / "cli")])
    got = open(os.path.join(folder, "synthetic-000.txt")).read()
    assert len(calls) == 6, "every frame's detection went through forward_augment"
    monkeypatch.undo()

    opts = track.build_parser().parse_args(ARGS + ["--augment", "--classes", "0", "1", "2", "3", "--agnostic_nms", "--results_root", str(tmp_path / "hand")])
    det = attempt_load(opts.model_path, cfg=opts.model_cfg, nc=opts.nc, img_size=256, max_batch=1)
    loader = tracker_dataloader.SyntheticLoader(6, 20, 256, 0)
    BaseTrack._count = 0
    tracker = track.TRACKER_DICT["bytetrack"](opts, frame_rate=30, gamma=opts.gamma)
    results = []
    for f in range(len(loader)):
        img, img0 = loader[f]
        head = det.forward_augment(img[None].cuda(), conf_thres=0.01)
        out = track.post_process_v7(head, img_size=img.shape[1:], ori_img_size=img0.shape, classes=[0, 1, 2, 3], agnostic=True)
        tracks = tracker.update(out, img0)
        keep = [t for t in tracks if t.tlwh[2] * t.tlwh[3] > opts.min_area]
        results.append((f + 1, [t.track_id for t in keep], [t.tlwh for t in keep], [t.cls for t in keep]))
    track.save_results(str(tmp_path / "hand"), "by_hand", "synthetic-000", results)
    want = open(os.path.join(str(tmp_path / "hand"), "by_hand", "synthetic-000.txt")).read()
    assert got == want and len(got.splitlines()) > 0


def test_track_cli_augment_with_device_preprocess_is_the_same_file(tmp_path):
    """synthetic frames have the network's size: with --device_preprocess pass 0 reads the uint8 frame through the plain forward's input path and the scaled passes
    resample the same frame -- (float)u8 / 255 on the device is the loader's float32 image, so both runs write the same file"""
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    outs = []
    for extra in ([], ["--device_preprocess"]):
        BaseTrack._count = 0
        folder = track.cli(ARGS + ["--augment", "--results_root", str(tmp_path / ("r%d" % len(outs)))] + extra)
        outs.append(open(os.path.join(folder, "synthetic-000.txt")).read())
    assert outs[0] == outs[1] and len(outs[0].splitlines()) > 0


def test_augment_from_raw_frames_refuses_frames_that_need_letterboxing():
    from yolov7_tracker_amd.detector import attempt_load
    det = attempt_load("random:yolov7-tiny", nc=10, img_size=256, max_batch=1)
    with pytest.raises(ValueError, match="letterbox"):
        det.forward_frames_augment(torch.zeros((1, 200, 256, 3), dtype=torch.uint8), img_size=256)
    out, hw = det.forward_frames_augment(torch.zeros((1, 256, 256, 3), dtype=torch.uint8), img_size=256)
    assert hw == (256, 256) and out.shape[1] == sum(out.rows)
