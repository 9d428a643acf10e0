"""--classes / --agnostic_nms of the tracker CLI (the reference's detect.py:166-167): the parser accepts them and the values reach non_max_suppression through
post_process_v7 -- on the CPU with a recording stand-in, and on the GPU through track.cli on a short synthetic sequence, where the fused forward stays in use."""
import pytest
import torch


def test_parser_accepts_classes_and_agnostic_nms():
    from yolov7_tracker_amd.tracker import track
    p = track.build_parser()
    o = p.parse_args(["--classes", "0", "2", "--agnostic_nms"])
    assert o.classes == [0, 2] and o.agnostic_nms is True
    o = p.parse_args([])
    assert o.classes is None and o.agnostic_nms is False
    assert p.parse_args(["--classes", "5"]).classes == [5]
    with pytest.raises(SystemExit):
        p.parse_args(["--classes", "person"])


def test_post_process_v7_hands_the_options_to_the_nms(monkeypatch):
    from yolov7_tracker_amd.tracker import track
    seen = []

    def fake_nms(out, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, labels=()):
        seen.append((conf_thres, classes, agnostic, multi_label))
        return [torch.tensor([[10.0, 20.0, 50.0, 60.0, 0.75, 2.0]]), torch.zeros((0, 6))]

    monkeypatch.setattr(track, "non_max_suppression", fake_nms)
    res = track.post_process_v7(object(), (128, 128), (128, 128), all_images=True, classes=[0, 2], agnostic=True)
    assert seen == [(0.01, [0, 2], True, False)] and len(res) == 2 and res[0][0].tolist() == [10.0, 20.0, 50.0, 60.0, 0.75, 2.0]
    track.post_process_v7(object(), (128, 128), (128, 128))
    assert seen[1] == (0.01, None, False, False)                           # the defaults are the reference's call (track.py:239)


@pytest.mark.gpu
def test_track_cli_passes_classes_and_agnostic_nms(tmp_path, monkeypatch):
    """track.cli --classes 0 2 --agnostic_nms on six synthetic frames: every post_process_v7 call carries the two values, works on a FUSED forward's output, and returns
    rows of the listed classes only"""
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    calls, inner = [], track.post_process_v7

    def recording(out, *a, **k):
        res = inner(out, *a, **k)
        calls.append((out.fused, k.get("classes"), k.get("agnostic"), sorted({float(c) for r in res for c in r[:, 5].tolist()})))
        return res

    monkeypatch.setattr(track, "post_process_v7", recording)
    track.cli(["--dataset", "synthetic", "--tracker", "bytetrack", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "640", "--synthetic_dets",
               "--synthetic_frames", "6", "--synthetic_objs", "20", "--results_root", str(tmp_path), "--classes", "0", "2", "--agnostic_nms"])
    assert len(calls) == 6
    for fused, classes, agnostic, seen_cls in calls:
        assert fused == 0.01 and classes == [0, 2] and agnostic is True and set(seen_cls) <= {0.0, 2.0}
