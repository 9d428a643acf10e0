"""GPU: the tracker CLI with --device_decode (after the --device_preprocess CLI test of tests/test_cli_gpu.py): a folder of JPEG frames on disk, the detector's real
decode + NMS output feeding the tracker.  The frames the device decodes are byte for byte the frames PIL decodes, so the result files -- and with --save_images the
written .jpg files -- must be identical with --device_preprocess and with --device_decode, also when one file of the folder is progressive and falls back to PIL."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sequence(root, progressive_at=None):
    from PIL import Image
    seq = root / "seqs" / "uav0001"
    seq.mkdir(parents=True)
    rng = np.random.default_rng(0)
    small = rng.integers(0, 256, (64 // 8 + 4, 96 // 8 + 4, 3)).astype(np.float32)
    big = np.kron(small, np.ones((8, 8, 1), np.float32)).astype(np.uint8)
    for i in range(6):                                     # a slowly panning scene of six 96 x 64 frames
        Image.fromarray(big[2 * i:2 * i + 64, 3 * i:3 * i + 96]).save(seq / ("%07d.jpg" % (i + 1)), quality=90, progressive=(i == progressive_at))
    return {'DATASET_ROOT': str(root), 'SEQ_SUBDIR': 'seqs', 'CERTAIN_SEQS': [None], 'IGNORE_SEQS': [None], 'CATEGORY_DICT': {}, 'YAML_DICT': ''}


@pytest.mark.parametrize("progressive_at,extra", [(None, []), (3, ["--batch", "4"]), (None, ["--save_images", "--batch", "2"])],
                         ids=["baseline", "one_progressive_file", "save_images"])
def test_track_cli_device_decode_equals_device_preprocess(tmp_path, progressive_at, extra):
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    outs, images = [], []
    for k, flag in enumerate(["--device_preprocess", "--device_decode"]):
        cfgs = _sequence(tmp_path / ("data%d" % k), progressive_at)      # (a data root per run: --save_images writes under it)
        BaseTrack._count = 0
        opts = track.build_parser().parse_args(["--dataset", "visdrone", "--tracker", "sort", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "96",
                                                "--min_area", "0", "--conf_thresh", "0.05", "--results_root", str(tmp_path / ("res%d" % k)), flag] + extra)
        folder = track.main(opts, cfgs)
        outs.append(open(os.path.join(folder, "uav0001.txt")).read())
        image_dir = os.path.join(cfgs['DATASET_ROOT'], 'result_images', 'uav0001')
        images.append({n: open(os.path.join(image_dir, n), "rb").read() for n in sorted(os.listdir(image_dir))} if os.path.isdir(image_dir) else {})
    assert track.decode_counts["uav0001"] == {'device': 6 - (progressive_at is not None), 'host': int(progressive_at is not None)}
    assert outs[0] == outs[1]
    assert images[0] == images[1] and len(images[0]) == (6 if "--save_images" in extra else 0)
