"""Records tests/golden/map_match.npz and tests/golden/map_compute.npz from the seeded cases of tests/map_scenes.py, with the REFERENCE's own functions (they must
be importable: oracle/ref_harness.py; the tests need only the recorded files).

    python tests/golden/make_golden_map.py

  map_match.npz    per matching case `<name>.correct / .conf / .cls / .nt`: the literal per-image loop of tests/map_np.py run with the reference's
                   utils.general.box_iou, scale_coords and xywh2xyxy in place of the restatement's
  map_compute.npz  per compute case `<name>.p / .r / .ap / .f1 / .classes`: the reference's ap_per_class itself (utils/metrics.py, reached through
                   utils.general.fitness.__globals__: a direct import of utils.metrics runs into its circular import)

The reference alone is deterministic only under two conditions, which the recorder ASSERTS for every case it records: all confidences of a case are distinct
(np.argsort(-conf) is not a stable sort), and no prediction has two same-class targets at exactly equal IoU.  Equal confidences are tested against tests/map_np.py
only."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_harness      # noqa: E402
from tests import map_np, map_scenes as sc      # noqa: E402


def main():
    g = ref_harness.load_detector().general
    ref_ap_per_class = g.fitness.__globals__["ap_per_class"]

    def ref_scale(coords, lb):
        gain, padx, pady, h0, w0 = (float(v) for v in lb)
        return g.scale_coords((1, 1), coords, (h0, w0), ((gain, gain), (padx, pady)))

    def ref_stats(pred, labels, hw, lb):
        saved = map_np.box_iou, map_np.scale_coords, map_np.xywh2xyxy
        map_np.box_iou, map_np.scale_coords, map_np.xywh2xyxy = g.box_iou, ref_scale, g.xywh2xyxy
        try:
            return map_np.image_stats(pred, labels, hw, lb, box_iou_fn=g.box_iou)
        finally:
            map_np.box_iou, map_np.scale_coords, map_np.xywh2xyxy = saved

    out = {}
    for name, make in sc.MATCH_CASES.items():
        case = make()
        confs = np.concatenate([p[:, 4].numpy() for p in case["preds"]])
        assert len(np.unique(confs)) == len(confs), "%s: equal confidences" % name
        for b, pred in enumerate(case["preds"]):      # no prediction with two same-class targets at exactly equal best IoU
            lab = case["targets"][case["targets"][:, 0] == b, 1:]
            if len(pred) and len(lab):
                pn, tb = map_np.native_boxes(pred, lab, case["hw"], case["lb"][b])
                iou = g.box_iou(pn, tb).numpy()
                same = pred[:, 5].numpy()[:, None] == lab[:, 0].numpy()[None, :]
                for p in range(len(pred)):
                    v = iou[p][same[p]]
                    assert len(v) < 2 or (v == v.max()).sum() == 1 or v.max() == 0, "%s: image %d prediction %d has tied targets" % (name, b, p)
        cor, conf, cls, nt = sc.expected_stats(case, ref_stats)
        mine = sc.expected_stats(case)
        assert all(np.array_equal(a, b) for a, b in zip((cor, conf, cls, nt), mine)), "%s: the restatement differs from the reference's functions" % name
        assert np.array_equal(cor, sc.expected_stats(case, map_np.image_stats_rule)[0]), "%s: the parallel rule differs from the literal loop" % name
        out.update({name + ".correct": cor, name + ".conf": conf, name + ".cls": cls, name + ".nt": nt})
        print("%-12s rows %4d  true at 0.5: %3d  at 0.95: %3d" % (name, len(cor), int(cor[:, 0].sum()) if len(cor) else 0, int(cor[:, 9].sum()) if len(cor) else 0))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "map_match.npz"), **out)

    out = {}
    for name, make in sc.COMPUTE_CASES.items():
        case = make()
        assert len(np.unique(case["conf"])) == len(case["conf"]), "%s: equal confidences" % name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            ref = sc.expected_compute(case, ref_ap_per_class)
        mine = sc.expected_compute(case)
        for k in ("p", "r", "ap", "f1", "classes"):
            assert np.array_equal(ref[k], mine[k]), "%s: the stable-order restatement differs from the reference in %s" % (name, k)
            out[name + "." + k] = ref[k]
        print("%-12s rows %6d  classes %3d  mean AP@.5 %.6f" % (name, len(case["conf"]), len(ref["classes"]), ref["ap"][:, 0].mean() if len(ref["ap"]) else 0.0))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "map_compute.npz"), **out)


if __name__ == "__main__":
    main()
