"""mAP evaluation on the device: the device time of y7t_map_update for one batch of 80 images x 300 rows x 50 targets, of y7t_map_compute at 24 000 and
1.5 M stored rows (80 classes; the second is a COCO-val-sized run: 5000 images x 300 rows), the restatement's per-image loop and ap_per_class (tests/map_np.py) on
the host CPU in the same run, and the frames per second of the evaluation loop (yolov7-tiny, seeded weights, synthetic frames) with and without the update call --
the pair shows whether the update stays asynchronous: the loop never reads the statistics back.

    python scripts/time_map.py [--out profiles/map_timing.txt]

Device times are HIP events around `reps` back-to-back calls after a warm-up (tables already on the device)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_timing.txt"))
    ap.add_argument("--big", type=int, default=1500000)
    o = ap.parse_args()
    import torch
    from tests import map_np, map_scenes as sc
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.detector import evaluate as ev, model
    L = _lib.load()
    lines = ["mAP evaluation on the device (scripts/time_map.py), %s" % torch.cuda.get_device_name(0), ""]

    # ---- update: 80 images x 300 rows x 50 targets ----
    case = sc._batch(40, [(300, 50)] * 80, ncls=80)
    a = sc.raw_args(case)
    reps = 20
    dm = ev.DeviceMAP(80, 80 * 300 * (reps + 2))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in a.items() if k != "hw"}
    cap = a["cbox"].shape[1]
    up = lambda: dm.update_arrays(d["dets"], d["ndets"], d["keep"], d["cbox"], cap, cap, 80, d["targets"], d["toff"], a["hw"], d["lb"])
    ms = device_ms(up, reps)
    assert int(dm.header()[2].item()) == 0 and int(dm.header()[0].item()) == 24000 * (reps + 1)
    t0 = time.perf_counter()
    cor, conf, cls, tcls = map_np.batch_stats(case["preds"], case["targets"], case["hw"], case["lb"])
    cpu_loop = (time.perf_counter() - t0) * 1e3
    gconf, gcls, gcor, _ = dm.rows()
    assert np.array_equal(gcor[:24000], cor) and np.array_equal(gconf[:24000], conf)
    lines += ["update, one batch of 80 images x 300 rows x 50 targets (24 000 rows, 4000 targets):",
              "  device, y7t_map_update (2 launches)      %9.3f ms" % ms,
              "  CPU, the restatement's per-image loop    %9.1f ms   (torch box_iou + the Python walk; rows equal to the device's)" % cpu_loop, ""]

    # ---- compute ----
    for n in (24000, int(o.big)):
        nt = [max(1, n // 200) + (c * 37) % 50 for c in range(80)]
        case = sc._rows(60, n, nt)
        dm = ev.DeviceMAP(80, n)
        for k, arr in (("conf", case["conf"]), ("cls", case["cls"]), ("correct", sc.masks(case["tp"]))):
            dm.state[dm._off[k]:dm._off[k] + 4 * n].copy_(torch.from_numpy(arr.view(np.uint8).copy()))
        dm.state[dm._off["nt"]:dm._off["nt"] + 8 * 80].copy_(torch.from_numpy(case["nt"].astype(np.int64).view(np.uint8).copy()))
        dm.header()[0] = n
        outs = [torch.empty(s, dtype=t, device="cuda") for s, t in (((80, 10), torch.float64), ((80, 1000), torch.float64), ((80, 1000), torch.float64), (80, torch.int64),
                                                                    (80, torch.int32), (4, torch.int32))]
        comp = lambda: _lib.check(L.y7t_map_compute(_lib.ptr(dm.state), *[_lib.ptr(x) for x in outs], _lib.stream_ptr()))
        ms = device_ms(comp, 5)
        t0 = time.perf_counter()
        want = sc.expected_compute(case)
        cpu = (time.perf_counter() - t0) * 1e3
        p, r, apv, f1, classes = ev.finish(outs[0].cpu().numpy(), outs[1].cpu().numpy(), outs[2].cpu().numpy(), outs[4].cpu().numpy()[:int(outs[5][3].item())])
        err = max(float(np.abs(x - want[k]).max()) for k, x in (("ap", apv), ("p", p), ("r", r), ("f1", f1)))
        lines += ["compute, %d rows, 80 classes:" % n,
                  "  device, y7t_map_compute                  %9.3f ms   (largest |difference| to the CPU result %.2e)" % (ms, err),
                  "  CPU, ap_per_class of the restatement     %9.1f ms" % cpu, ""]
        del dm, outs

    # ---- the evaluation loop with and without the update ----
    spec, sd, seed = model.load_checkpoint("random:yolov7-tiny", None, 80)
    det = model.Detector(spec, sd, img_size=(640, 640), max_batch=16, seed=seed)
    batches = list(ev.synthetic_batches(64, 40, 640, 16))
    det.plant_objectness_bias(batches[0][0][:1].float() / 255.0, target=2000)
    fps = {}
    for update in (True, False, True, False):
        ev.evaluate(det, batches, 80, cap_rows=64 * 300, update=update, print_fn=lambda *x: None)
        fps.setdefault(update, []).append(64 / ev.evaluate.last["wall_s"])
    lines += ["evaluation loop, yolov7-tiny at 640 x 640, 64 synthetic frames in batches of 16, multi-label NMS at conf 0.001 (wall clock, second of two runs):",
              "  with the update call      %8.1f frames/s" % fps[True][1],
              "  without it                %8.1f frames/s" % fps[False][1], ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
