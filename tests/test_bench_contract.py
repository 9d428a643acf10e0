"""CPU: the bench.py contract that can be checked without a GPU -- the command line the driver uses, the refusal to run without a device (no CPU
fallback), and the shape of the bench lines committed under profiles/ (what `python bench.py` printed on the MI355X): every key the driver and the judge
read, the arithmetic that ties them together, and the scope rules (value is whole-job throughput, roofline priced against the nominal peak,
cpu_baseline a bounded port run on stated cores, vs_baseline null while BASELINE.json publishes nothing)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(name):
    txt = open(os.path.join(ROOT, "profiles", name)).read().strip().splitlines()[-1]
    return json.loads(txt)


def test_bench_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert "no CPU fallback" in (r.stdout + r.stderr)
    assert not any(l.startswith("{") for l in r.stdout.splitlines())          # and prints no JSON line


def test_bench_command_line_is_the_drivers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in r.stdout
    sys.path.insert(0, ROOT)
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py"]
        a = bench.parse()
    finally:
        sys.argv = old
    assert a.gpus == 1 and 1 <= a.steps <= 50 and 0 <= a.warmup <= 20          # no flags: one GPU, a run of minutes
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    assert a.full is False and a.dump_outputs is None                          # a plain run: the headline only, nothing written


def test_dump_outputs_writes_what_a_caller_receives(tmp_path):
    """--dump-outputs: the last timed step's NMS rows and returned tracks, float32 / float64, rows past each frame's count zeroed"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    B, cap_t = 3, 16
    g = torch.Generator().manual_seed(0)
    dets = torch.rand((B, 300, 6), generator=g)
    ndets = torch.tensor([5, 0, 300], dtype=torch.int32)
    rows = torch.rand((B, cap_t + 1, 8), dtype=torch.float64, generator=g)
    counts = [4, 0, cap_t]
    for b, n in enumerate(counts):
        rows[b, cap_t].view(torch.int32)[0] = n
    bench.dump_outputs(str(tmp_path), dets, ndets, rows, cap_t)
    got = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}
    assert set(got) == {"detections", "detection_counts", "tracks", "track_counts"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["detection_counts"].tolist() == [5, 0, 300] and got["track_counts"].tolist() == counts
    d, t = got["detections"], got["tracks"]
    assert d.shape == (B, 300, 6) and t.shape == (B, cap_t, 7)
    for b in range(B):
        n = int(ndets[b])
        np.testing.assert_array_equal(d[b, :n], dets[b, :n].numpy())
        assert not d[b, n:].any()
        np.testing.assert_array_equal(t[b, :counts[b]], rows[b, :counts[b], :7].numpy())
        assert not t[b, counts[b]:].any()


def test_gpus_n_without_a_launcher_starts_n_ranks_itself():
    """VERDICT r2 missing 1: `python bench.py --gpus N` must be N ranks (one per GPU, RCCL), not an n_gpus = 1 line.  Without a launcher in the
    environment bench.py re-executes itself under torch.distributed.run -- the driver's own command line -- and refuses a WORLD_SIZE that disagrees."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "20", "--warmup", "5"],
                       env=dict(env, Y7T_BENCH_DRYRUN_LAUNCH="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    j = " ".join(cmd)
    assert "-m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port" in j
    assert j.endswith("bench.py --gpus 8 --steps 20 --warmup 5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "must agree" in (r.stdout + r.stderr)
    assert not any(l.startswith("{") for l in r.stdout.splitlines())
    # under an external launcher WITHOUT --gpus the world size is the launcher's (`torchrun --nproc-per-node 8 bench.py`) ...
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=dict(env, WORLD_SIZE="8", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert "must agree" not in (r.stdout + r.stderr)
    # ... and a container's stray WORLD_SIZE=1 (no RANK / LOCAL_RANK) is not a launcher: --gpus N still starts its own N ranks
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="1", Y7T_BENCH_DRYRUN_LAUNCH="1"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "--nproc-per-node 2" in " ".join(json.loads(r.stdout.strip().splitlines()[-1])["launch"]), r.stdout + r.stderr


@pytest.mark.parametrize("name,workload", [("r06_bench_line.json", "configs[1]"), ("r04_bench_line.json", "configs[1]"), ("r03_bench_line.json", "configs[1]"), ("r02_bench_line.json", "configs[1]"), ("r02_bench_line_cfg3.json", "configs[2]"),
                                           ("r02_bench_line_cfg4.json", "configs[3]")])
def test_committed_bench_lines_keep_the_contract(name, workload):
    l = _line(name)
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline"):
        assert k in l, k
    assert l["unit"] == "frames/s" and l["higher_is_better"] is True and l["scaling"] == "weak" and l["data"] == "synthetic" and l["dtype"] == "f16"
    assert l["metric"].startswith("end-to-end fps (detect+track)") and base["metric"].startswith("end-to-end fps (detect+track)")
    assert l["vs_baseline"] is None and base["published"] == {}                   # nothing published for this metric
    c = l["config"]
    assert workload in c["workload"] and "model" not in c
    # value = frames of all ranks / wall time of the timed steps
    fps = c["frames_per_step"] * c.get("sequences_per_gpu", 1) * l["n_gpus"] / (l["ms_per_step"] * 1e-3)
    assert abs(fps - l["value"]) / l["value"] < 0.02 or abs(c["frames_per_step"] * l["n_gpus"] / (l["ms_per_step"] * 1e-3) - l["value"]) / l["value"] < 0.02
    r = l["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0          # nominal dense fp16 peak, not the measured power-limited one
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0.0 < r["frac"] < 1.0
    # achieved = algorithmic FLOP of one launch list / its HIP-event duration
    assert abs(r["achieved"] - r["algorithmic_gflop_per_launch_list"] / r["launch_list_ms"]) / r["achieved"] < 0.01
    assert r["traffic"] is None or r["traffic"] > 0
    if workload == "configs[1]":          # the driver's line (the other workloads are parity / stress cases run with --workload)
        b = l["cpu_baseline"]
        assert b["kind"] == "port" and b["unit"] == "frames/s" and b["cores"] >= 1 and b["value"] > 0 and b["sample"]
        assert l["value"] > 10 * b["value"]


def test_headline_line_carries_parity_and_reference_semantics_fps():
    """round 3: `parity` describes the TIMED weights -- raw heads, every pre-NMS candidate at SURVEY 8a's bar, the final boxes -- and says which third-party
    kernels are unpinned; traffic is only printed for the launch list it was measured on"""
    l = _line("r03_bench_line.json")
    p = l["parity"]
    assert p["weights"] == "conditioned" and max(p["heads_mean_abs_err_over_logit_std"]) < 0.004
    c = p["candidates_before_nms"]
    assert c["n_both"] >= 1000 and c["frac_within_bar"] == 1.0 and c["n_class_differs"] == 0 and c["max_dcoord"] <= 1.0 and c["max_dconf"] <= 5e-3
    assert c["n_only_one_side"] <= 0.02 * c["n_both"] and c["max_margin_only_one_side"] <= 1e-3
    assert p["boxes_matched_same_class_1px_conf5e-3"] >= 0.97 * p["boxes_oracle"] and p["third_party"].startswith("unpinned")
    assert l["latency_mode"]["f32_chw_host"] and l["latency_mode"]["u8_hwc_host"] and l["fps_incl_h2d"]["value"] < l["value"] * 1.05
    r, t = l["roofline"], json.load(open(os.path.join(ROOT, "profiles", "r03_conv_hbm_traffic.json")))
    assert len(l["config"]["launch_list_sha"]) == 16 and t["launch_list_sha"] and t["commit"] != "unknown"
    assert (r["traffic"] is None) == (t["launch_list_sha"] != l["config"]["launch_list_sha"] or "not reported" in (r["traffic_note"] or ""))


def test_round4_line_measures_what_the_reference_timer_measures():
    """round 4: all four Detect levels live and EVERY candidate at SURVEY 8a's full bar, kept-set differences explained row by row, the
    track rows on the host inside the timed region, rotating input batches, the tracker-side roofline pieces, the reference's own speed beside the port's, and
    `traffic` reported because the committed PMC passes were taken on this very launch list"""
    l = _line("r04_bench_line.json")
    c = l["config"]
    assert c["track_rows_copied_to_host_inside_the_timed_region"] is True and c["input_batches_rotated"] >= 4
    p = l["parity"]
    cb = p["candidates_before_nms"]
    lv = cb["candidates_per_detect_level"]
    assert len(lv) == 4 and all(n >= 50 for n in lv) and sum(lv) == cb["n_got"]            # every Detect level supplies candidates (bench.LEVEL_QUOTA)
    assert cb["frac_within_bar"] == 1.0 and cb["n_out_of_coord_bar"] == 0 and cb["n_class_differs"] == 0 and cb["max_dconf"] <= 5e-3
    assert cb["min_iou_of_boxes_off_by_more_than_px"] >= 0.99                      # a candidate may miss the 1 px only if its IoU is >= 0.99
    bx = p["boxes_by_anchor_row"]
    assert bx["kept_by_one_side_only"] == sum(bx["reasons"].values()) and "unexplained" not in bx["reasons"]
    assert bx["kept_by_both"] >= 0.97 * bx["oracle_keeps"]
    rt = l["roofline_tracker"]
    assert rt["peak"] == 8000.0 and rt["unit"] == "GB/s" and {"kf_multi_predict_100_tracks", "iou_cost_500x500", "decode_nms_unfused"} <= set(rt["pieces"])
    for v in rt["pieces"].values():
        assert abs(v["achieved"] - v["algorithmic_bytes"] * v.get("frames_per_launch", 1) / (v["us_per_frame"] * v.get("frames_per_launch", 1) * 1e3)) / v["achieved"] < 0.02
    rop = l["cpu_baseline"]["reference_over_port"]
    assert 0 < rop["as_its_cli_runs_it_no_no_grad"] < rop["with_no_grad"] < 1.0        # the reference itself is slower than the port that is timed
    t = json.load(open(os.path.join(ROOT, "profiles", "r04_conv_hbm_traffic.json")))
    assert t["launch_list_sha"] == c["launch_list_sha"] and len(t["commit"]) == 40
    assert l["roofline"]["traffic"] is None or abs(l["roofline"]["traffic"] - t["hbm_bytes_per_frame"] * 32 / 1e9) / l["roofline"]["traffic"] < 0.05 or l["roofline"]["traffic"] > 0


def test_round6_line_carries_the_coupled_passes_and_says_what_value_is():
    """round 6: the tracker fed by the step's own NMS rows on the device is TIMED (`coupled`: the rows as they are; `coupled_confident_rows`: with the
    score gain that gives the tracker the headline's association load), `value` says which pass it is and why, the CPU baseline says why it does not use every core, the
    roofline object carries the re-measured random-operand ceiling, and the PMC traffic belongs to this very launch list"""
    l = _line("r06_bench_line.json")
    assert "never `value`" in l["value_note"] and l["fps_incl_h2d"]["value"] > 0
    c, cc = l["coupled"], l["coupled_confident_rows"]
    for v in (c, cc):
        assert v["fps"] > 0 and v["tracker_status"] == 0 and v["launch_list_ms"] > 0 and v["tracker_chain_ms"] > 0 and v["note"]
    assert c["score_gain_in_the_handover"] == 1.0 and cc["score_gain_in_the_handover"] > 1.0
    assert c["nms_rows_per_frame_mean"] > 100                                                     # the tracker reads the full NMS output, most of it below its thresholds
    assert cc["rows_at_or_above_0.3_0.2_0.15_mean"][1] >= 0.5 * l["config"]["dets_per_frame_timed_mean"]      # ... and with the gain as many confident rows as the scene has detections
    assert cc["tracks_per_frame_mean"] > c["tracks_per_frame_mean"]
    b = l["cpu_baseline"]
    assert b["kind"] == "port" and b["cores"] <= b["host_cpu_count"] and "thrash" in b["why_not_every_core"] and str(b["cores"]) in b["detector_s_per_frame_by_threads"]
    r = l["roofline"]
    assert r["sustained_peak"] == 1627.0 and abs(r["frac_of_sustained_peak"] - r["achieved"] / 1627.0) < 1e-3
    t = json.load(open(os.path.join(ROOT, "profiles", "r06_conv_hbm_traffic.json")))
    assert t["launch_list_sha"] == l["config"]["launch_list_sha"] and len(t["commit"]) == 40 and t["frames_per_launch_list"] == l["config"]["frames_per_step"]
    assert r["traffic"] is not None and abs(r["traffic"] - t["hbm_bytes_per_frame"] * t["frames_per_launch_list"]) / r["traffic"] < 0.05
    ow = l["other_workloads"]
    assert ow["cfg3"]["fps"] > 0 and ow["cfg4"]["fps"] > 0 and ow["cfg4"]["roofline_reid"]["frac"] > 0
    lm = l["latency_mode"]
    assert lm["u8_hwc_host"]["fps"] > lm["f32_chw_host"]["fps"] > 300
