"""GPU: GSI on the device (csrc/y7t_gsi.hip; DESIGN.md section 4 "GSI").

The two statements of tests/test_gsi_cpu.py for the device: interpolated rows, offsets and source indices ARRAY-EQUAL to the recording; every smoothed value within
4 E of the recorded 50-digit solution (E = the NumPy float64 restatement's own largest distance to it; the margin of 4 allows for another summation order and a
one-ulp exp), on every track of the set -- 1 to 300 rows, either side of the LDS / HBM switch, both clips of the length scale -- with every status word clear.
A track's result is the same bits from call to call, alone or in the full batch, with the batch reversed, and from an object with fewer slots than tracks.  A
planted singular system (two equal frames, regularisation switched off through the ABI) sets its track's bit and leaves the track as it came.  Then the CLI."""
import os

import numpy as np
import pytest

from tests import gsi_np, gsi_scenes as sc

pytestmark = pytest.mark.gpu

NAMES = sorted(sc.SCENES)


@pytest.fixture(scope="module")
def model():
    from yolov7_tracker_amd.tracker.gsi import DeviceGSI
    return DeviceGSI(max_tracks=64, max_rows=2048, max_len=300)


def test_constants_are_the_headers():
    from tests._hostsim import gsi as hs
    assert hs.constants() == dict(lds_len=128, max_len=4096)      # the fixture's 128- and 129-row tracks sit either side of the switch


@pytest.mark.parametrize("name", NAMES)
def test_interpolation_is_array_equal_to_the_recording(model, name):
    s = sc.goldens()[name]
    got = model.interpolate(s["runs_in"], s["offsets_in"], int(s["interval"]))
    assert got["count"] == len(s["runs"]) and got["status"] == 0
    assert np.array_equal(got["runs"].view(np.uint64), s["runs"].view(np.uint64))
    assert np.array_equal(got["offsets"], s["offsets"]) and np.array_equal(got["src"], s["src"])


def test_interpolation_reports_overflow_and_writes_inside_its_capacity():
    from yolov7_tracker_amd.tracker.gsi import DeviceGSI
    s = sc.goldens()["t10"]
    tight = DeviceGSI(max_tracks=16, max_rows=len(s["runs"]) - 1, max_len=299)
    got = tight.interpolate(s["runs_in"], s["offsets_in"], 20)
    assert got["status"] == 3 and got["count"] == len(s["runs"]) and np.array_equal(got["offsets"], s["offsets"])
    assert np.array_equal(got["runs"], s["runs"][:-1]) and np.array_equal(got["src"], s["src"][:-1])


@pytest.mark.parametrize("name", NAMES)
def test_smoothed_columns_within_4E_of_the_exact_solution(model, name):
    s = sc.goldens()[name]
    E, bound = sc.bound()
    got, status = model.smooth(s["runs"], s["offsets"], s["len_scale"])
    assert not status.any()
    errs = [float(np.abs(got[lo:hi] - s["exact"][lo:hi]).max()) for lo, hi in zip(s["offsets"][:-1], s["offsets"][1:])]
    print("%s: device max |smoothed - exact| = %.3g   E = %.3g   bound 4 E = %.3g   per track %s" % (name, max(errs), E, bound, " ".join("%.2g" % e for e in errs)))
    assert max(errs) <= bound


def test_both_stages_back_to_back_give_the_same_bits(model):
    s = sc.goldens()["t10"]
    lens = np.diff(s["offsets"])
    res = model.run(s["runs_in"], s["offsets_in"], s["len_scale"], int(s["interval"]), longest=int(lens.max()))
    want, _ = model.smooth(s["runs"], s["offsets"], s["len_scale"])
    assert res["status"] == 0 and not res["track_status"].any() and np.array_equal(res["runs"], s["runs"]) and np.array_equal(res["src"], s["src"])
    assert np.array_equal(res["cols"].view(np.uint64), want.view(np.uint64))


def test_a_tracks_result_is_bit_identical_whatever_surrounds_it(model):
    from yolov7_tracker_amd.tracker.gsi import DeviceGSI
    s = sc.goldens()["t10"]
    off = s["offsets"]
    a, _ = model.smooth(s["runs"], off, s["len_scale"])
    model.smooth(sc.goldens()["t6p5"]["runs"], sc.goldens()["t6p5"]["offsets"], sc.goldens()["t6p5"]["len_scale"])      # other data in between
    b, _ = model.smooth(s["runs"], off, s["len_scale"])
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # alone
    for k in (0, 3, 9, 10, 12):      # 1, 16, 128, 129 and 300 rows
        lo, hi = int(off[k]), int(off[k + 1])
        c, st = model.smooth(s["runs"][lo:hi], [0, hi - lo], s["len_scale"][k:k + 1])
        assert st.tolist() == [0] and np.array_equal(c.view(np.uint64), a[lo:hi].view(np.uint64)), k
    # the batch reversed
    order = np.arange(len(off) - 1)[::-1]
    runs_r = np.concatenate([s["runs"][off[k]:off[k + 1]] for k in order])
    off_r = np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in order])]).astype(np.int32)
    d, st = model.smooth(runs_r, off_r, s["len_scale"][order])
    assert not st.any()
    for j, k in enumerate(order):
        assert np.array_equal(d[off_r[j]:off_r[j + 1]].view(np.uint64), a[off[k]:off[k + 1]].view(np.uint64)), k
    # an object with fewer slots than tracks: the thirteen tracks go in groups of three (128, 129 and 131 rows share one group and two pool slots)
    small = DeviceGSI(max_tracks=3, max_rows=len(s["runs"]), max_len=300)
    e, st = small.smooth(s["runs"], off, s["len_scale"])
    assert not st.any() and np.array_equal(e.view(np.uint64), a.view(np.uint64))


def test_a_singular_system_sets_its_bit_and_leaves_the_track(model):
    """two equal frames survive only because the regularisation is switched off through the ABI: the second pivot is exactly zero (1 - 1 * 1)"""
    runs = np.array([[5, 1, 2, 3, 4], [5, 9, 8, 7, 6], [1, 10, 20, 30, 40], [2, 11, 21, 31, 41], [3, 12, 22, 32, 42]], np.float64)
    got, status = model.smooth(runs, [0, 2, 5], [3.0, 3.0], reg=0.0)
    assert status.tolist() == [1, 0] and np.array_equal(got[:2], runs[:2, 1:]) and np.isfinite(got).all()
    assert np.abs(got[2:] - gsi_np.smooth_track(runs[2:, 0], runs[2:, 1:], 3.0, 0.0)).max() < 1e-9


def test_bad_arguments_are_refused_with_the_documented_codes(model):
    import torch
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker.gsi import DeviceGSI, GSI
    L = _lib.load()
    E_ARG, E_CAPACITY, E_STATE = -1, -3, -4
    for caps in ((0, 1, 1), (32769, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 4097)):
        assert L.y7t_gsi_workspace_bytes(*caps) == 0
    nbytes = int(L.y7t_gsi_workspace_bytes(4, 64, 32))
    blob = torch.zeros(nbytes + 512, dtype=torch.uint8, device="cuda")
    base = blob.data_ptr() + (-blob.data_ptr()) % 256
    st = _lib.stream_ptr()
    runs = torch.zeros((8, 5), dtype=torch.float64, device="cuda")
    runs[:, 0] = torch.arange(8)
    off = torch.tensor([0, 8], dtype=torch.int32, device="cuda")
    ls = torch.ones(1, dtype=torch.float64, device="cuda")
    out = torch.zeros((8, 4), dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.y7t_gsi_smooth(base, runs.data_ptr(), off.data_ptr(), ls.data_ptr(), 1, 8, 1e-10, out.data_ptr(), status.data_ptr(), st) == E_STATE      # never initialised
    assert L.y7t_gsi_init(base + 16, nbytes, 4, 64, 32, st) == E_ARG          # misaligned
    assert L.y7t_gsi_init(base, nbytes - 1, 4, 64, 32, st) == E_ARG           # too small
    assert L.y7t_gsi_init(base, nbytes, 0, 64, 32, st) == E_ARG
    assert L.y7t_gsi_init(base, nbytes, 4, 64, 32, st) == 0
    assert L.y7t_gsi_smooth(base, runs.data_ptr(), off.data_ptr(), ls.data_ptr(), 1, 33, 1e-10, out.data_ptr(), status.data_ptr(), st) == E_CAPACITY      # before any launch
    assert b"33 rows" in L.y7t_last_error()
    assert L.y7t_gsi_smooth(base, runs.data_ptr(), None, ls.data_ptr(), 1, 8, 1e-10, out.data_ptr(), status.data_ptr(), st) == E_ARG
    assert L.y7t_gsi_smooth(base, runs.data_ptr(), off.data_ptr(), ls.data_ptr(), 1, 8, -1.0, out.data_ptr(), status.data_ptr(), st) == E_ARG
    assert L.y7t_gsi_smooth(base, None, off.data_ptr(), None, 0, 0, 1e-10, None, None, st) == 0
    # a track longer than the `longest` the caller states is flagged and left, not smoothed
    assert L.y7t_gsi_smooth(base, runs.data_ptr(), off.data_ptr(), ls.data_ptr(), 1, 7, 1e-10, out.data_ptr(), status.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [2] and torch.equal(out, runs[:, 1:])
    head = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert L.y7t_gsi_interpolate(base, None, off.data_ptr(), 0, 20, None, off.data_ptr(), None, head.data_ptr(), head.data_ptr() + 4, st) == 0
    assert L.y7t_gsi_interpolate(base, None, off.data_ptr(), 1, 20, None, off.data_ptr(), None, head.data_ptr(), head.data_ptr() + 4, st) == E_ARG
    assert L.y7t_gsi_release(base) == 0
    assert L.y7t_gsi_interpolate(base, None, off.data_ptr(), 0, 20, None, off.data_ptr(), None, head.data_ptr(), head.data_ptr() + 4, st) == E_STATE
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        DeviceGSI(max_len=4097)
    with pytest.raises(_lib.Y7TError, match=r"track id 87 has 300 rows"):
        GSI(DeviceGSI(16, 2048, 299)).apply(sc.goldens()["t10"]["rows_in"])


@pytest.mark.parametrize("name", NAMES)
def test_apply_returns_the_recorded_rows_within_the_bound(model, name):
    from yolov7_tracker_amd.tracker.gsi import GSI
    s = sc.goldens()[name]
    out = GSI(model, int(s["interval"]), float(s["tau"])).apply(s["rows_in"])
    want = s["rows_out"]
    assert out.shape == want.shape and np.array_equal(out[:, :2], want[:, :2]) and np.array_equal(out[:, 6:], want[:, 6:])
    assert np.abs(out[:, 2:6] - want[:, 2:6]).max() <= 2 * sc.bound()[1]      # (both sides lie within 4 E of the exact columns)


def _rows_of(path):
    return np.array([[float(v) for v in line.split(",")[:6]] for line in open(path).read().splitlines()], np.float64).reshape(-1, 6)


def test_track_cli_fills_the_frames_the_tracker_missed(tmp_path):
    """plumbing: a short ByteTrack run over scene detections with misses, without and with --gsi, and with --aflink in front of it"""
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    from yolov7_tracker_amd.tracker.gsi import GSI, DeviceGSI
    common = ["--dataset", "synthetic", "--tracker", "bytetrack", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "320", "--synthetic_dets",
              "--synthetic_frames", "40", "--synthetic_objs", "12", "--synthetic_miss", "0.2"]
    files = []
    for extra, sub in (([], "plain"), (["--gsi"], "gsi"), (["--aflink", "random:aflink:0:1.5", "--gsi"], "both"), (["--aflink", "random:aflink:0:1.5"], "linked")):
        BaseTrack._count = 0
        folder = track.cli(common + extra + ["--results_root", str(tmp_path / sub)])
        files.append(os.path.join(folder, "synthetic-000.txt"))
    plain, smoothed, both, linked = (_rows_of(f) for f in files)
    keys = lambda r: set(zip(r[:, 0].astype(int).tolist(), r[:, 1].astype(int).tolist()))
    assert len(plain) > 0 and keys(plain) < keys(smoothed)                   # rows on frames where the tracker had a miss, none lost
    assert len(keys(smoothed)) == len(smoothed) and len(keys(both)) == len(both)      # no (frame, id) twice
    model = DeviceGSI(64, 4096, 64)
    want = GSI(model).apply(plain)
    assert np.array_equal(smoothed[:, :2], want[:, :2]) and np.abs(smoothed[:, 2:6] - want[:, 2:6]).max() <= 0.0051      # (written as %.2f)
    want = GSI(model).apply(linked)                                          # both in StrongSORT++'s order: GSI of the linked rows
    assert np.array_equal(both[:, :2], want[:, :2]) and np.abs(both[:, 2:6] - want[:, 2:6]).max() <= 0.0051
    assert all(line.endswith(",-1,-1,-1") for line in open(files[1]).read().splitlines())


def test_gsi_module_cli_smooths_a_file_written_earlier(tmp_path):
    from yolov7_tracker_amd.tracker import gsi
    s = sc.goldens()["t6p5"]
    src, dst = tmp_path / "results.txt", tmp_path / "smoothed.txt"
    with open(src, "w") as f:
        for r in s["rows_in"]:
            f.write("%d,%d,%.2f,%.2f,%.2f,%.2f,%d.0,-1,-1,-1\n" % (int(r[0]), int(r[1]), r[2], r[3], r[4], r[5], int(r[6])))
    gsi.main(["--input", str(src), "--output", str(dst), "--tau", "6.5"])
    got = np.array([[float(v) for v in line.split(",")[:7]] for line in open(dst).read().splitlines()])
    want = s["rows_out"]
    assert got.shape == want.shape and np.array_equal(got[:, :2], want[:, :2]) and np.array_equal(got[:, 6], want[:, 6]) and np.abs(got[:, 2:6] - want[:, 2:6]).max() < 0.02
