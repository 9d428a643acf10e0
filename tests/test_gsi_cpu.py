"""CPU: GSI without a GPU (DESIGN.md section 4 "GSI").  The host build of csrc/y7t_gsi.h (tests/_hostsim/gsi.py: the interpolation and the per-track smoother the
device's workgroups run, the matrix instruction replaced by the same sums in the same order) against the recorded fixtures: interpolated rows ARRAY-EQUAL to the
NumPy restatement (tests/gsi_np.py) and to the recording; every smoothed value within 4 E of the 50-digit solution, E being the NumPy float64 restatement's own
largest distance to it over the recorded set (the rule of tests/test_aflink_gpu.py and tests/test_deepmot_gpu.py: the margin of 4 allows for another summation
order and a one-ulp exp; two float64 orders tried when the bound was chosen differed by at most 1.8 times their own distance to the exact solution).  Then
tracker/gsi.py's host side on the host build, the module CLI's file round trip and track.py's flags.

Measured when written (4 E = 1.78e-4 px): host build 2.9e-5, NumPy against scikit-learn 6.8e-5 (profiles/gsi_margins.txt)."""
import numpy as np
import pytest

from tests import gsi_np, gsi_scenes as sc

NAMES = sorted(sc.SCENES)


def test_fixture_set_holds_the_required_cases():
    g = sc.goldens()
    assert sorted(g) == NAMES and len({float(s["E"]) for s in g.values()}) == 1 and 0 < sc.bound()[0] < 1e-3
    lengths = np.concatenate([np.diff(s["offsets"]) for s in g.values()]).tolist()
    for want in (1, 2, 15, 16, 17, 31, 33, 64, 65, 128, 129, 131, 300):
        assert want in lengths
    assert max(lengths) <= 300
    steps = set()
    for s in g.values():
        for k in range(len(s["ids"])):
            steps |= set(np.diff(s["runs_in"][s["offsets_in"][k]:s["offsets_in"][k + 1], 0]).astype(int).tolist())
        assert len(np.unique(s["rows_in"][:, :2], axis=0)) == len(s["rows_in"]) - 1      # one duplicated (frame, id)
        assert np.any(np.diff(s["rows_in"][:, 0]) < 0) and np.any(np.diff(s["ids"]) > 1)       # shuffled; non-contiguous ids
    assert {1, 2, 19, 20, 21} <= steps
    t10, t6, t2 = g["t10"], g["t6p5"], g["t2"]
    assert np.diff(t10["runs"][t10["offsets"][11]:t10["offsets"][12], 0]).max() == 21          # open gaps: the frames are not equally spaced
    assert t6["len_scale"][0] == 1 / 6.5 and np.diff(t6["offsets"])[0] == 300                   # the 1 / tau clip
    assert t2["len_scale"][0] == 4.0 and t2["len_scale"][2] == 0.5 and 0.5 < t2["len_scale"][1] < 4.0      # the tau**2 clip
    # smoothing moves values by pixels: a smoother that returns its input fails the 4 E test
    assert np.abs(t10["exact"] - t10["runs"][:, 1:]).max() > 1.0
    for s in g.values():
        assert np.array_equal(s["len_scale"], gsi_np.len_scale(np.diff(s["offsets"]), float(s["tau"])))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_recording(name):
    s = sc.goldens()[name]
    rows_in, tau = sc.scene_rows(name)
    assert np.array_equal(rows_in, s["rows_in"]) and tau == float(s["tau"])
    rows, ids, off = gsi_np.order(rows_in)
    assert np.array_equal(ids, s["ids"]) and np.array_equal(off, s["offsets_in"]) and np.array_equal(rows[:, [0, 2, 3, 4, 5]], s["runs_in"])
    runs, off2, src = gsi_np.interpolate(s["runs_in"], off, int(s["interval"]))
    assert np.array_equal(runs, s["runs"]) and np.array_equal(off2, s["offsets"]) and np.array_equal(src, s["src"])


@pytest.mark.parametrize("name", NAMES)
def test_host_build_interpolation_is_array_equal(name):
    from tests._hostsim import gsi as hs
    s = sc.goldens()[name]
    got = hs.interpolate(s["runs_in"], s["offsets_in"], int(s["interval"]), max_rows=len(s["runs"]), max_len=300)
    assert got["count"] == len(s["runs"]) and got["status"] == 0
    assert np.array_equal(got["runs"].view(np.uint64), s["runs"].view(np.uint64))
    assert np.array_equal(got["offsets"], s["offsets"]) and np.array_equal(got["src"], s["src"])


def test_host_build_interpolation_reports_overflow():
    from tests._hostsim import gsi as hs
    s = sc.goldens()["t10"]
    got = hs.interpolate(s["runs_in"], s["offsets_in"], 20, max_rows=len(s["runs"]) - 1, max_len=299)
    assert got["status"] == 3 and got["count"] == len(s["runs"]) and np.array_equal(got["runs"], s["runs"][:-1])


@pytest.mark.parametrize("name", NAMES)
def test_host_build_smoother_within_4E_of_the_exact_solution(name):
    from tests._hostsim import gsi as hs
    s = sc.goldens()[name]
    E, bound = sc.bound()
    got, status = hs.smooth(s["runs"], s["offsets"], s["len_scale"])
    assert not status.any()
    errs = [float(np.abs(got[lo:hi] - s["exact"][lo:hi]).max()) for lo, hi in zip(s["offsets"][:-1], s["offsets"][1:])]
    print("%s: host build max |smoothed - exact| = %.3g   E = %.3g   bound 4 E = %.3g   per track %s" % (name, max(errs), E, bound, " ".join("%.2g" % e for e in errs)))
    assert max(errs) <= bound


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_the_release_regressor(name):
    s = sc.goldens()[name]
    E, bound = sc.bound()
    got = gsi_np.smooth(s["runs"], s["offsets"], float(s["tau"]))
    err_sk, err_rec = float(np.abs(got - s["cols_sk"]).max()), float(np.abs(got - s["cols_np"]).max())
    print("%s: NumPy restatement against scikit-learn's prediction %.3g, against its own recording %.3g   bound 4 E = %.3g" % (name, err_sk, err_rec, bound))
    assert err_sk <= bound and err_rec <= bound


def test_host_build_flags_a_non_positive_pivot_and_leaves_the_track():
    """two equal frames survive only because the regularisation is switched off: the second pivot is exactly zero"""
    from tests._hostsim import gsi as hs
    runs = np.array([[5, 1, 2, 3, 4], [5, 9, 8, 7, 6], [1, 10, 20, 30, 40], [2, 11, 21, 31, 41], [3, 12, 22, 32, 42]], np.float64)
    got, status = hs.smooth(runs, [0, 2, 5], [3.0, 3.0], reg=0.0)
    assert status.tolist() == [1, 0] and np.array_equal(got[:2], runs[:2, 1:]) and np.isfinite(got).all()
    assert np.abs(got[2:] - gsi_np.smooth_track(runs[2:, 0], runs[2:, 1:], 3.0, 0.0)).max() < 1e-9


def _host_gsi(**kw):
    from tests._hostsim.gsi import HostGSI
    from yolov7_tracker_amd.tracker.gsi import GSI
    return GSI(HostGSI(**kw.pop("caps", {})), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_apply_on_the_host_build_orders_rows_and_carries_tails(name):
    s = sc.goldens()[name]
    E, bound = sc.bound()
    out = _host_gsi(interval=int(s["interval"]), tau=float(s["tau"])).apply(s["rows_in"])
    want = s["rows_out"]
    assert out.shape == want.shape and np.array_equal(out[:, :2], want[:, :2]) and np.array_equal(out[:, 6:], want[:, 6:])
    assert np.array_equal(np.lexsort((out[:, 1], out[:, 0])), np.arange(len(out))) and len(np.unique(out[:, :2], axis=0)) == len(out)
    assert np.abs(out[:, 2:6] - want[:, 2:6]).max() <= 2 * bound      # (both sides lie within 4 E of the exact columns)
    assert not np.any(out[:, 6] == 9.0)                               # the duplicate behind its original was dropped
    # a new row carries the class of the row at the start of its gap
    rows, _, _ = gsi_np.order(s["rows_in"])
    key = {(r[0], r[1]): r[6] for r in rows}
    new = [r for r in out if (r[0], r[1]) not in key]
    assert len(new) == len(out) - len(rows) and len(new) > 0 or name == "t2"
    for r in new[:50]:
        f0 = max(f for (f, i) in key if i == r[1] and f < r[0])
        assert r[6] == key[(f0, r[1])]


def test_apply_refuses_a_track_longer_than_max_len_with_its_id():
    from yolov7_tracker_amd import _lib
    s = sc.goldens()["t10"]
    with pytest.raises(_lib.Y7TError, match=r"track id 87 has 300 rows"):
        _host_gsi(caps=dict(max_len=299)).apply(s["rows_in"])
    with pytest.raises(_lib.Y7TError, match=r"max_rows"):
        _host_gsi(caps=dict(max_rows=len(s["runs"]) - 1)).apply(s["rows_in"])


def test_apply_on_an_empty_table_and_on_one_row():
    g = _host_gsi()
    assert g.apply(np.zeros((0, 7))).shape == (0, 7)
    one = np.array([[4.0, 2.0, 10.0, 20.0, 30.0, 40.0, 1.0]])
    out = g.apply(one)
    assert out.shape == (1, 7) and np.array_equal(out[:, [0, 1, 6]], one[:, [0, 1, 6]]) and np.abs(out[:, 2:6] - one[:, 2:6]).max() < 1e-7
    with pytest.raises(ValueError):
        g.apply(np.zeros((3, 5)))


def test_module_cli_round_trip_on_the_host_build(tmp_path, capsys):
    from tests._hostsim.gsi import HostGSI
    from yolov7_tracker_amd.tracker import gsi
    s = sc.goldens()["t6p5"]
    src, dst = tmp_path / "results.txt", tmp_path / "smoothed.txt"
    with open(src, "w") as f:
        for r in s["rows_in"]:
            f.write("%d,%d,%.2f,%.2f,%.2f,%.2f,%d.0,-1,-1,-1\n" % (int(r[0]), int(r[1]), r[2], r[3], r[4], r[5], int(r[6])))
    gsi.main(["--input", str(src), "--output", str(dst), "--tau", "6.5"], model=HostGSI())
    lines = open(dst).read().splitlines()
    got = np.array([[float(v) for v in line.split(",")[:7]] for line in lines])
    want = s["rows_out"]
    assert got.shape == want.shape and np.array_equal(got[:, :2], want[:, :2]) and np.array_equal(got[:, 6], want[:, 6])
    assert np.abs(got[:, 2:6] - want[:, 2:6]).max() < 0.02 and all(line.endswith(".0,-1,-1,-1") for line in lines)      # (%.2f in, %.2f out)


def test_track_cli_takes_the_gsi_flags_and_is_off_by_default():
    from yolov7_tracker_amd.tracker import track
    p = track.build_parser()
    o = p.parse_args([])
    assert o.gsi is False and o.gsi_interval == 20 and o.gsi_tau == 10
    o = p.parse_args(["--gsi", "--gsi_interval", "12", "--gsi_tau", "8.5"])
    assert o.gsi is True and o.gsi_interval == 12 and o.gsi_tau == 8.5
    assert "not filtered by --min_area" in " ".join([a.help for a in p._actions if "--gsi" in a.option_strings][0].split())


def test_smooth_results_keeps_track_py_results_without_rows_and_their_form():
    from tests._hostsim.gsi import HostGSI
    from yolov7_tracker_amd.tracker import gsi
    assert gsi.smooth_results([(1, [], [], []), (2, [], [], [])]) == [(1, [], [], []), (2, [], [], [])]
    res = [(1, [7], [np.array([1.0, 2.0, 3.0, 4.0])], [0.0]), (2, [], [], []), (4, [7, 9], [np.array([4.0, 5.0, 3.0, 4.0]), np.array([50.0, 50.0, 5.0, 5.0])], [0.0, 2.0])]
    out = gsi.smooth_results(res, model=HostGSI())
    assert [(f, ids) for f, ids, _, _ in out] == [(1, [7]), (2, [7]), (3, [7]), (4, [7, 9])] and [c for _, _, _, c in out] == [[0.0], [0.0], [0.0], [0.0, 2.0]]
    from yolov7_tracker_amd.tracker.aflink import results_rows
    assert np.abs(results_rows(out)[:, 2:6] - gsi_np.apply(results_rows(res))[:, 2:6]).max() < 0.011      # (results_rows reads the boxes back as their %.2f text)
