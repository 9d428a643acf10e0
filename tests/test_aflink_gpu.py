"""GPU: AFLink on the device (csrc/y7t_aflink.hip; DESIGN.md section 4 "AFLink").

The network: every score within 4 E of the reference module's recorded float64 score, E being the reference's own float32-versus-float64 gap over the recorded
set (the rule tests/test_deepmot_gpu.py applies to the DHN; the margin of 4 allows for a different summation order) -- at batch sizes around a wave, a workgroup of
the head and a chunk of pairs; bit-identical from call to call.  The candidate stage: pair list and count equal to the recorded ones, transformed blocks bit-equal
to the NumPy restatement (tests/aflink_np.py).  AFLink.link returns the recorded rows exactly.  The CLI plumbing."""
import os

import numpy as np
import pytest

from tests import aflink_np, aflink_scenes as sc

pytestmark = pytest.mark.gpu

HEAD_PAIRS = 8      # Y7T_AFL_HEAD_PAIRS: pairs per workgroup of the pooling + classifier kernel
CHUNK = 2048        # Y7T_AFL_CHUNK: pairs per chunk (the network runs layer by layer over a chunk)
SIZES = [1, 2, 63, 64, 65, 257, HEAD_PAIRS + 1, CHUNK + 1]


@pytest.fixture(scope="module")
def model():
    from yolov7_tracker_amd.tracker.aflink import DeviceAFLink
    return DeviceAFLink(sc.weights(), max_tracklets=256, max_rows=1 << 16, max_pairs=4096)


def _pool(P, shift=0):
    g = sc.pairs_golden()
    idx = (np.arange(P) * 7 + shift) % len(g["x1"])      # (every recorded pair once P >= 256; a different order than the fixture's)
    return g["x1"][idx], g["x2"][idx], g["scores64"][idx]


def test_constants_are_the_headers():
    from tests._hostsim import aflink as hs
    assert hs.constants() == dict(chunk=CHUNK, head_pairs=HEAD_PAIRS)


@pytest.mark.parametrize("P", SIZES)
def test_score_pairs_within_4E_of_the_float64_reference(model, P):
    g = sc.pairs_golden()
    x1, x2, want = _pool(P)
    got = model.score_pairs(x1, x2).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (P,)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("P = %d: max |device - float64| = %.3g   e_ref = %.3g   bound 4 E = %.3g" % (P, err, float(g["e_ref"]), 4 * float(g["E"])))
    assert err <= 4 * float(g["E"])


def test_score_pairs_with_a_chunk_smaller_than_the_batch():
    """an object sized for 5 pairs scores 13 in chunks of 5: the same bits as the large object's"""
    from yolov7_tracker_amd.tracker.aflink import DeviceAFLink
    g = sc.pairs_golden()
    small = DeviceAFLink(sc.weights(), max_tracklets=4, max_rows=16, max_pairs=5)
    x1, x2, want = _pool(13, 3)
    got = small.score_pairs(x1, x2).cpu().numpy()
    assert np.abs(got.astype(np.float64) - want).max() <= 4 * float(g["E"])


def test_scores_are_bit_identical_from_call_to_call(model):
    x1, x2, _ = _pool(CHUNK + 1)
    a = model.score_pairs(x1, x2).cpu().numpy()
    y1, y2, _ = _pool(65, 11)
    model.score_pairs(y2, y1)      # other data in between
    b = model.score_pairs(x1, x2).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and a pair's score does not depend on its place in the batch
    c = model.score_pairs(x1[::-1].copy(), x2[::-1].copy()).cpu().numpy()[::-1]
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


def _scene_table(s):
    rows = s["rows_in"][np.argsort(s["rows_in"][:, 0], kind="stable")]
    return aflink_np.tracklets(rows)


@pytest.mark.parametrize("name", sorted(sc.link_goldens()) or ["<no aflink_link_*.npz fixture>"])
def test_candidates_on_the_recorded_scenes(model, name):
    s = sc.link_goldens()[name]
    _, table, offsets = _scene_table(s)
    got = model.candidates(table, offsets, tuple(s["thrT"]), float(s["thrS"]), blocks=True)
    assert got["count"] == len(s["pairs"]) and got["status"] == 0 and np.array_equal(got["pairs"], s["pairs"])
    _, x1, x2 = aflink_np.candidates(table, offsets, tuple(s["thrT"]), float(s["thrS"]))
    assert np.array_equal(got["x1"].view(np.uint32), x1.view(np.uint32)) and np.array_equal(got["x2"].view(np.uint32), x2.view(np.uint32))
    if len(s["pairs"]):
        err = float(np.abs(got["scores"].astype(np.float64) - s["scores64"]).max())
        print("%s: %d candidates, max |device - float64| = %.3g   bound 4 E = %.3g" % (name, len(s["pairs"]), err, 4 * float(s["E"])))
        assert err <= 4 * float(s["E"])


@pytest.mark.parametrize("name", ["n1", "n2", "n65", "lengths", "constant_column", "single_rows", "distance_edge", "dense"])
def test_candidates_on_the_edge_geometries(model, name):
    """pair list and blocks equal to the restatement; the scores of the call (the count stays on the device) are the bits y7t_aflink_score_pairs_f32 gives for
    the same blocks, and on the small tables within 4 E of the float64 walk of the packed weights"""
    table, offsets = sc.geometry_tables()[name]
    pairs, x1, x2 = aflink_np.candidates(table, offsets)
    got = model.candidates(table, offsets, blocks=True)
    assert got["count"] == len(pairs) and got["status"] == 0 and np.array_equal(got["pairs"], pairs)
    assert np.array_equal(got["x1"].view(np.uint32), x1.view(np.uint32)) and np.array_equal(got["x2"].view(np.uint32), x2.view(np.uint32))
    if len(pairs):
        again = model.score_pairs(x1, x2).cpu().numpy()
        assert np.array_equal(got["scores"].view(np.uint32), again.view(np.uint32))
    if 0 < len(pairs) <= 32:
        E = float(sc.pairs_golden()["E"])
        assert np.abs(got["scores"].astype(np.float64) - aflink_np.forward_packed(sc.packed(), x1, x2)).max() <= 4 * E


def test_overflow_is_reported_and_link_raises():
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker.aflink import AFLink, DeviceAFLink
    table, offsets = sc.geometry_tables()["n65"]
    pairs = aflink_np.candidates(table, offsets)[0]
    tight = DeviceAFLink(sc.weights(), max_tracklets=65, max_rows=len(table), max_pairs=len(pairs) - 1)
    got = tight.candidates(table, offsets)
    assert got["count"] == len(pairs) and got["status"] & 1 and np.array_equal(got["pairs"], pairs[:-1])
    exact = DeviceAFLink(sc.weights(), max_tracklets=65, max_rows=len(table), max_pairs=len(pairs))
    assert exact.candidates(table, offsets)["status"] == 0
    rows = np.zeros((len(table), 6))
    rows[:, 0], rows[:, 2:4] = table[:, 0], table[:, 1:3]
    rows[:, 1] = np.repeat(np.arange(65) + 1, np.diff(offsets))
    with pytest.raises(_lib.Y7TError):
        AFLink(tight).link(rows)
    with pytest.raises(_lib.Y7TError):
        tight.candidates(np.zeros((66, 3)), np.arange(67))      # more tracklets than the object was sized for


@pytest.mark.parametrize("name", sorted(sc.link_goldens()) or ["<no aflink_link_*.npz fixture>"])
def test_link_returns_the_recorded_rows(model, name):
    from yolov7_tracker_amd.tracker.aflink import AFLink
    s = sc.link_goldens()[name]
    out = AFLink(model, tuple(s["thrT"]), float(s["thrS"]), float(s["thrP"])).link(s["rows_in"])
    assert out.shape == s["rows_out"].shape and np.array_equal(out, s["rows_out"])


def test_bad_arguments_are_refused_with_the_documented_codes(model):
    import torch
    from yolov7_tracker_amd import _lib
    L = _lib.load()
    E_ARG, E_CAPACITY, E_STATE = -1, -3, -4
    assert L.y7t_aflink_num_weights() == aflink_np.N_WEIGHTS
    for caps in ((0, 1, 1), (32769, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, (1 << 24) + 1)):
        assert L.y7t_aflink_workspace_bytes(*caps) == 0
    nbytes = int(L.y7t_aflink_weight_bytes()) + int(L.y7t_aflink_workspace_bytes(4, 16, 4))
    blob = torch.zeros(nbytes + 512, dtype=torch.uint8, device="cuda")
    base = blob.data_ptr() + (-blob.data_ptr()) % 256
    w = sc.packed()
    st = _lib.stream_ptr()
    assert L.y7t_aflink_init(base + 16, nbytes, w.ctypes.data, 4, 16, 4, st) == E_ARG          # misaligned
    assert L.y7t_aflink_init(base, nbytes - 1, w.ctypes.data, 4, 16, 4, st) == E_ARG           # too small
    assert L.y7t_aflink_init(base, nbytes, None, 4, 16, 4, st) == E_ARG
    assert L.y7t_aflink_init(base, nbytes, w.ctypes.data, 0, 16, 4, st) == E_ARG
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    x = torch.zeros((2, 30, 3), dtype=torch.float32, device="cuda")
    assert L.y7t_aflink_score_pairs_f32(base, x.data_ptr(), x.data_ptr(), 2, out.data_ptr(), st) == E_STATE      # never initialised
    assert L.y7t_aflink_init(base, nbytes, w.ctypes.data, 4, 16, 4, st) == 0
    assert L.y7t_aflink_score_pairs_f32(base, None, x.data_ptr(), 2, out.data_ptr(), st) == E_ARG
    assert L.y7t_aflink_score_pairs_f32(base, x.data_ptr(), x.data_ptr(), -1, out.data_ptr(), st) == E_ARG
    assert L.y7t_aflink_score_pairs_f32(base, x.data_ptr(), x.data_ptr(), 0, out.data_ptr(), st) == 0
    rows = torch.zeros((8, 3), dtype=torch.float64, device="cuda")
    off = torch.arange(9, dtype=torch.int32, device="cuda")
    pairs = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    head = torch.zeros(2, dtype=torch.int32, device="cuda")
    args = (pairs.data_ptr(), None, None, out.data_ptr(), head.data_ptr(), head.data_ptr() + 4, st)
    assert L.y7t_aflink_candidates(base, rows.data_ptr(), off.data_ptr(), 5, 0.0, 30.0, 75.0, *args) == E_CAPACITY
    assert L.y7t_aflink_candidates(base, rows.data_ptr(), None, 4, 0.0, 30.0, 75.0, *args) == E_ARG
    assert L.y7t_aflink_candidates(base, rows.data_ptr(), off.data_ptr(), -1, 0.0, 30.0, 75.0, *args) == E_ARG
    assert L.y7t_aflink_candidates(base, rows.data_ptr(), off.data_ptr(), 0, 0.0, 30.0, 75.0, *args) == 0
    torch.cuda.synchronize()
    assert head.cpu().tolist() == [0, 0]
    assert L.y7t_aflink_release(base) == 0
    assert L.y7t_aflink_score_pairs_f32(base, x.data_ptr(), x.data_ptr(), 2, out.data_ptr(), st) == E_STATE
    torch.cuda.synchronize()


def _rows_of(path):
    return np.array([[float(v) for v in line.split(",")[:6]] for line in open(path).read().splitlines()], np.float64).reshape(-1, 6)


def test_track_cli_links_the_rows_it_would_have_written(tmp_path, model):
    """plumbing only: a short ByteTrack run over scene detections with many misses, without and with --aflink; the linked file is AFLink.link of the first file's
    rows, and the unflagged file is what the CLI wrote before the flag existed (the ids of the NumPy oracle)"""
    from oracle import tracker_np
    from yolov7_tracker_amd import synth
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.aflink import AFLink, DeviceAFLink
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    g = sc.pairs_golden()
    spec = "random:aflink:%d:%g" % (int(g["seed"]), float(g["gain"]))
    common = ["--dataset", "synthetic", "--tracker", "bytetrack", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "320", "--synthetic_dets",
              "--synthetic_frames", "40", "--synthetic_objs", "12", "--synthetic_miss", "0.5", "--track_buffer", "3"]
    files = []
    for extra, sub in (([], "plain"), (["--aflink", spec], "linked")):
        BaseTrack._count = 0
        folder = track.cli(common + extra + ["--results_root", str(tmp_path / sub)])
        files.append(os.path.join(folder, "synthetic-000.txt"))
    plain, linked = _rows_of(files[0]), _rows_of(files[1])
    want = AFLink(DeviceAFLink(sc.weights(), 256, 1 << 16, 1 << 16)).link(plain)
    assert len(plain) > 0 and np.array_equal(linked, want[:, :6])
    assert all(line.endswith(",1.0,-1,-1,-1") for line in open(files[1]).read().splitlines())
    # the unflagged run: the oracle's ids, frame by frame
    dets = synth.make_detections(40, 12, 320, 0, miss=0.5)
    ref = tracker_np.run("bytetrack", dets, track_buffer=3)
    ids = [(f + 1, tid) for f, rows in enumerate(ref) for tid, tlwh, cls, score in rows if tlwh[2] * tlwh[3] > 150]
    assert [(int(r[0]), int(r[1])) for r in plain] == ids


def test_aflink_module_cli_links_a_file_written_earlier(tmp_path, model):
    from yolov7_tracker_amd.tracker import aflink
    s = sc.link_goldens()[sorted(k for k, v in sc.link_goldens().items() if bool(v["flag_accepted"]))[0]]
    src, dst = tmp_path / "results.txt", tmp_path / "linked.txt"
    with open(src, "w") as f:
        for r in s["rows_in"]:
            f.write("%d,%d,%.2f,%.2f,%.2f,%.2f,1.0,-1,-1,-1\n" % (int(r[0]), int(r[1]), r[2], r[3], r[4], r[5]))
    aflink.main(["--input", str(src), "--output", str(dst), "--aflink", "random:aflink:%d:%g" % (int(s["seed"]), float(s["gain"]))])
    assert np.array_equal(_rows_of(dst), s["rows_out"]) and open(dst).read().splitlines()[0].endswith(",1.0,-1,-1,-1")
