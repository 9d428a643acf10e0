"""C-BIoU on the MI355X: the device frame step (csrc/y7t_track_cbiou.h) through every entry point -- C_BIoUTracker frame by frame, y7t_tracker_step_frames,
y7t_tracker_step_batch -- against the reference's golden vectors (tests/golden/tracker_c_biou_*.npz) and the CPU build of the same program; the tracker
CLI with --tracker c_biou."""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import _hostsim as hs  # noqa: E402
from tests import tracker_case as tc  # noqa: E402
from yolov7_tracker_amd.tracker.c_biou_tracker import C_BIoUTracker  # noqa: E402

NAMES = tc.NAMES["c_biou"]
load_golden = functools.partial(tc.load_golden, "c_biou")
new_tracker = functools.partial(tc.new_tracker, C_BIoUTracker)


@pytest.mark.parametrize("threads", [64, 256, 1024])
@pytest.mark.parametrize("name", NAMES)
def test_c_biou_tracker_matches_reference_golden(name, threads):
    g = load_golden(name)
    t = new_tracker(g["conf"], threads)
    for f, d in enumerate(g["dets"]):
        cur = t.update(d, None)
        check = f % 10 == 9 or f == len(g["dets"]) - 1
        tc.check_tracks(cur, g, f, True, ([x.track_id for x in t.tracked_stracks], [x.track_id for x in t.lost_stracks]) if check else None)


def test_c_biou_track_views():
    """the per-track attributes of the reference's C_BIoUSTrack on the views update() returns"""
    from yolov7_tracker_amd.tracker.basetrack import TrackState
    g = load_golden("misses")
    t = new_tracker()
    for d in g["dets"][:40]:
        cur = t.update(d, None)
    tr = cur[0]
    buf = tr.origin_bbox_buffer
    assert 1 <= len(buf) <= 6 and buf[-1].dtype == np.float32 and np.array_equal(buf[-1], tr.tlwh)
    assert tr.state == TrackState.Tracked and tr.is_activated and tr.frame_id == 40 and tr.end_frame == 40
    assert np.array_equal(tr.tlbr, np.concatenate([tr.tlwh[:2], tr.tlwh[2:] + tr.tlwh[:2]]))
    for a in ("motion_state1", "motion_state2", "buffer_bbox1", "buffer_bbox2"):
        v = getattr(tr, a)
        assert v.shape == (4,) and v.dtype == np.float32 and (v >= 0).all()
    assert t.lost_stracks and all(x.state == TrackState.Lost for x in t.lost_stracks)
    assert max(x.time_since_update for x in t.lost_stracks) >= 1


def test_c_biou_update_without_detection():
    t = new_tracker()
    assert t.update_without_detection(None, None) == [] and t.frame_id == 1      # empty pool: the frame advances
    d = np.array([[10, 10, 60, 90, 0.9, 0], [200, 40, 260, 160, 0.8, 1]], np.float32)
    t.update(d, None)
    assert t.update_without_detection(None, None) == []      # only unconfirmed tracks: the pool is still empty
    t.update(d, None)
    with pytest.raises(NotImplementedError):
        t.update_without_detection(None, None)


def test_c_biou_step_frames_equals_frame_by_frame():
    """y7t_tracker_step_frames (the list arena in LDS) over groups of frames == the frame-by-frame step"""
    g = load_golden("misses")
    t = new_tracker()
    dd = [torch.from_numpy(d).cuda() for d in g["dets"]]
    outs = [torch.zeros((t.cap_t + 1, 8), dtype=torch.float64, device="cuda") for _ in dd]
    for f0 in range(0, len(dd), 16):
        t._launch_frames(t.frames_table(dd[f0:f0 + 16], outs[f0:f0 + 16]))
    torch.cuda.synchronize()
    assert t._status() == 0
    for f, o in enumerate(outs):
        h = o.cpu().numpy()
        rows = h[:int(h[t.cap_t].view(np.int32)[0])]
        ids, tlwh, _, score = g["frames"][f]
        assert rows[:, 0].astype(np.int64).tolist() == ids.tolist(), "frame %d" % f
        assert np.array_equal(rows[:, 1:5], tlwh) and np.array_equal(rows[:, 6].astype(np.float32), score)
    assert ([x.track_id for x in t.tracked_stracks], [x.track_id for x in t.lost_stracks]) == (g["tracked"][-1], g["lost"][-1])


def test_c_biou_batch_with_shared_id_counter_equals_single_runs():
    """y7t_tracker_step_batch over four C-BIoU pools with ONE id counter: every pool returns the rows of its single run (boxes, classes, scores, slots),
    each of its ids stands for one id of the single run, and no id is handed out twice"""
    from yolov7_tracker_amd import _lib, synth
    L = _lib.load()
    nseq, nfr, cap = 4, 30, 512
    seqs = [synth.make_detections(nfr, 30 + 20 * s, seq_idx=60 + s, miss=0.2) for s in range(nseq)]
    nbytes = int(L.y7t_tracker_state_bytes(cap, cap))

    def mk(ids):
        st = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nseq)]
        for s in range(nseq):
            _lib.check(L.y7t_tracker_init(_lib.ptr(st[s]), nbytes, hs.HostSimTracker.TRACKERS["c_biou"], 0, cap, cap, 0.2, 0.5, 30, 1, _lib.ptr(ids[s]), _lib.stream_ptr()))
        return st
    outs = torch.zeros((nseq, cap + 1, 8), dtype=torch.float64, device="cuda")
    own_ids = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(nseq)]      # one id counter per pool; the states keep their ADDRESSES: the tensors live as long as the states
    st = mk(own_ids)
    single = [[] for _ in range(nseq)]
    for f in range(nfr):
        for s in range(nseq):
            d = torch.from_numpy(seqs[s][f]).cuda()
            _lib.check(L.y7t_tracker_step(_lib.ptr(st[s]), _lib.ptr(d), d.shape[0], _lib.ptr(outs[s]), cap,
                                          ctypes.c_void_p(outs[s].data_ptr() + cap * 64), 0, None, _lib.stream_ptr()))
            torch.cuda.synchronize()
            h = outs[s].cpu().numpy()
            single[s].append(h[:int(h[cap].view(np.int32)[0])].copy())
    shared = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = mk([shared] * nseq)
    state_ptrs = torch.tensor([x.data_ptr() for x in st], dtype=torch.int64, device="cuda")
    out_ptrs = torch.tensor([outs[s].data_ptr() for s in range(nseq)], dtype=torch.int64, device="cuda")
    counts = torch.zeros(nseq, dtype=torch.int32, device="cuda")
    maps = [{} for _ in range(nseq)]
    for f in range(nfr):
        dd = [torch.from_numpy(seqs[s][f]).cuda() for s in range(nseq)]
        det_ptrs = torch.tensor([d.data_ptr() for d in dd], dtype=torch.int64, device="cuda")
        n_dev = torch.tensor([d.shape[0] for d in dd], dtype=torch.int32, device="cuda")
        _lib.check(L.y7t_tracker_step_batch(_lib.ptr(state_ptrs), _lib.ptr(det_ptrs), _lib.ptr(n_dev), _lib.ptr(out_ptrs), _lib.ptr(counts), cap,
                                            nseq, 0, None, _lib.stream_ptr()))
        torch.cuda.synchronize()
        c, h = counts.cpu().numpy(), outs.cpu().numpy()
        for s in range(nseq):
            got, want = h[s, :c[s]], single[s][f]
            assert c[s] == len(want)
            np.testing.assert_array_equal(got[:, 1:], want[:, 1:])
            for a, b in zip(want[:, 0].astype(int), got[:, 0].astype(int)):
                assert maps[s].setdefault(a, b) == b
    allid = [b for m in maps for b in m.values()]
    assert len(allid) == len(set(allid)) and int(shared.item()) >= max(allid)      # a single run's id is always the same batch id, no id twice


@pytest.mark.parametrize("seed", range(3))
def test_c_biou_device_equals_host_build_on_crowds(seed):
    from yolov7_tracker_amd import synth
    dets = synth.make_detections(15, 500, seq_idx=90 + seed, miss=0.15, bounce=True)
    host = hs.HostSimTracker("c_biou")
    t = new_tracker(threads=512)
    for f, d in enumerate(dets):
        want = host.update(d)
        cur = t.update(d, None)
        assert [x.track_id for x in cur] == [r[0] for r in want], "frame %d" % f
        assert np.array_equal(np.array([x.tlwh for x in cur], np.float64).reshape(-1, 4), np.array([r[1] for r in want]).reshape(-1, 4))


def test_c_biou_pool_overflow_raises():
    from yolov7_tracker_amd import _lib, synth
    t = new_tracker(max_tracks=24)
    with pytest.raises(_lib.Y7TError, match="overflow"):
        for d in synth.make_detections(5, 60, seq_idx=3):
            t.update(d, None)


def test_c_biou_pool_refused_by_deepsort_step():
    from yolov7_tracker_amd import _lib
    t = new_tracker()
    L = t._L
    fb = int(L.y7t_deepsort_feature_bytes(t.cap_t, t.cap_d, 128, 8))
    feat = torch.zeros(fb, dtype=torch.uint8, device="cuda")
    _lib.check(L.y7t_deepsort_init(_lib.ptr(feat), fb, t.cap_t, t.cap_d, 128, 8, _lib.stream_ptr()))
    d = torch.tensor([[10, 10, 60, 90, 0.9, 0]], dtype=torch.float32, device="cuda")
    f = torch.zeros((1, 128), dtype=torch.float32, device="cuda")
    r = L.y7t_tracker_step_deepsort(_lib.ptr(t._state), _lib.ptr(feat), t.cap_t, _lib.ptr(d), 1, _lib.ptr(f), _lib.ptr(t._out), t.cap_t, t._count_ptr, 0,
                                    _lib.stream_ptr())
    torch.cuda.synchronize()
    assert r != 0 and t._status() & 8      # Y7T_ERR_KIND


@pytest.mark.parametrize("batch", [1, 8])
def test_track_cli_c_biou_synthetic(tmp_path, batch):
    """tracker/track.py --dataset synthetic --tracker c_biou --synthetic_dets: the result file the 'default' golden implies"""
    from yolov7_tracker_amd.tracker import track
    from yolov7_tracker_amd.tracker.basetrack import BaseTrack
    BaseTrack._count = 0
    folder = track.cli(["--dataset", "synthetic", "--tracker", "c_biou", "--model_path", "random:yolov7-tiny", "--nc", "10", "--img_size", "1280",
                        "--synthetic_dets", "--synthetic_frames", "100", "--synthetic_objs", "80", "--results_root", str(tmp_path), "--batch", str(batch)])
    got = open(os.path.join(folder, "synthetic-000.txt")).read()
    g = load_golden("default")
    lines = []
    for f, (ids, tlwh, _, _) in enumerate(g["frames"]):
        for tid, b in zip(ids, tlwh):
            if np.float32(b[2]) * np.float32(b[3]) > 150:      # (the track's tlwh is float32, like the reference's C_BIoUSTrack.tlwh)
                lines.append(f'{f + 1},{tid},{b[0]:.2f},{b[1]:.2f},{b[2]:.2f},{b[3]:.2f},1.0,-1,-1,-1\n')
    assert got == "".join(lines)
