"""GPU: the baseline JPEG decoder kernels (csrc/y7t_jpegdec.hip) against the NumPy restatement (tests/jpegdec_np.py; tests/test_jpegdec_cpu.py holds it to Pillow and
the host build of the same header to it) byte for byte: every size x sampling of the matrix with the files of a geometry as one batch, at the default and the smallest
subsequence length; a stream of several runs and one that synchronises as slowly as a stream can; repeatability and independence of the batch; this project's own
encoder's device output decoded again; the C ABI's refusals.  Only well-formed files reach the device."""
import ctypes

import numpy as np
import pytest

from tests import jpegdec_cases as cases

pytestmark = pytest.mark.gpu


def _decoder(data, max_batch, subseq_bytes=0, max_file_bytes=None):
    from yolov7_tracker_amd.tracker import jpeg_decode
    info = jpeg_decode.parse(data)
    return jpeg_decode.DeviceJpegDecoder(info.H, info.W, info.components, info.sampling, max_batch=max_batch, max_file_bytes=max_file_bytes or 4 * len(data) + 4096,
                                         subseq_bytes=subseq_bytes)


@pytest.mark.parametrize("sampling", cases.SAMPLINGS)
def test_device_equals_the_restatement_on_the_matrix(sampling):
    from yolov7_tracker_amd.tracker import jpeg_decode
    for size in cases.SIZES:
        files = [d for _, d in cases.matrix()[(size, sampling)]]
        want = np.stack([cases.reference(d)[2] for d in files])
        for subseq_bytes in (0, jpeg_decode.SUBSEQ_MIN):
            dec = _decoder(files[0], len(files), subseq_bytes, max_file_bytes=max(len(d) for d in files))
            frames, status = dec.decode(files)
            assert not status.cpu().numpy().any(), (size, subseq_bytes, status.cpu().tolist())
            got = frames.cpu().numpy()
            assert np.array_equal(got, want), (size, subseq_bytes, [n for (n, _), g, w in zip(cases.matrix()[(size, sampling)], got, want) if not np.array_equal(g, w)])


@pytest.mark.parametrize("which", ["multi_run", "slow"])
def test_streams_that_need_rounds(which):
    """160 x 160 noise at quality 100 (several runs: launches after the first find work) and the stream no lane of which is right before its predecessor is"""
    from yolov7_tracker_amd.tracker import jpeg_decode
    data = cases.multi_run_stream() if which == "multi_run" else cases.slow_stream()
    want = cases.reference(data)[2]
    for subseq_bytes in (0, jpeg_decode.SUBSEQ_MIN):
        dec = _decoder(data, 1, subseq_bytes)
        frames, status = dec.decode([data])
        assert int(status[0]) == 0 and np.array_equal(frames[0].cpu().numpy(), want), subseq_bytes
        S = subseq_bytes or jpeg_decode.SUBSEQ_DEFAULT
        info = jpeg_decode.parse(data)
        launches = max(1, -(-(-(-int(info.desc["scan_len"]) // S)) // 256))
        rounds = int(dec.rounds(1)[0])
        assert 1 <= rounds <= launches, (rounds, launches)      # launch r settles run r
        if which == "multi_run":
            assert launches >= 3 and rounds >= 2


def test_two_calls_and_any_batch_give_the_same_bytes():
    """a file's frame alone, inside a batch of eight different files at either end, and from a second call"""
    files = [d for _, d in cases.matrix()[((37, 53), "420")]][:8]
    assert len(set(files)) == 8
    dec = _decoder(files[0], 8, max_file_bytes=max(len(d) for d in files))
    first, st = dec.decode(files)
    again, _ = dec.decode(files)
    assert not st.cpu().numpy().any() and np.array_equal(first.cpu().numpy(), again.cpu().numpy())
    rev, _ = dec.decode(files[::-1])
    assert np.array_equal(rev.cpu().numpy()[::-1], first.cpu().numpy())
    for b in (0, 5, 7):
        alone, _ = dec.decode([files[b]])
        assert np.array_equal(alone[0].cpu().numpy(), first[b].cpu().numpy()) and np.array_equal(alone[0].cpu().numpy(), cases.reference(files[b])[2])
    parts = _decoder(files[0], 3, max_file_bytes=max(len(d) for d in files)).decode(files)[0]      # a list longer than max_batch goes in parts
    assert np.array_equal(parts.cpu().numpy(), first.cpu().numpy())


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("shape", [(37, 53), (64, 48)])
def test_our_encoders_device_output_decodes_to_the_restatement(sub, shape):
    from tests import jpegdec_np
    from yolov7_tracker_amd.tracker.render import DeviceRenderer
    frames = np.stack([cases.frame(shape[0], shape[1], kind, seed=5)[..., ::-1] for kind in ("ramp", "noise")])
    files = DeviceRenderer(shape[0], shape[1], quality=90, subsampling=sub, max_batch=2).encode(frames)
    got, status = _decoder(files[0], 2, max_file_bytes=max(len(f) for f in files)).decode(files)
    assert not status.cpu().numpy().any()
    for g, f in zip(got.cpu().numpy(), files):
        assert np.array_equal(g, jpegdec_np.decode(f))


def test_abi_refusals_launch_nothing():
    import torch
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker import jpeg_decode
    L = _lib.load()
    data = cases.matrix()[((17, 33), "420")][0][1]
    info = jpeg_decode.parse(data)
    dec = _decoder(data, 2, max_file_bytes=len(data) + 8)
    dev, descs = dec.upload([data, data])
    frames = torch.full((2 * 17 * 33 * 3 + 8,), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    P, S = _lib.ptr, _lib.stream_ptr
    dp = ctypes.c_void_p(descs.ctypes.data)
    call = lambda obj, files, d, B, fr, st: L.y7t_jpegdec_decode(obj, files, d, B, fr, st, S())      # noqa: E731
    E_ARG, E_CAPACITY, E_STATE = -1, -3, -4
    assert call(P(dec._obj), None, dp, 2, P(frames), P(status)) == E_ARG
    assert call(P(dec._obj), P(dev), None, 2, P(frames), P(status)) == E_ARG
    assert call(P(dec._obj), P(dev), dp, 2, None, P(status)) == E_ARG
    assert call(P(dec._obj), P(dev), dp, 2, P(frames), None) == E_ARG
    assert call(P(dec._obj), P(dev), dp, 2, ctypes.c_void_p(frames.data_ptr() + 1), P(status)) == E_ARG
    assert call(P(dec._obj), P(dev), dp, 2, P(frames), ctypes.c_void_p(status.data_ptr() + 2)) == E_ARG
    assert call(P(dec._obj), P(dev), dp, 3, P(frames), P(status)) == E_CAPACITY
    assert call(ctypes.c_void_p(dec._obj.data_ptr() + 256), P(dev), dp, 2, P(frames), P(status)) == E_STATE
    long_ = descs.copy()
    long_["file_len"][1] = len(data) + 9
    assert call(P(dec._obj), P(dev), ctypes.c_void_p(long_.ctypes.data), 2, P(frames), P(status)) == E_CAPACITY
    outside = descs.copy()
    outside["scan_len"][0] = len(data)
    assert call(P(dec._obj), P(dev), ctypes.c_void_p(outside.ctypes.data), 2, P(frames), P(status)) == E_ARG
    assert L.y7t_jpegdec_bytes(17, 33, 3, 2, 2, 1000, 12) == 0 and L.y7t_jpegdec_bytes(17, 33, 1, 2, 2, 1000, 0) == 0 and L.y7t_jpegdec_bytes(17, 33, 3, 2, 0, 1000, 0) == 0
    assert L.y7t_jpegdec_bytes(17, 33, 3, 2, 2, 1000, jpeg_decode.SUBSEQ_MIN) > 0 and L.y7t_jpegdec_bytes(17, 33, 3, 2, 2, 1000, jpeg_decode.SUBSEQ_MIN - 4) == 0
    assert L.y7t_jpegdec_init(ctypes.c_void_p(dec._obj.data_ptr() + 1), 1 << 30, 17, 33, 3, 2, 2, 1000, 0, S()) == E_ARG
    torch.cuda.synchronize()
    assert (frames == 7).all() and (status == 9).all(), "a refused call wrote something"
    assert call(P(dec._obj), P(dev), dp, 2, P(frames), P(status)) == 0      # ... and the same arguments, sound, decode
    torch.cuda.synchronize()
    assert (status[:2] == 0).all() and np.array_equal(frames[:17 * 33 * 3].cpu().numpy().reshape(17, 33, 3), cases.reference(data)[2])
    assert (info.H, info.W) == (17, 33)
