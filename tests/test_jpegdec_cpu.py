"""CPU: the baseline JPEG decoder's arithmetic (DESIGN.md section 4 "JPEG decoding") without a GPU.  The NumPy restatement (tests/jpegdec_np.py) against Pillow's
decode -- libjpeg-turbo with its defaults, what TrackerLoader returns today -- byte for byte; the host build of csrc/y7t_jpegdec.h (tests/_hostsim/jpegdec.py: the
device's functions and launches as loops) against the restatement at three stages; the synchronisation rounds against the bound DESIGN derives; the marker parser's
refusals; corrupt streams, on the host build only (under canaries, and in a stand-alone program built with the address and undefined-behaviour sanitizers); the
loader's device_decode hand-over."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import jpegdec_cases as cases
from tests import jpegdec_np
from tests._hostsim import jpegdec as hostsim
from yolov7_tracker_amd.tracker import jpeg_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


needs_turbo = pytest.mark.skipif(not _turbo(), reason="Pillow is not built on libjpeg-turbo here: its decode is not the yardstick the specification was checked against")


@needs_turbo
def test_restatement_equals_pillow_on_the_matrix():
    n = 0
    for key, files in cases.matrix().items():
        for name, data in files:
            assert np.array_equal(cases.reference(data)[2], cases.pillow_bgr(data)), (key, name)
            n += 1
    assert n == 7 * 4 * 24


def _own_streams():
    from tests import render_np
    out = []
    for i, (h, w) in enumerate([(1, 1), (2, 3), (7, 9), (8, 8), (15, 17), (16, 16), (17, 33), (31, 6), (37, 53), (48, 70)]):
        frame = cases.frame(h, w, "noise" if i % 2 else "ramp", seed=i)
        for sub in ("420", "444"):
            out.append(((h, w, sub), render_np.encode(frame, quality=90, subsampling=sub)))
    return out


@needs_turbo
def test_restatement_equals_pillow_on_our_encoders_streams():
    """the streams of this project's own encoder (tests/render_np.py::encode: Annex K tables, a restart interval of one MCU row), 4:2:0 and 4:4:4, ten sizes"""
    for key, data in _own_streams():
        assert np.array_equal(jpegdec_np.decode(data), cases.pillow_bgr(data)), key


def _check_stages(data, subseq_bytes, what, lanes=hostsim.LANES):
    info = jpeg_decode.parse(data)
    assert info is not None, what
    diffs, coefs, frame = cases.reference(data)
    r = hostsim.decode(data, info, subseq_bytes, lanes)
    assert r.rc == 0 and r.status == 0 and r.clean, (what, r.rc, r.status)
    assert np.array_equal(r.diffs, diffs), (what, "coefficients per block")
    assert np.array_equal(r.coefs, coefs), (what, "DC values after the scan")
    assert np.array_equal(r.frame, frame), (what, "frame")
    # a run of n lanes agrees with its entry after at most n + 1 rounds, and launch r settles run r: the launches made suffice
    assert 1 <= r.iters <= min(r.nsub, lanes) + 1 and 1 <= r.rounds <= r.launches == max(1, -(-r.nsub // lanes)), (what, r.iters, r.rounds, r.launches)
    return r


@pytest.mark.parametrize("subseq_bytes", [0, -1], ids=["default", "smallest"])
def test_host_build_equals_restatement_at_three_stages(subseq_bytes):
    subseq_bytes = jpeg_decode.SUBSEQ_DEFAULT if subseq_bytes == 0 else hostsim.subseq_min()
    assert hostsim.subseq_min() == jpeg_decode.SUBSEQ_MIN
    for key, files in cases.matrix().items():
        for name, data in files:
            _check_stages(data, subseq_bytes, (key, name))
    for key, data in _own_streams():
        _check_stages(data, subseq_bytes, key)


@pytest.mark.parametrize("subseq_bytes", [jpeg_decode.SUBSEQ_DEFAULT, jpeg_decode.SUBSEQ_MIN])
def test_host_build_on_a_stream_of_several_runs(subseq_bytes):
    """160 x 160 noise at quality 100, 4:4:4, no restart markers: several workgroup runs, and launches after the first that find work"""
    r = _check_stages(cases.multi_run_stream(), subseq_bytes, "multi-run")
    assert r.launches >= 3 and r.rounds >= 2, (r.launches, r.rounds)


def test_slow_to_synchronise_stream():
    """a stream whose lanes do not agree within a round: in this noise at quality 100 every block holds all 64 coefficients, the three components' blocks look
    alike, and a lane that starts on the wrong component stays on it -- so a run of n lanes needs its n + 1 rounds (the restatement counts the same), and with runs
    of 2 or 4 lanes every launch settles exactly one more run: the worst case the bound is derived for, reached and not exceeded"""
    data = cases.slow_stream()
    r = _check_stages(data, jpeg_decode.SUBSEQ_MIN, "slow")
    assert r.iters == r.nsub + 1 and r.iters > 100
    assert (r.rounds, r.iters, r.launches) == jpegdec_np.sync_rounds(data, jpeg_decode.SUBSEQ_MIN)
    for lanes in (4, 2):
        r = _check_stages(data, jpeg_decode.SUBSEQ_MIN, "slow, runs of %d" % lanes, lanes=lanes)
        assert r.rounds == r.launches > 40 and r.iters == lanes + 1
        assert (r.rounds, r.iters, r.launches) == jpegdec_np.sync_rounds(data, jpeg_decode.SUBSEQ_MIN, lanes)


# ---- the parser ----
def _patched(data, marker, at, value):
    """the byte `at` bytes behind the first marker `marker` (0xFF, marker) replaced"""
    i = data.index(bytes([0xFF, marker]))
    return data[:i + at] + bytes([value]) + data[i + at + 1:]


def test_parse_takes_the_matrix_and_refuses_what_is_out_of_scope():
    rgb = cases.frame(17, 33, "noise", seed=3)
    good = cases.write(rgb, "420", 75)
    info = jpeg_decode.parse(good)
    assert (info.H, info.W, info.components, info.sampling) == (17, 33, 3, jpeg_decode.SAMPLING["420"])
    assert good[int(info.desc["scan_off"]) + int(info.desc["scan_len"]):] == b"\xff\xd9"
    for (size, sampling), files in cases.matrix().items():
        i = jpeg_decode.parse(files[0][1])
        assert (i.H, i.W, i.sampling) == (size[0], size[1], jpeg_decode.SAMPLING[sampling])
    sof = good.index(b"\xff\xc0")
    refused = {
        "progressive (SOF2)": cases.write(rgb, "420", 75, progressive=True),
        "four components (CMYK)": cases.write(rgb, "444", 75, mode="CMYK"),
        "extended sequential (SOF1)": _patched(good, 0xC0, 1, 0xC1),
        "lossless (SOF3)": _patched(good, 0xC0, 1, 0xC3),
        "arithmetic coding (SOF9)": _patched(good, 0xC0, 1, 0xC9),
        "12-bit precision": _patched(good, 0xC0, 4, 12),
        "16-bit quantisation table": _patched(good, 0xDB, 4, 0x10),
        "sampling 4:1:1": _patched(good, 0xC0, 11, 0x41),
        "sampling 1x2": _patched(good, 0xC0, 11, 0x12),
        "subsampled chrominance over it": _patched(good, 0xC0, 14, 0x21),
        "DNL (no height in SOF0)": good[:sof + 5] + b"\0\0" + good[sof + 7:],
        "DNL segment": good[:sof] + b"\xff\xdc\x00\x04\x00\x11" + good[sof:],
        "a width above the ABI's limit": good[:sof + 7] + struct.pack(">H", jpeg_decode.MAX_SIDE + 1) + good[sof + 9:],
        "two scans": good[:-2] + good[good.index(b"\xff\xda"):],
        "Adobe RGB": good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + good[2:],
        "a table the scan names is missing": _patched(good, 0xDA, 6, 0x33),
        "not a JPEG": b"\x89PNG\r\n\x1a\n" + good,
        "empty": b"",
    }
    for what, data in refused.items():
        assert jpeg_decode.parse(data) is None, what
    from PIL import Image
    for what in ("progressive (SOF2)", "four components (CMYK)"):      # real files, which Pillow itself opens
        assert Image.open(io.BytesIO(refused[what])).size == (33, 17)
    assert jpeg_decode.parse(good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + good[2:]) is not None      # Adobe, transform YCbCr


# ---- corrupt streams: the host build only ----
def _corrupt_set():
    """-> (info of the sound file, [corrupt files]): a small file cut at every 37th byte, and 200 seeded single-byte corruptions of its scan"""
    good = cases.write(cases.frame(37, 53, "noise", seed=11), "420", 75, restart=3)
    info = jpeg_decode.parse(good)
    out = [good[:n] for n in range(0, len(good), 37)]
    rng = np.random.RandomState(5)
    lo, hi = int(info.desc["scan_off"]), len(good) - 2
    for _ in range(200):
        at = int(rng.randint(lo, hi))
        out.append(good[:at] + bytes([int(rng.randint(0, 256))]) + good[at + 1:])
    return good, info, out


def _records(info, files):
    """every corrupt file with the record the product's parser gives it (a file the parser refuses never reaches the decoder; a cut file keeps the sound file's
    record where the parser still accepts the header) -> [(record, bytes)]"""
    out = []
    for data in files:
        i = jpeg_decode.parse(data)
        if i is None or (i.H, i.W, i.sampling) != (info.H, info.W, info.sampling):
            continue
        out.append((i, data))
    return out


def test_corrupt_streams_are_harmless_on_the_host_build():
    good, info, files = _corrupt_set()
    recs = _records(info, files)
    assert len(recs) >= 200
    ref = cases.reference(good)[2]
    flagged = same = 0
    for i, data in recs:
        for subseq_bytes in (jpeg_decode.SUBSEQ_DEFAULT, jpeg_decode.SUBSEQ_MIN):
            r = hostsim.decode(data, i, subseq_bytes)      # returns: every loop of the decoder is bounded by the scan's length
            assert r.rc == 0 and r.clean, "a write outside the frame or the workspace"
            if r.status == 0:      # "yields a frame": the stream is still a sound one, and the frame is the restatement's decode of it
                assert np.array_equal(r.frame, jpegdec_np.decode(data)), "status 0 on a stream the restatement reads otherwise"
            flagged += r.status != 0
            same += r.status == 0 and np.array_equal(r.frame, ref)
    assert flagged >= 100      # most corruptions break the code; one that lands in a value's bits decodes to another picture with status 0
    # a record that lies about its file is refused like the C ABI refuses it
    bad = info._replace(desc=info.desc.copy())
    bad.desc["scan_len"] = len(good)
    assert hostsim.decode(good, bad, jpeg_decode.SUBSEQ_DEFAULT).rc == -1


def test_corrupt_streams_under_the_sanitizers_in_a_program_of_their_own(tmp_path):
    """tests/_hostsim/jpegdec_corrupt_main.cpp built with -fsanitize=address,undefined and run over the same set: it must exit clean.  Nothing is preloaded and
    nothing that Python loads is sanitised."""
    _, info, files = _corrupt_set()
    recs = _records(info, files)
    blob = bytearray()
    n = 0
    for i, data in recs:
        for subseq_bytes in (jpeg_decode.SUBSEQ_DEFAULT, jpeg_decode.SUBSEQ_MIN):
            blob += struct.pack("<6i", i.H, i.W, i.sampling, subseq_bytes, hostsim.LANES, len(data)) + np.array(i.desc).tobytes() + data
            n += 1
    path = tmp_path / "set.bin"
    path.write_bytes(struct.pack("<i", n) + bytes(blob))
    exe = tmp_path / "jpegdec_corrupt"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", os.path.join(ROOT, "tests", "_hostsim", "jpegdec_corrupt_main.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)      # (the sanitizers' runtimes are linked statically: the environment is the caller's)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    assert run.stdout.startswith("%d cases, " % n)


# ---- the loader ----
def _folder(tmp_path, progressive_at=None):
    seq = tmp_path / "seq"
    seq.mkdir()
    files = []
    for k in range(4):
        data = cases.write(cases.frame(24, 40, "noise", seed=20 + k), "420", 90, progressive=(k == progressive_at))
        (seq / ("%05d.jpg" % k)).write_bytes(data)
        files.append(data)
    return seq, files


def test_loader_with_device_decode_hands_over_the_files_bytes(tmp_path):
    import torch
    from yolov7_tracker_amd.tracker import tracker_dataloader
    seq, files = _folder(tmp_path)
    loader = tracker_dataloader.TrackerLoader(str(seq), 640, device_decode=True)
    assert [loader[k][1] for k in range(len(loader))] == files and loader[0][0].numel() == 0
    batches = list(torch.utils.data.DataLoader(loader, batch_size=3, collate_fn=tracker_dataloader.collate_bytes))
    assert [b for _, part in batches for b in part] == files and [len(part) for _, part in batches] == [3, 1]
    plain = tracker_dataloader.TrackerLoader(str(seq), 640, device_preprocess=True)      # the switch off: the decoded frame, as before
    assert np.array_equal(plain[1][1].numpy(), cases.pillow_bgr(files[1]))


def test_parse_refuses_the_progressive_file_of_a_folder_and_the_host_decodes_it(tmp_path):
    """(the fallback COUNT of such a folder is the CLI's: tests/test_jpegdec_cli_gpu.py)"""
    from yolov7_tracker_amd.tracker import tracker_dataloader
    seq, files = _folder(tmp_path, progressive_at=2)
    loader = tracker_dataloader.TrackerLoader(str(seq), 640, device_decode=True)
    infos = [jpeg_decode.parse(loader[k][1]) for k in range(len(loader))]
    assert [i is None for i in infos] == [False, False, True, False]
    assert np.array_equal(jpeg_decode.decode_host(files[2]), cases.pillow_bgr(files[2]))      # ... and the fallback is today's path
