"""CPU: the annotated-frame path without a GPU.  The host build of csrc/y7t_render.h (tests/_hostsim/render.py -- the functions the device kernels call) against the
NumPy restatement of DESIGN.md section 4 "Rendering" (tests/render_np.py): the overlay array-equal, the JPEG files byte for byte; Pillow (libjpeg) as the independent
decoder of every stream and the independent encoder the quality is measured against; the header's facts; the Motion-JPEG AVI."""
import io
import struct
import warnings

import numpy as np
import pytest

from tests import render_np as rn
from tests import render_scenes as rs

# twice the largest shortfall of the NumPy restatement against Pillow's encoder over these very scenes (scripts/render_margins.py -> profiles/render_margins.txt:
# 0.0457 dB, 0.13838 of the size -- small files are mostly header, and ours carries DRI and a restart marker per MCU row)
PSNR_MARGIN_DB = 0.0914
SIZE_MARGIN = 0.27676
CASES = [(sub, W, H, name) for sub in rs.SUBSAMPLINGS for W, H in rs.shapes(sub) for name in rs.SCENES]
_host = {}


def host_files(sub, W, H, name):
    """the host build's file at every quality, encoded once and shared"""
    from tests._hostsim import render as hs
    key = (sub, W, H, name)
    if key not in _host:
        frame = rs.scene(name, W, H)
        _host[key] = (frame, {q: hs.encode(frame, q, sub) for q in rs.QUALITIES})
    return _host[key]


# ---- overlay ----
@pytest.mark.parametrize("name", sorted(rs.OVERLAY_CASES))
def test_overlay_host_build_equals_the_restatement(name):
    from tests._hostsim import render as hs
    frame, tracks = rs.overlay_case(name)
    got = hs.draw(frame[None], [tracks])
    assert np.array_equal(got, rn.draw(frame[None], [tracks]))
    changed = np.any(got[0] != frame, -1)
    if name == "none" or name.startswith("outside"):
        assert not changed.any()      # nothing to draw, or every primitive beyond the frame: the frame as it came
    else:
        assert changed.any()


def test_overlay_facts():
    """the geometry the specification names, pixel by pixel on the host build"""
    from tests._hostsim import render as hs
    frame = np.zeros((48, 64, 3), np.uint8)
    # x = -0.5, y = -0.99 truncate toward zero to 0, 0 (floor would give -1): the outline's columns are -1 .. 1, so column 1 is drawn and column 2 is not
    out = hs.draw(frame[None], [[(-0.5, -0.99, 20.9, 12.5, 8, b"")]])[0]
    color = rn.get_color(8)
    assert tuple(out[5, 1]) == color and tuple(out[5, 2]) == (0, 0, 0) and tuple(out[1, 5]) == color and tuple(out[2, 5]) == (0, 0, 0)
    assert tuple(out[5, 19]) == color and tuple(out[5, 21]) == color and tuple(out[5, 22]) == (0, 0, 0) and tuple(out[5, 18]) == (0, 0, 0)      # int(-0.5 + 20.9) = 20
    # a zero-area box is the 3 x 3 dot of its thickened point
    out = hs.draw(frame[None], [[(30.0, 30.0, 0.0, 0.0, 9, b"")]])[0]
    assert np.argwhere(np.any(out != 0, -1)).tolist() == [[y, x] for y in (29, 30, 31) for x in (29, 30, 31)]
    # colours: id 0 black, 85 wraps (3 * 85 = 255), 2^31 - 1 needs 64 bits
    assert rn.get_color(85) == (0, 0, 0) and rn.get_color(2 ** 31 - 1) == ((37 * 3 * (2 ** 31 - 1)) % 255, (17 * 3 * (2 ** 31 - 1)) % 255, (29 * 3 * (2 ** 31 - 1)) % 255)
    out = hs.draw(frame[None] + 7, [[(10.0, 20.0, 20.0, 10.0, 2 ** 31 - 1, b""), (40.0, 20.0, 10.0, 10.0, 1, b"")]])[0]
    assert tuple(out[20, 15]) == rn.get_color(2 ** 31 - 1) and tuple(out[20, 45]) == (111, 51, 87)
    # the later track wins: its rectangle over the earlier label and over the earlier rectangle; its own label over both
    first, second = (10.0, 20.0, 30.0, 20.0, 12, b"van-12"), (8.0, 8.0, 30.0, 20.0, 13, b"bus-13")
    both = hs.draw(frame[None], [[first, second]])[0]
    only_first, only_second = hs.draw(frame[None], [[first]])[0], hs.draw(frame[None], [[second]])[0]
    text = np.all(only_first == rn.TEXT_COLOR, -1)
    ring2 = np.all(only_second == rn.get_color(13), -1)
    assert (text & ring2).any(), "the scene no longer puts the later rectangle over the earlier label"
    assert np.array_equal(both[np.any(only_second != 0, -1)], only_second[np.any(only_second != 0, -1)])
    rest = ~np.any(only_second != 0, -1)
    assert np.array_equal(both[rest], only_first[rest])
    # the input is not modified and an empty label draws nothing but the box
    assert not frame.any()


# ---- JPEG ----
@pytest.mark.parametrize("sub,W,H,name", CASES)
def test_jpeg_host_build_equals_the_restatement(sub, W, H, name):
    frame, files = host_files(sub, W, H, name)
    for q in rs.QUALITIES:
        assert files[q] == rn.encode(frame, q, sub), (q,)


@pytest.mark.parametrize("sub,W,H,name", CASES)
def test_pillow_decodes_every_stream_to_its_own_coefficients(sub, W, H, name):
    """libjpeg's planes lie within 1.0 (IEEE 1180's peak error of its integer IDCT) of the float64 inverse DCT of the coefficients the stream carries: every
    coefficient was coded, stuffed and delimited correctly.  4:4:4: all three planes (draft YCbCr: no colour conversion, no upsampling); 4:2:0: the Y plane"""
    from PIL import Image
    frame, files = host_files(sub, W, H, name)
    for q in rs.QUALITIES:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            im = Image.open(io.BytesIO(files[q]))
            assert im.size == (W, H) and im.format == "JPEG"
            im.draft("YCbCr" if sub == "444" else "L", im.size)
            im.load()
        got = np.asarray(im).astype(np.float64).reshape(H, W, -1)
        coefs, qt = rn.coefficients(frame, q, sub)
        want = rn.idct_planes(coefs, qt)
        assert got.shape[2] == (3 if sub == "444" else 1)
        for c in range(got.shape[2]):
            err = np.abs(got[..., c] - want[c][:H, :W]).max()
            assert err <= 1.0, (q, c, err)


@pytest.mark.parametrize("sub,W,H,name", CASES)
def test_quality_and_size_against_pillows_encoder(sub, W, H, name):
    frame, files = host_files(sub, W, H, name)
    for q in rs.QUALITIES:
        ours, theirs, n_ours, n_theirs = rn.against_pillow(frame, files[q], q, sub)
        print("%s %dx%d %s q%d: PSNR %.3f dB (Pillow %.3f), %d bytes (Pillow %d)" % (name, W, H, sub, q, ours, theirs, n_ours, n_theirs))
        assert ours >= theirs - PSNR_MARGIN_DB, (q, ours, theirs)
        assert n_ours <= n_theirs * (1 + SIZE_MARGIN), (q, n_ours, n_theirs)


@pytest.mark.parametrize("sub", rs.SUBSAMPLINGS)
@pytest.mark.parametrize("q", rs.QUALITIES)
def test_header_facts(sub, q):
    W, H = rs.shapes(sub)[4]      # more than 8 MCU rows
    frame, files = host_files(sub, W, H, "ramps")
    data = files[q]
    segs, start = rn.segments(data)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA] and segs[0][1][:5] == b"JFIF\0"
    # DQT: the IJG scaling of Annex K (typed here from the standard's luminance table; the chrominance one through Pillow's quality-50 file)
    k1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
    s = 5000 // q if q < 50 else 200 - 2 * q
    lum = np.clip((np.array(k1) * s + 50) // 100, 1, 255)
    assert list(segs[1][1][1:]) == lum[rn.ZIG].tolist() and segs[1][1][0] == 0
    assert list(segs[2][1][1:]) == rn.quant_tables(q)[1][rn.ZIG].tolist() and segs[2][1][0] == 1
    sof = segs[3][1]
    assert sof[0] == 8 and struct.unpack(">HH", sof[1:5]) == (H, W) and sof[5] == 3
    assert [sof[7], sof[10], sof[13]] == ([0x22, 0x11, 0x11] if sub == "420" else [0x11, 0x11, 0x11])
    m = 16 if sub == "420" else 8
    mcols, mrows = -(-W // m), -(-H // m)
    assert struct.unpack(">H", segs[8][1])[0] == mcols and mrows > 8
    # the restart markers: every FF that is neither stuffed nor EOI, in order, cycling 0 .. 7
    body = data[start:]
    marks = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] != 0]
    assert marks == [0xD0 + r % 8 for r in range(mrows - 1)] + [0xD9] and data[-2:] == b"\xff\xd9"


def test_scenes_drive_the_mechanisms_they_are_for():
    """a scene that stops exercising its mechanism fails here, not silently"""
    for sub in rs.SUBSAMPLINGS:
        stats = {}
        data = rn.encode(rs.scene("random", 48, 64), 100, sub, stats)
        assert b"\xff\x00" in data[rn.segments(data)[1]:] and stats["stuffed"] > 0 and stats["dc_cat"] == 11
        rn.encode(rs.scene("basis77", 48, 64), 95, sub, stats)
        assert stats["zrl"] > 0
        rn.encode(rs.scene("flat", 48, 64), 95, sub, stats)
        assert stats["zrl"] == 0 and stats["dc_cat"] <= 8
        coefs, _ = rn.coefficients(rs.scene("alternate", 48, 64), 95, sub)
        dc = coefs[0][..., 0, 0]
        assert dc.max() > 900 // 2 and dc.min() < -900 // 2      # (quality 95: the luminance DC's quantiser is 2)
        # the strip: more than 256 blocks in its one MCU row, so the device takes it in chunks
        assert 1920 // (16 if sub == "420" else 8) * (6 if sub == "420" else 3) > 256


def test_worst_case_row_fits_its_slot():
    """the longest code a block can have is 22 bits of DC and 63 x 26 of AC; the random scene at quality 100 comes near it and stays below the slot's share"""
    for sub in rs.SUBSAMPLINGS:
        data = rn.encode(rs.scene("random", 200, 120), 100, sub)
        m = 16 if sub == "420" else 8
        blocks = -(-200 // m) * -(-120 // m) * (6 if sub == "420" else 3)
        assert len(data) < blocks * 216 * 2 and len(data) > blocks * 60


# ---- AVI ----
def riff_chunks(data, at, end):
    out = []
    while at < end:
        tag, n = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        out.append((tag, at + 8, n))
        at += 8 + n + (n & 1)
    assert at == end
    return out


def test_mjpeg_avi_holds_the_very_jpeg_files(tmp_path):
    from tests._hostsim import render as hs
    from yolov7_tracker_amd.tracker.render import write_mjpeg_avi
    W, H = 48, 64
    files = [hs.encode(rs.scene(name, W, H), 95, "420") for name in ("ramps", "flat", "random", "basis77")]
    assert any(len(f) & 1 for f in files) and any(not len(f) & 1 for f in files), "the scenes no longer give chunks of odd and of even length"
    data = open(write_mjpeg_avi(str(tmp_path / "v" / "seq.avi"), files, (W, H), fps=15), "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    top = riff_chunks(data, 12, len(data))
    assert [t for t, _, _ in top] == [b"LIST", b"LIST", b"idx1"] and data[top[0][1]:top[0][1] + 4] == b"hdrl" and data[top[1][1]:top[1][1] + 4] == b"movi"
    hdrl = riff_chunks(data, top[0][1] + 4, top[0][1] + top[0][2])
    assert [t for t, _, _ in hdrl] == [b"avih", b"LIST"]
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    assert avih[0] == 1000000 // 15 and avih[4] == len(files) and avih[6] == 1 and (avih[8], avih[9]) == (W, H) and avih[3] & 0x10
    assert data[hdrl[1][1]:hdrl[1][1] + 4] == b"strl"
    strl = riff_chunks(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [t for t, _, _ in strl] == [b"strh", b"strf"]
    strh = data[strl[0][1]:strl[0][1] + strl[0][2]]
    assert strh[:8] == b"vidsMJPG" and struct.unpack("<II", strh[20:28]) == (1, 15) and struct.unpack("<I", strh[32:36])[0] == len(files)
    strf = data[strl[1][1]:strl[1][1] + strl[1][2]]
    assert struct.unpack("<Iii", strf[:12]) == (40, W, H) and strf[16:20] == b"MJPG"
    movi_at = top[1][1]
    frames = riff_chunks(data, movi_at + 4, movi_at + top[1][2])
    assert [t for t, _, _ in frames] == [b"00dc"] * len(files)
    assert [data[a:a + n] for _, a, n in frames] == files      # one chunk per frame, byte-equal to the .jpg; riff_chunks checked the padding to even
    idx = data[top[2][1]:top[2][1] + top[2][2]]
    assert len(idx) == 16 * len(files)
    for k, (_, a, n) in enumerate(frames):
        tag, flags, off, size = idx[16 * k:16 * k + 4], *struct.unpack("<III", idx[16 * k + 4:16 * k + 16])
        assert tag == b"00dc" and flags & 0x10 and size == n and movi_at + off == a - 8      # the offset points at the chunk's header, counted from 'movi'


def test_labels_and_track_rows():
    from yolov7_tracker_amd.tracker import render
    assert render.label_for(3, 17, {3: "car"}) == b"car-17" and render.label_for(3.0, 17, {}) == b"3-17" and render.label_for(np.float32(2), 5, None) == b"2-5"
    assert len(render.label_for(1, 2 ** 31 - 1, {1: "a-very-long-category-name"})) == 24
    rows, off = render.pack_tracks([[(1.5, 2.5, 3.0, 4.0, 7, b"0-7")], [], [(0, 0, 1, 1, 1, b""), (0, 0, 1, 1, 2, b"x" * 30)]])
    assert rows.dtype.itemsize == 48 and off.tolist() == [0, 1, 1, 3] and rows["len"].tolist() == [3, 0, 24] and bytes(rows["label"][0][:3]) == b"0-7"
