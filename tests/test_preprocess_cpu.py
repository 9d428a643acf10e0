"""CPU: the host side of the frame pre-processing, pinned without a GPU.

  * the two float32 restatements of the letterbox resize -- oracle/letterbox_np.py::resize_bilinear (what the device kernels are compared with bit for bit in
    tests/test_preprocess_gpu.py) and tracker/tracker_dataloader.py::_resize_linear (what the host loader feeds the network) -- against each other and against
    the float64 formula of tests/preproc_ref.py, at every resampled geometry of its table and on both image kinds;
  * the letterbox geometry rule of the loader, the oracle and Detector.letterbox_params against each other over a few thousand frame shapes;
  * the loader's whole letterboxed image against the oracle's.
Not pinned anywhere: OpenCV's own 8-bit INTER_LINEAR path (11-bit fixed-point weights, round half up on the x2 shrink); cv2 is not available to the suite."""
import zlib

import numpy as np
import pytest

from oracle import letterbox_np as lb
from tests import preproc_ref as pr
from tests.preproc_ref import GEOMETRIES, KINDS

RESAMPLED = [r for r in GEOMETRIES if r.resampled]
UNDECIDED_CAP = 0.05


def _loader():
    from yolov7_tracker_amd.tracker import tracker_dataloader
    return tracker_dataloader


def test_geometry_table():
    """the table's geometry column is what Detector.letterbox_params computes, and the stem instantiation it names is what the launcher's rule gives"""
    from yolov7_tracker_amd.detector.model import Detector
    for r in GEOMETRIES:
        assert tuple(int(v) for v in Detector.letterbox_params(r.shape, r.img_size, r.stride)) == r.geom, r
        if r.stem is not None:
            assert pr.stem_kernel_rule(r.shape, r.geom) == r.stem, r
            assert r.geom[0] % 64 == 0 and r.geom[1] % 64 == 0, r           # a yolov7-w6 plan exists
    bottom = lambda r: r.geom[0] - r.geom[4] - r.geom[2]
    right = lambda r: r.geom[1] - r.geom[5] - r.geom[3]
    assert bottom(pr.ROWS["157x211"]) == 17 and right(pr.ROWS["211x157"]) == 17 and bottom(pr.ROWS["157x211/s32"]) == 1 and right(pr.ROWS["128x91"]) == 19
    assert 9 * (512 // 32) ** 2 == 2304 > 2048                              # 16 x 16 tiles of the 256 x 256 ReOrg map: 256 workgroups get a second tile
    assert 1536 * 1536 > 8192 * 256                                         # k_letterbox_layout's grid is capped at 8192 blocks


def test_fp16_of_a_grey_level_does_not_depend_on_the_route():
    """the layout tensor's value of grey level g: float32 g / 255 rounded to fp16 (the kernels) == float64 g / 255 rounded to fp16 == fp16(g * fl32(1 / 255)) (the
    direct stem loader)"""
    g = np.arange(256)
    a = pr.u8_to_f16(g)
    assert np.array_equal(a.view(np.int16), (g / 255.0).astype(np.float16).view(np.int16))
    assert np.array_equal(a.view(np.int16), (g.astype(np.float32) * np.float32(0.00392156862745098)).astype(np.float16).view(np.int16))


@pytest.mark.parametrize("row", RESAMPLED, ids=repr)
def test_restatements_against_float64(row):
    """oracle and loader resize bit-equal (one formula written twice: this keeps the copies together, the evidence is the float64 reference); both == rint(v) on every decided pixel and within one grey level everywhere; equal to rint(v) everywhere where the
    arithmetic is exact (scale 2, 1/2, 3/2: numpy's rint rounds half to even like rintf); at most 5 % of the pixels undecided elsewhere"""
    td = _loader()
    _, _, new_h, new_w, _, _ = row.geom
    for kind in KINDS:
        for b, frame in enumerate(pr.frames_for(row, kind)):
            a = lb.resize_bilinear(frame, new_h, new_w)
            c = td._resize_linear(frame, new_h, new_w)
            assert a.dtype == c.dtype == np.uint8 and a.shape == c.shape == (new_h, new_w, 3)
            assert np.array_equal(a, c), "the oracle's and the loader's resize differ"
            v, delta = pr.resize_f64(frame, new_h, new_w)
            want = np.rint(v)
            dec = pr.decided(v, delta)
            share = 1.0 - dec.mean()
            off = np.abs(a.astype(np.float64) - want)
            print("UNDECIDED %-14s %-6s frame %d  %dx%d -> %dx%d  undecided %.3f %%  float32 != rint(v): %d of %d" % (
                row.name, kind, b, row.shape[0], row.shape[1], new_h, new_w, 100 * share, int((off > 0).sum()), off.size))
            assert not (off[dec] > 0).any(), "%d decided pixels differ from rint(v)" % int((off[dec] > 0).sum())
            assert off.max() <= 1
            if row.exact:
                assert np.array_equal(a, want.astype(np.uint8)), "%d values differ on an exact scale" % int((off > 0).sum())
            else:
                assert share <= UNDECIDED_CAP, share


def test_exact_shrink_has_ties_and_rounds_them_to_even():
    """128 x 256 -> 64 x 128 on noise: v is the mean of four grey levels, so a quarter of the values end in .5; the case means something only if both parities occur"""
    row = pr.ROWS["128x256"]
    frame = pr.frames_for(row, "noise")[0]
    v, _ = pr.resize_f64(frame, 64, 128)
    tie = (v - np.floor(v)) == 0.5
    assert 0.2 < tie.mean() < 0.3
    got = lb.resize_bilinear(frame, 64, 128)
    assert (got[tie] % 2 == 0).all() and (np.floor(v[tie]) % 2 == 0).any() and (np.floor(v[tie]) % 2 == 1).any()


def _shapes():
    rng = np.random.default_rng(zlib.crc32(b"letterbox shapes"))
    small = [(h, w) for h in range(1, 71) for w in range(1, 71)]
    return small + [tuple(int(v) for v in rng.integers(1, 2001, 2)) for _ in range(400)]


@pytest.mark.parametrize("img_size", [64, 128, 640, 1280])
def test_geometry_rule_of_loader_oracle_and_detector(monkeypatch, img_size):
    """Detector.letterbox_params, letterbox_np.letterbox and tracker_dataloader.letterbox place the same new_h x new_w image at the same (top, left) of the same
    H x W canvas, for every (H0, W0) in [1, 70]^2 and 400 random shapes up to 2000, at both strides.  The two image-producing ones run with their resize replaced
    by a constant image of the requested size (the resize itself is judged above; the rule does not depend on it): the size they ask for and the corners of the
    constant block in the padded result give their geometry."""
    from yolov7_tracker_amd.detector.model import Detector
    td = _loader()
    asked = []

    def stub(img, new_h, new_w):
        asked.append((new_h, new_w))
        return np.full((new_h, new_w, 3), 7, np.uint8)
    monkeypatch.setattr(lb, "resize_bilinear", stub)
    monkeypatch.setattr(td, "_resize_linear", stub)
    n = 0
    for (h0, w0) in _shapes():
        frame = np.full((h0, w0, 3), 7, np.uint8)
        for stride in (32, 64):
            H, W, new_h, new_w, top, left = (int(v) for v in Detector.letterbox_params((h0, w0), img_size, stride))
            assert H % stride == 0 and W % stride == 0 and H > 0 and W > 0
            assert 0 <= top and 0 <= left and top + new_h <= H and left + new_w <= W and new_h >= 1 and new_w >= 1, (h0, w0, img_size, stride)
            bottom, right = H - top - new_h, W - left - new_w
            assert abs(bottom - top) <= 1 and abs(right - left) <= 1
            del asked[:]
            a = lb.letterbox(frame, new_shape=(img_size, img_size), stride=stride)
            c = td.letterbox(frame, new_shape=(img_size, img_size), stride=stride)[0]
            assert asked in ([], [(new_h, new_w)] * 2) and (asked or (new_h, new_w) == (h0, w0))
            for img in (a, c):
                assert img.shape == (H, W, 3)
                assert (img[top, left] == 7).all() and (img[top + new_h - 1, left + new_w - 1] == 7).all()
                assert top == 0 or (img[top - 1, left] == 114).all()
                assert left == 0 or (img[top, left - 1] == 114).all()
                assert bottom == 0 or (img[top + new_h, left] == 114).all()
                assert right == 0 or (img[top, left + new_w] == 114).all()
            n += 1
    assert n == (70 * 70 + 400) * 2


@pytest.mark.parametrize("row", GEOMETRIES, ids=repr)
def test_whole_letterboxed_image_of_the_loader_equals_the_oracle(row):
    """tracker_dataloader.letterbox == letterbox_np.letterbox on every row: pad colour 114 exactly outside, the resampled (or copied) pixels inside"""
    td = _loader()
    H, W, new_h, new_w, top, left = row.geom
    for kind in KINDS:
        for frame in pr.frames_for(row, kind)[:2]:
            a = pr.letterbox_f32(frame, row.img_size, row.stride)
            c, ratio, (dw, dh) = td.letterbox(frame, new_shape=(row.img_size, row.img_size), stride=row.stride)
            assert a.shape == c.shape == (H, W, 3) and a.dtype == c.dtype == np.uint8
            assert np.array_equal(a, c)
            outside = np.ones((H, W), bool)
            outside[top:top + new_h, left:left + new_w] = False
            assert (c[outside] == 114).all()
            inside = c[top:top + new_h, left:left + new_w]
            want = lb.resize_bilinear(frame, new_h, new_w) if row.resampled else frame
            assert np.array_equal(inside, want)
