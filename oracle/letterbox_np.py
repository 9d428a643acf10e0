"""oracle/letterbox_np.py -- TEST INFRASTRUCTURE ONLY.

numpy restatement of the reference's frame pre-processing, /root/reference/tracker/tracker_dataloader.py:64-130:
`_letterbox` (scale ratio, `auto=True` padding to the stride multiple, cv2.resize INTER_LINEAR, cv2.copyMakeBorder 114) and the
BGR->RGB / CHW / float32 / 255 tail of `__getitem__`.

What is pinned for the resize (tests/preproc_ref.py, tests/test_preprocess_cpu.py, tests/test_preprocess_gpu.py):
  * `resize_bilinear` == the device samplers k_letterbox_layout and k_stem_u8, bit for bit: the same sequence of IEEE float32 operations (the device files are
    compiled without FMA contraction), checked on up- and downscaled, odd-sized, one-row and one-column frames, on noise and on smooth images.  The host
    loader's `_resize_linear` (yolov7_tracker_amd/tracker/tracker_dataloader.py) is this expression written out a second time, so its equality with this one is a
    guard against the two copies drifting apart, not evidence for either;
  * all of them == rint of the same formula evaluated in float64 wherever that value is further from a rounding tie than an a-priori bound on the float32
    error (the "decided" pixels, 95-100 % of them), and within one grey level elsewhere; at scale 2, 1/2 and 3/2 the float32 arithmetic is exact and every
    value is equal, ties rounded half to even.
PARITY STILL UNPINNED: OpenCV itself.  cv2 is not installed here and the reference has no fixture for it.  This restates cv2.INTER_LINEAR's geometry (half-pixel
centres, edge-clamped taps) in float arithmetic with rounding to uint8; OpenCV's own 8-bit path uses 11-bit fixed-point weights and rounds half up, so it can
differ from this by one grey level near rounding ties -- on the exact x2 shrink at every tie whose floor is even.
"""
import numpy as np


def letterbox(img, new_shape=(640, 640), color=(114, 114, 114), auto=True, scaleup=True, stride=32):
    shape = img.shape[:2]
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)
    dw /= 2
    dh /= 2
    if shape[::-1] != new_unpad:
        img = resize_bilinear(img, new_unpad[1], new_unpad[0])
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    out = np.empty((img.shape[0] + top + bottom, img.shape[1] + left + right, 3), np.uint8)
    row = np.empty((out.shape[1], 3), np.uint8)
    row[...] = np.asarray(color, np.uint8)
    out[...] = row                      # whole rows of the pad colour: 20 times faster at 1280 x 1280 than broadcasting the three bytes over every pixel
    out[top:top + img.shape[0], left:left + img.shape[1]] = img
    return out


def resize_bilinear(img, new_h, new_w):
    H0, W0 = img.shape[:2]
    f32 = np.float32
    fy = (np.arange(new_h, dtype=f32) + f32(0.5)) * f32(f32(H0) / f32(new_h)) - f32(0.5)
    fx = (np.arange(new_w, dtype=f32) + f32(0.5)) * f32(f32(W0) / f32(new_w)) - f32(0.5)
    y0, x0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
    wy, wx = (fy - y0.astype(f32))[:, None, None], (fx - x0.astype(f32))[None, :, None]
    y1, x1 = np.clip(y0 + 1, 0, H0 - 1), np.clip(x0 + 1, 0, W0 - 1)
    y0, x0 = np.clip(y0, 0, H0 - 1), np.clip(x0, 0, W0 - 1)
    im = img.astype(f32)
    t0 = (f32(1) - wx) * im[y0][:, x0] + wx * im[y0][:, x1]
    t1 = (f32(1) - wx) * im[y1][:, x0] + wx * im[y1][:, x1]
    return np.rint((f32(1) - wy) * t0 + wy * t1).astype(np.uint8)


def to_model_input(img_bgr_u8):
    """__getitem__ tail: BGR HWC uint8 -> RGB CHW float32 / 255"""
    x = np.ascontiguousarray(img_bgr_u8[:, :, ::-1].transpose(2, 0, 1)).astype(np.float32)
    return x / np.float32(255.0)
