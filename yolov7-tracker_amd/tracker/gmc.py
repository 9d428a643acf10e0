"""Camera-motion estimation on the device: the `GMC` class of the reference (its tracker/botsort.py:13-248) for method='ecc' -- cv2.findTransformECC
with MOTION_EUCLIDEAN on a blurred half-resolution gray frame (botsort.py:78-109) -- as HIP kernels of liby7t.so (csrc/y7t_ecc.hip: y7t_ecc_prepare_u8,
y7t_ecc_align).  DESIGN.md section 4 "GMC / ECC" states the arithmetic and what is not claimed against OpenCV's fixed-point 8-bit routines.

    tracker.ECC = GMC('ecc')                    # StrongSORT: an object with apply(raw_frame, detections) -> (2, 3)
    tracker.gmc = GMC('ecc').apply_device       # BoT-SORT: the warp stays on the device, no host round trip

method='features' is the feature path of the reference (applyFeaures, botsort.py:111-235, what its BoT-SORT runs as GMC('orb')): FAST corners, rotated-BRIEF
descriptors, Hamming 2-NN matching, the three filters and a 4-DOF RANSAC as kernels of csrc/y7t_orb.hip (y7t_orb_extract_u8, y7t_orb_estimate) -- a specification
of our own, DESIGN.md section 4 "GMC / features", not OpenCV's ORB.

    tracker.gmc = GMC('features').apply_device  # BoT-SORT: the frame's detections mask their boxes out of the corners

Out of this scope: method 'orb', 'sift' (OpenCV's own detectors and estimateAffinePartial2D) and 'file' (pre-computed matrices of MOTChallenge): NotImplementedError."""
import numpy as np

MOTION_EUCLIDEAN = 1      # cv2.MOTION_EUCLIDEAN == Y7T_ECC_MOTION_EUCLIDEAN
FAILED = 3                # Y7T_ECC_STATUS_FAILED


class _DeviceEcc:
    """the two launches' worth of liby7t.so: frames and planes are torch tensors on the GPU"""

    def __init__(self):
        import torch
        from .. import _lib
        _lib.require_gpu()
        self._torch, self._lib, self._L = torch, _lib, _lib.load()
        self._ws = {}

    def prepare(self, frame, downscale):
        torch, _lib = self._torch, self._lib
        if not isinstance(frame, torch.Tensor):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise _lib.Y7TError("GMC: the frame must be (H, W, 3) uint8 BGR, got %s %s" % (tuple(frame.shape), frame.dtype))
        frame = frame.cuda().contiguous()
        H, W = int(frame.shape[0]), int(frame.shape[1])
        plane = torch.empty((H // downscale, W // downscale, 4), dtype=torch.float32, device="cuda")
        _lib.check(self._L.y7t_ecc_prepare_u8(_lib.ptr(frame), H, W, int(downscale), _lib.ptr(plane), _lib.stream_ptr()))
        return plane

    def align(self, tmpl, img, max_iters, eps):
        import ctypes
        torch, _lib = self._torch, self._lib
        h, w = int(img.shape[0]), int(img.shape[1])
        if tuple(tmpl.shape) != tuple(img.shape):
            raise _lib.Y7TError("GMC: the frame size changed from %s to %s" % (tuple(tmpl.shape[:2]), (h, w)))
        if (h, w) not in self._ws:
            nb = ctypes.c_size_t()
            _lib.check(self._L.y7t_ecc_workspace_bytes(h, w, ctypes.byref(nb)))
            self._ws[(h, w)] = torch.empty(nb.value // 8 + 1, dtype=torch.float64, device="cuda")
        out = torch.empty(10, dtype=torch.float64, device="cuda")      # the warp, then the status: one copy brings both to the host
        _lib.check(self._L.y7t_ecc_align(_lib.ptr(tmpl), _lib.ptr(img), h, w, MOTION_EUCLIDEAN, int(max_iters), float(eps), _lib.ptr(self._ws[(h, w)]),
                                         _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + 48), _lib.stream_ptr()))
        return out[:6], out[6:]


class _DeviceFeatures:
    """the eleven launches' worth of liby7t.so for method='features': frames, states (keypoints + descriptors of a frame) and the workspace are torch tensors on
    the GPU; nothing is read back"""

    def __init__(self):
        import torch
        from .. import _lib
        _lib.require_gpu()
        self._torch, self._lib, self._L = torch, _lib, _lib.load()
        self._ws = {}
        self._keep = None

    def workspace(self, h, w, cap):
        import ctypes
        if (h, w, cap) not in self._ws:
            nb = ctypes.c_size_t()
            self._lib.check(self._L.y7t_orb_workspace_bytes(h, w, cap, ctypes.byref(nb)))
            self._ws[(h, w, cap)] = self._torch.empty(nb.value // 16 * 16 + 16, dtype=self._torch.uint8, device="cuda")
        return self._ws[(h, w, cap)]

    def _dets(self, dets):
        """-> ((n, 6) float32 device rows or None, n): the count is the shape's, so no copy to the host"""
        torch = self._torch
        if dets is None or len(dets) == 0:
            return None, 0
        if not isinstance(dets, torch.Tensor):
            dets = torch.from_numpy(np.ascontiguousarray(np.asarray(dets, np.float32).reshape(len(dets), -1)))
        rows = torch.zeros((dets.shape[0], 6), dtype=torch.float32, device="cuda")
        c = min(6, int(dets.shape[1]))
        rows[:, :c] = dets[:, :c].to(device="cuda", dtype=torch.float32)
        return rows, int(dets.shape[0])

    def extract(self, frame, downscale, dets, cap, state=None):
        import ctypes
        torch, _lib = self._torch, self._lib
        if not isinstance(frame, torch.Tensor):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise _lib.Y7TError("GMC: the frame must be (H, W, 3) uint8 BGR, got %s %s" % (tuple(frame.shape), frame.dtype))
        frame = frame.cuda().contiguous()
        H, W = int(frame.shape[0]), int(frame.shape[1])
        if state is None:
            nb = ctypes.c_size_t()
            _lib.check(self._L.y7t_orb_state_bytes(cap, ctypes.byref(nb)))
            state = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        rows, n = self._dets(dets)
        _lib.check(self._L.y7t_orb_extract_u8(_lib.ptr(frame), H, W, int(downscale), _lib.ptr(rows) if n else None, n, cap,
                                              _lib.ptr(self.workspace(H // downscale, W // downscale, cap)), _lib.ptr(state), _lib.stream_ptr()))
        self._keep = (frame, rows)      # (alive until the next frame's launches are behind them on the stream)
        return state

    def estimate(self, prev, cur, h, w, downscale, cap):
        import ctypes
        torch, _lib = self._torch, self._lib
        out = torch.empty(12, dtype=torch.float64, device="cuda")      # the warp, then the status: one copy brings both to the host
        _lib.check(self._L.y7t_orb_estimate(_lib.ptr(prev), _lib.ptr(cur), h, w, int(downscale), cap, _lib.ptr(self.workspace(h, w, cap)), _lib.ptr(out),
                                            ctypes.c_void_p(out.data_ptr() + 48), _lib.stream_ptr()))
        return out[:6], out[6:]


FEATURE_WARNINGS = {2: 'Warning: not enough matching points',                        # botsort.py:228 (Y7T_ORB_STATUS_NOT_ENOUGH)
                    3: 'Warning: find transform failed. Set warp as identity'}       # no hypothesis with two inliers (Y7T_ORB_STATUS_NO_MODEL)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


class GMC:
    """GMC(method='ecc', downscale=2, verbose=None) of the reference, plus `faithful`.

    apply(raw_frame, detections=None) -> (2, 3) float64 ndarray, the warp from the template frame's coordinates to this frame's; identity for the first
    frame and when the alignment fails (the reference's warning text is printed then).  raw_frame: (H, W, 3) uint8 BGR as a NumPy array or a host or
    device tensor.  apply_device(frame) -> the same warp as a (6,) float64 DEVICE tensor, enqueued on the current stream with no host round trip (so no
    warning either; `last_status` keeps {iterations, flag, rho, |rho - rho_last|} on the device).

    faithful=True (default) keeps two quirks of the reference's applyEcc:
      * prevFrame is never replaced after the first frame (botsort.py:92-100), so EVERY frame is aligned to frame 0;
      * the translation is not multiplied by `downscale` (applyFeaures does, botsort.py:224-226; applyEcc does not), so it is in half-resolution pixels.
    faithful=False aligns each frame to the previous one and rescales the translation to full-resolution pixels -- what upstream BoT-SORT does and what
    moving-camera footage needs.

    method='features' (the reference's applyFeaures; `faithful`, `max_iters` and `eps` do not apply): every frame is matched against the previous one, the boxes
    of `detections` ((n, >= 4) tlbr rows in full-resolution pixels, a NumPy array or a host or device tensor) are masked out of the corners, at most
    `max_keypoints` corners are kept (the first in row-major order), and the translation is in full-resolution pixels (botsort.py:224-226).  The identity comes
    back for the first frame, with fewer than 2 current or no previous keypoints, with 4 good matches or fewer (apply prints the reference's warning) and when no
    hypothesis has two inliers.  `last_status` keeps {n_prev, n_cur, good matches, inliers, flag, truncated} on the device.

    method='none' returns the identity; 'orb', 'sift' and 'file' raise NotImplementedError.  max_iters / eps: the reference's criteria (100, 1e-5).
    backend: an object with prepare(frame, downscale) and align(tmpl, img, max_iters, eps) -- for 'features' with extract(frame, downscale, dets, cap, state) and
    estimate(prev, cur, h, w, downscale, cap) -- (tests run the host build of the kernels through it)."""

    def __init__(self, method='ecc', downscale=2, verbose=None, faithful=True, max_iters=100, eps=1e-5, backend=None, max_keypoints=8192):
        if method in ('none', 'None'):
            method = 'none'
        elif method in ('orb', 'sift', 'file', 'files'):
            raise NotImplementedError("GMC method %r: only 'ecc' and 'none' are in scope of the device path (ORB / SIFT matching and the "
                                      "MOTChallenge GMC files are not)" % (method,))
        elif method not in ('ecc', 'features'):
            raise ValueError("Error: Unknown CMC method:" + str(method))      # botsort.py:58
        self.method = method
        self.downscale = max(1, int(downscale))
        self.faithful = bool(faithful)
        self.max_iters, self.eps = int(max_iters), float(eps)
        self.max_keypoints = int(max_keypoints)
        self._backend = backend if backend is not None else (_DeviceEcc() if method == 'ecc' else _DeviceFeatures() if method == 'features' else None)
        self._states, self._frames, self._size = [None, None], 0, None      # 'features': the previous and the current state, double buffered
        self.prevFrame = None               # the template PLANE ({I, gx, gy} per pixel), not the gray frame
        self.initializedFirstFrame = False
        self.last_status = None
        self._keep = None

    def _estimate_features(self, raw_frame, detections):
        H, W = int(raw_frame.shape[0]), int(raw_frame.shape[1])
        if self._size not in (None, (H, W)):
            raise ValueError("GMC: the frame size changed from %s to %s" % (self._size, (H, W)))
        self._size = (H, W)
        slot = self._frames & 1      # (the state of two frames ago is overwritten: its estimate is behind this extraction on the stream)
        cur = self._states[slot] = self._backend.extract(raw_frame, self.downscale, detections, self.max_keypoints, self._states[slot])
        self._frames += 1
        if not self.initializedFirstFrame:
            self.initializedFirstFrame = True
            self.prevFrame = cur
            return None
        warp, status = self._backend.estimate(self._states[slot ^ 1], cur, H // self.downscale, W // self.downscale, self.downscale, self.max_keypoints)
        self.prevFrame = cur
        self.last_status = status
        return warp, status

    def _estimate(self, raw_frame, detections=None):
        """-> (warp (6,), status) in the backend's memory, or None for the first frame"""
        if self.method == 'features':
            return self._estimate_features(raw_frame, detections)
        plane = self._backend.prepare(raw_frame, self.downscale)
        if not self.initializedFirstFrame:
            self.prevFrame = plane
            self.initializedFirstFrame = True
            return None
        warp, status = self._backend.align(self.prevFrame, plane, self.max_iters, self.eps)
        self._keep = (self.prevFrame, plane)      # (alive until the next frame's launches are behind them on the stream)
        if not self.faithful:
            self.prevFrame = plane
            if self.downscale > 1:
                scale = np.array([1.0, 1.0, self.downscale, 1.0, 1.0, self.downscale])
                warp = warp * (scale if isinstance(warp, np.ndarray) else warp.new_tensor(scale))
        self.last_status = status
        return warp, status

    def apply(self, raw_frame, detections=None):
        if self.method == 'none':
            return np.eye(2, 3)
        r = self._estimate(raw_frame, detections)
        if r is None:
            return np.eye(2, 3)
        warp, status = r
        if isinstance(warp, np.ndarray):
            both = np.concatenate([warp, status])
        else:
            import torch
            both = torch.cat([warp, status]).cpu().numpy()      # one copy for the matrix and the flag
        if self.method == 'features':
            if int(both[10]) in FEATURE_WARNINGS:
                print(FEATURE_WARNINGS[int(both[10])])
        elif int(both[7]) == FAILED:
            print('Warning: find transform failed. Set warp as identity')      # botsort.py:107
        return both[:6].reshape(2, 3).astype(np.float64)

    def apply_device(self, raw_frame, detections=None):
        eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        if self.method == 'none':
            import torch
            return torch.tensor(eye, dtype=torch.float64, device="cuda")
        r = self._estimate(raw_frame, detections)
        if r is not None:
            return r[0]
        if isinstance(self.prevFrame, np.ndarray):      # (a host backend)
            return np.array(eye)
        import torch
        return torch.tensor(eye, dtype=torch.float64, device=self.prevFrame.device)
