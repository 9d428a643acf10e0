"""tests/_hostsim/ecc.py -- TEST INFRASTRUCTURE ONLY: the ECC kernel bodies of csrc/y7t_ecc.h of the host build -- the per-pixel programs of the prepare and the
iteration launch one "lane" at a time, the slab combine and the 3x3 solve, with the device's reduction order -- so that the camera-motion estimate can be tested
without a GPU."""
import ctypes

import numpy as np

from tests._hostsim import build_ecc

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_ecc())
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.hs_ecc_ws_bytes.restype = ctypes.c_size_t
        L.hs_ecc_ws_bytes.argtypes = [ci, ci]
        L.hs_ecc_num_wg.argtypes = [ci, ci]
        L.hs_ecc_prepare.argtypes = [vp, ci, ci, ci, vp]
        L.hs_ecc_sums.argtypes = [vp, vp, ci, ci, cd, cd, cd, vp]
        L.hs_ecc_align.argtypes = [vp, vp, ci, ci, ci, cd, vp, vp]
        L.hs_ecc_solve.argtypes = [vp, vp, vp]
        L.hs_ecc_sincos.argtypes = [cd, vp]
        L.hs_ecc_principal.restype = cd
        L.hs_ecc_principal.argtypes = [cd]
        assert L.hs_ecc_pix_bytes() == 16
        _lib = L
    return _lib


def num_wg(h, w):
    return lib().hs_ecc_num_wg(h, w)


def prepare(bgr, downscale=2):
    """(H, W, 3) uint8 BGR -> (h, w, 4) float32 plane {I, gx, gy, 0}"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    H, W = bgr.shape[:2]
    plane = np.zeros((H // downscale, W // downscale, 4), np.float32)
    lib().hs_ecc_prepare(bgr.ctypes.data, H, W, int(downscale), plane.ctypes.data)
    return plane


def _planes(tmpl, img):
    tmpl, img = np.ascontiguousarray(tmpl, np.float32), np.ascontiguousarray(img, np.float32)
    assert tmpl.shape == img.shape and tmpl.ndim == 3 and tmpl.shape[2] == 4
    return tmpl, img


def sums(tmpl, img, p):
    """the 21 combined sums of one iteration at p = (theta, tx, ty)"""
    tmpl, img = _planes(tmpl, img)
    out = np.zeros(21, np.float64)
    lib().hs_ecc_sums(tmpl.ctypes.data, img.ctypes.data, tmpl.shape[0], tmpl.shape[1], float(p[0]), float(p[1]), float(p[2]), out.ctypes.data)
    return out


def align(tmpl, img, max_iters=100, eps=1e-5):
    """-> (warp (6,) float64, status (4,) float64 = iterations, flag, rho, |rho - rho_last|)"""
    tmpl, img = _planes(tmpl, img)
    warp, status = np.zeros(6, np.float64), np.zeros(4, np.float64)
    lib().hs_ecc_align(tmpl.ctypes.data, img.ctypes.data, tmpl.shape[0], tmpl.shape[1], int(max_iters), float(eps), warp.ctypes.data, status.ctypes.data)
    return warp, status


def solve(sums21, p=(0.0, 0.0, 0.0), rho=-1.0, rho_last=0.0):
    """the 3x3 solve of one iteration -> (p, rho, flag)"""
    S = np.ascontiguousarray(sums21, np.float64)
    state = np.array(list(p) + [rho, rho_last], np.float64)
    it = np.zeros(2, np.int32)
    lib().hs_ecc_solve(S.ctypes.data, state.ctypes.data, it.ctypes.data)
    return state[:3].copy(), float(state[3]), int(it[1])


def sincos(th):
    sc = np.zeros(2, np.float64)
    lib().hs_ecc_sincos(float(th), sc.ctypes.data)
    return sc[0], sc[1]


class HostEcc:
    """the estimator's backend on the host: what tracker/gmc.py's device backend does through liby7t.so (the `backend=` seam of GMC)"""

    def prepare(self, frame, downscale):
        if hasattr(frame, "cpu"):
            frame = frame.cpu().numpy()
        return prepare(frame, downscale)

    def align(self, tmpl, img, max_iters, eps):
        return align(tmpl, img, max_iters, eps)
