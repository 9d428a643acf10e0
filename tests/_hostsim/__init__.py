"""tests/_hostsim -- TEST INFRASTRUCTURE ONLY: CPU builds (g++, -ffp-contract=off) of device code, so that its control flow and pinned arithmetic can be
tested without a GPU.  Never imported by the product package.

  liby7t_hostsim*.so  (y7t_hostsim.cpp)      the portable tracker workgroup programs of csrc/y7t_track_*.h at nt = 1, every tracker kind: bound here (`lib()`);
                                              HostSimTracker below, HostStrongSORT in strongsort.py, HostDeepMOT in deepmot.py
  liby7t_hostsim_ecc.so (y7t_hostsim_ecc.cpp) the ECC kernel bodies of csrc/y7t_ecc.h (they share no code with the tracker programs): bound in ecc.py

Y7T_HOSTSIM_DEFS="-DY7T_NEXT_TRACKER=1": a second tracker library with experimental macros of the headers switched on (the tests then run against it).
Y7T_HOSTSIM_FAST_BYTES: the workgroup's fast scratch -- 131072 bytes by default, like the device's LDS budget (csrc/y7t_tracker.hip: kFastBytes), so the placement
branches taken here are the ones the GPU takes; 0 runs everything out of the state blob (the other branches), any other value sizes it."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "yolov7-tracker_amd", "csrc")
_DEFS = os.environ.get("Y7T_HOSTSIM_DEFS", "").split()
_SO = os.path.join(_HERE, "liby7t_hostsim%s.so" % ("_" + "".join(c for c in "".join(_DEFS) if c.isalnum()) if _DEFS else ""))
_SO_ECC = os.path.join(_HERE, "liby7t_hostsim_ecc.so")
FAST_BYTES = 131072


def _build(so, src, defs=(), force=False):
    """compile tests/_hostsim/<src> into <so> when it is older than the source or any header of csrc/ (a hand-kept list would miss a new one)"""
    src = os.path.join(_HERE, src)
    deps = [src] + [os.path.join(_CSRC, h) for h in os.listdir(_CSRC) if h.endswith(".h")]
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"] + list(defs) + ["-o", so, src])
    return so


def reset_fast_bytes():
    """the fast scratch back to what the environment asks for (after a test that ran with another size)"""
    ctypes.CDLL(_SO).hs_set_fast_bytes(int(os.environ.get("Y7T_HOSTSIM_FAST_BYTES", str(FAST_BYTES))))


def build_ecc(force=False):
    return _build(_SO_ECC, "y7t_hostsim_ecc.cpp", force=force)


def build(force=False):
    """both libraries -> the path of the tracker programs'"""
    build_ecc(force)
    _build(_SO, "y7t_hostsim.cpp", _DEFS, force)
    reset_fast_bytes()
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, ci, cd, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
        L.hs_tracker_bytes.restype = sz
        L.hs_tracker_bytes.argtypes = [ci, ci]
        L.hs_tracker_init.argtypes = [vp] + [ci] * 6 + [cd] * 3 + [vp]
        L.hs_tracker_step.argtypes = [vp, vp, ci, vp, ci, vp]
        L.hs_kf_gmc.argtypes = [vp, vp, vp]
        L.hs_tracker_status.argtypes = [vp]
        L.hs_arena_begin.argtypes = [vp]
        L.hs_arena_end.argtypes = [vp]
        L.hs_lapjv.argtypes = [vp, ci, ci, cd, vp, vp]
        L.hs_lapsap.argtypes = L.hs_lapjv.argtypes
        L.hs_laplit.argtypes = L.hs_lapjv.argtypes
        L.hs_iou_cost.argtypes = [vp, ci, vp, ci, vp]
        L.hs_kf_initiate.argtypes = [ci, vp, ci, vp, vp]
        L.hs_kf_predict.argtypes = [ci, vp, vp]
        L.hs_kf_update.argtypes = [ci, vp, vp, vp, cd]
        L.hs_kf_project.argtypes = [ci, vp, vp, cd, vp, vp]
        L.hs_kf_gating.argtypes = [ci, vp, vp, vp, ci]
        L.hs_kf_gating.restype = cd
        L.hs_pyset_difference.argtypes = [ci, vp, ci, vp]
        # DeepSORT
        L.hs_feat_bytes.restype = sz
        L.hs_feat_bytes.argtypes = [ci] * 4
        L.hs_feat_init.argtypes = [vp] + [ci] * 4
        L.hs_deepsort_step.argtypes = [vp, vp, vp, ci, vp, vp, ci]
        L.hs_feat_status.argtypes = [vp]
        L.hs_np_pairwise_sumsq.restype = ctypes.c_float
        L.hs_np_pairwise_sumsq.argtypes = [vp, ci]
        L.hs_blas_sdot_self.restype = ctypes.c_float
        L.hs_blas_sdot_self.argtypes = [vp, ci]
        L.hs_feat_store.argtypes = [vp, vp, ci, ci]
        L.hs_feat_normalize.argtypes = [vp, ci, ci, vp]
        # StrongSORT
        L.hs_ss_feat_bytes.restype = sz
        L.hs_ss_feat_bytes.argtypes = [ci, ci, ci]
        L.hs_ss_feat_init.argtypes = [vp, ci, ci, ci, cd]
        L.hs_strongsort_step.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp]
        L.hs_strongsort_predict.argtypes = [vp, vp, ci]
        L.hs_ss_feat_status.argtypes = [vp]
        L.hs_ss_vec_offset.restype = sz
        L.hs_ss_vec_offset.argtypes = [ci, ci, ci]
        L.hs_ss_cdist.argtypes = [vp, ci, vp, ci, ci, vp]
        L.hs_ss_ema.argtypes = [vp, vp, ci]
        L.hs_ss_fuse.restype = cd
        L.hs_ss_fuse.argtypes = [cd, cd, cd]
        # DeepMOT
        L.hs_deepmot_front.argtypes = [vp, vp, ci, ci, ci, vp, ctypes.c_longlong]
        L.hs_deepmot_back.argtypes = [vp, vp, vp, ctypes.c_uint, vp, ci]
        L.hs_dm_ecu_iou.restype = cd
        L.hs_dm_ecu_iou.argtypes = [vp, vp, cd, ci, ci]
        _lib = L
    return _lib


def pyset_difference(n, matched):
    """order of `list(set(range(n)) - set(matched))` as the device program emulates it"""
    member = np.zeros(max(n, 1), np.int32)
    member[list(matched)] = 1
    out = np.zeros(max(n, 1), np.int32)
    c = lib().hs_pyset_difference(n, member.ctypes.data, len(set(matched)), out.ctypes.data)
    assert c >= 0
    return out[:c].tolist()


def np_pairwise_sumsq(x):
    """y7t_np_pairwise_sumsq of a float32 vector (np.linalg.norm(axis=1)'s sum, before the sqrt) -> np.float32"""
    x = np.ascontiguousarray(x, np.float32)
    return np.float32(lib().hs_np_pairwise_sumsq(x.ctypes.data, x.size))


def blas_sdot_self(x):
    """y7t_blas_sdot_self of a float32 vector (the 1-D np.linalg.norm's sum, before the sqrt) -> np.float32"""
    x = np.ascontiguousarray(x, np.float32)
    return np.float32(lib().hs_blas_sdot_self(x.ctypes.data, x.size))


def feat_store(src, update):
    """y7t_feat_store: the ring row a raw appearance vector becomes (update: STrack.update's f / norm(f) first)"""
    src = np.ascontiguousarray(src, np.float32)
    dst = np.empty_like(src)
    lib().hs_feat_store(dst.ctypes.data, src.ctypes.data, src.size, int(bool(update)))
    return dst


def feat_normalize(feats):
    """y7t_feat_normalize_dets: the (n, dim) detection features of a frame, every row divided by its norm"""
    feats = np.ascontiguousarray(feats, np.float32)
    out = np.empty_like(feats)
    if len(feats):
        lib().hs_feat_normalize(feats.ctypes.data, feats.shape[0], feats.shape[1], out.ctypes.data)
    return out


def lapjv(cost, limit, sap=False, literal=False):
    """JV on lap's implicit extended matrix (sap=False), the reduced shortest-augmenting-path solver with its tie fallback (sap=True), or
    lapjv.cpp run literally (literal=True)"""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    x = np.empty(max(nr, 1), np.int32)
    y = np.empty(max(nc, 1), np.int32)
    if nr and nc:
        (lib().hs_laplit if literal else lib().hs_lapsap if sap else lib().hs_lapjv)(cost.ctypes.data, nr, nc, float(limit), x.ctypes.data, y.ctypes.data)
    else:
        x[:] = -1
        y[:] = -1
    return x[:nr].copy(), y[:nc].copy()


class HostSimTracker:
    TRACKERS = {"sort": 0, "bytetrack": 1, "botsort": 2, "deepsort": 3, "c_biou": 4, "uavmot": 5, "strongsort": 6, "deepmot": 7}      # include/y7t.h: Y7T_TRACKER_<NAME>
    KINDS = {"default": 0, "naive": 1, "botsort": 2, "strongsort": 3}

    def __init__(self, kind="bytetrack", conf_thresh=0.2, track_buffer=30, kalman_format="default", iou_thresh=0.5,
                 frame_rate=30, cap_t=1024, cap_d=1024, ids=None, f32_quirk=1, feature_fn=None, feat_dim=128, feat_budget=100):
        self.ids = ids if ids is not None else np.zeros(1, np.int32)
        n = lib().hs_tracker_bytes(cap_t, cap_d)
        self.blob = np.zeros(n, np.uint8)
        self.cap_t, self.cap_d = cap_t, cap_d
        lib().hs_tracker_init(self.blob.ctypes.data, self.TRACKERS[kind], self.KINDS[kalman_format], cap_t, cap_d,
                              int(frame_rate / 30.0 * track_buffer), f32_quirk, conf_thresh, max(0.15, conf_thresh - 0.3),
                              iou_thresh, self.ids.ctypes.data)
        self.out = np.zeros((cap_t, 8), np.float64)
        self.kind, self.feature_fn, self.feat_dim = kind, feature_fn, feat_dim
        if kind == "deepsort":
            self.fblob = np.zeros(lib().hs_feat_bytes(cap_t, cap_d, feat_dim, feat_budget), np.uint8)
            lib().hs_feat_init(self.fblob.ctypes.data, cap_t, cap_d, feat_dim, feat_budget)

    def update(self, det, warp=None):
        if self.kind == "deepsort" and det is not None:
            det = np.ascontiguousarray(det, dtype=np.float32).reshape(-1, 6)
            feats = np.zeros((max(len(det), 1), self.feat_dim), np.float32)
            if len(det):
                feats[:len(det)] = self.feature_fn(det[:, :4])     # (the reference extracts them for the rows above det_thresh only)
            cnt = lib().hs_deepsort_step(self.blob.ctypes.data, self.fblob.ctypes.data, det.ctypes.data, det.shape[0], feats.ctypes.data,
                                         self.out.ctypes.data, self.cap_t)
            if lib().hs_tracker_status(self.blob.ctypes.data) or lib().hs_feat_status(self.fblob.ctypes.data):
                raise RuntimeError("tracker capacity exceeded")
            return [(int(r[0]), r[1:5].copy(), float(r[5]), float(r[6])) for r in self.out[:cnt]]
        wp = None
        if warp is not None:
            self._warp = np.ascontiguousarray(warp, dtype=np.float64).reshape(6)
            wp = self._warp.ctypes.data
        if det is None:
            n, ptr = -1, None
        else:
            det = np.ascontiguousarray(det, dtype=np.float32).reshape(-1, 6)
            n, ptr = det.shape[0], det.ctypes.data
        cnt = lib().hs_tracker_step(self.blob.ctypes.data, ptr, n, self.out.ctypes.data, self.cap_t, wp)
        st = lib().hs_tracker_status(self.blob.ctypes.data)
        if st:
            raise RuntimeError("tracker capacity exceeded (status %d)" % st)
        return [(int(r[0]), r[1:5].copy(), float(r[5]), float(r[6])) for r in self.out[:cnt]]


def run(kind, dets_per_frame, warps=None, arena_frames=0, **kw):
    """arena_frames > 0: the frames run in groups of that many with the index lists in the launch-long arena (y7t_arena_load ... frames ... y7t_arena_store),
    like the frames of one k_tracker_step_frames launch on the device"""
    trk = HostSimTracker(kind, **kw)
    out = []
    for i, d in enumerate(dets_per_frame):
        if arena_frames and i % arena_frames == 0:
            assert lib().hs_arena_begin(trk.blob.ctypes.data)
        out.append(trk.update(d, None if warps is None else warps[i]))
        if arena_frames and (i % arena_frames == arena_frames - 1 or i == len(dets_per_frame) - 1):
            lib().hs_arena_end(trk.blob.ctypes.data)
    return out
