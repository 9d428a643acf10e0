"""DeepMOT (/root/reference/tracker/deepmot.py:143-324, "How to train your deep multi-object tracker") on the device track pool: ByteTrack whose first
association solves 1 - DHN(D) at 0.9, where D = matching.ecu_iou_distance(strack_pool, D_high, image shape) cast to float32 and DHN is the Deep Hungarian
Net (class Munkrs, deepmot.py:10-140): two stacked bidirectional 2-layer GRUs of hidden size 256 over the matrix flattened row-major, then column-major,
three linear layers and a sigmoid.  A frame is the front program, the network's launches and the back program of liby7t.so (y7t_tracker_step_deepmot;
csrc/y7t_track_deepmot.h, csrc/y7t_dhn.hip).

Deviations from the reference, both stated in DESIGN.md: the network runs in eval() mode (the reference never calls .eval(), so the 0.2 dropout between its GRU
layers is live and its output is random from call to call), and it runs on the device whatever `is_cuda` says.

The reference's quirk is kept: the second association's unmatched indices, which point into the still-Tracked leftovers of the first, are applied to
strack_pool (deepmot.py:269-272).

opts.dhn_path: a file that torch.load reads as a Munkrs state dict (keys and shapes are checked), or `random:dhn[:seed[:scale]]` for the seeded weights of
synth.make_dhn_weights (no DHN.pth ships with the reference).  `ori_img` supplies shape[:2] only."""
import weakref

import numpy as np
import torch

from .. import _lib, synth
from .basetrack import BaseTracker, STrack, TrackState, joint_stracks, sub_stracks, remove_duplicate_stracks  # noqa: F401


def load_dhn_weights(path):
    """opts.dhn_path -> {name: float32 numpy array} in Munkrs.state_dict() order"""
    shapes = synth.dhn_tensor_shapes()
    if isinstance(path, str) and path.startswith("random"):
        parts = path.split(":")
        if len(parts) < 2 or parts[1] != "dhn" or len(parts) > 4:
            raise ValueError("dhn_path %r: random:dhn[:seed[:scale]]" % (path,))
        seed = int(parts[2]) if len(parts) > 2 and parts[2] else 0
        scale = float(parts[3]) if len(parts) > 3 and parts[3] else 1.0
        return synth.make_dhn_weights(seed, scale)
    sd = torch.load(path, map_location="cpu")
    if hasattr(sd, "state_dict"):
        sd = sd.state_dict()
    if not isinstance(sd, dict):
        raise ValueError("dhn_path %r does not hold a state dict" % (path,))
    sd = {k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}
    missing = [n for n, _ in shapes if n not in sd]
    extra = [k for k in sd if k not in dict(shapes)]
    if missing or extra:
        raise ValueError("dhn_path %r is not a Munkrs state dict: missing %s, unexpected %s" % (path, missing[:4], extra[:4]))
    out = {}
    for name, shape in shapes:
        a = torch.as_tensor(sd[name]).detach().cpu().to(torch.float32).numpy()
        if tuple(a.shape) != tuple(shape):
            raise ValueError("dhn_path %r: %s has shape %s, expected %s" % (path, name, tuple(a.shape), tuple(shape)))
        out[name] = np.ascontiguousarray(a)
    return out


def pack_dhn_weights(weights):
    """the 38 tensors -> one float32 vector in state_dict() order (what y7t_dhn_init takes)"""
    return np.concatenate([np.asarray(weights[n], np.float32).reshape(-1) for n, _ in synth.dhn_tensor_shapes()])


class TorchDHN(torch.nn.Module):
    """The network as a torch module (eval mode, any device / dtype): what the device kernels are checked against, and what a host without a GPU evaluates.
    forward(D (h, w)) -> (h, w) sigmoid output."""

    def __init__(self, weights):
        super().__init__()
        self.lstm_row = torch.nn.GRU(1, 256, num_layers=2, bidirectional=True)
        self.lstm_col = torch.nn.GRU(512, 256, num_layers=2, bidirectional=True)
        self.hidden2tag_1 = torch.nn.Linear(512, 256)
        self.hidden2tag_2 = torch.nn.Linear(256, 64)
        self.hidden2tag_3 = torch.nn.Linear(64, 1)
        self.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in weights.items()})
        self.eval()

    @torch.no_grad()
    def forward(self, D):
        h, w = D.shape
        rows, _ = self.lstm_row(D.reshape(h * w, 1, 1))                                        # row-major sequence
        cols, _ = self.lstm_col(rows.reshape(h, w, 512).transpose(0, 1).reshape(h * w, 1, 512))  # column-major sequence
        y = cols.reshape(w, h, 512).transpose(0, 1).reshape(h * w, 512)
        return torch.sigmoid(self.hidden2tag_3(self.hidden2tag_2(self.hidden2tag_1(y)))).reshape(h, w)


class DeviceDHN:
    """The network on the device: the weights and the workspace for matrices of up to max_h x max_w.  Trackers may share one object."""

    def __init__(self, weights, max_h=128, max_w=128):
        _lib.require_gpu()
        self._L = _lib.load()
        self.max_h, self.max_w = int(max_h), int(max_w)
        nbytes = int(self._L.y7t_dhn_weight_bytes()) + int(self._L.y7t_dhn_workspace_bytes(self.max_h, self.max_w))
        packed = pack_dhn_weights(weights)
        if packed.size != int(self._L.y7t_dhn_num_weights()):
            raise ValueError("%d weights, the network has %d" % (packed.size, int(self._L.y7t_dhn_num_weights())))
        self._blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        weakref.finalize(self._blob, DeviceDHN._release, self._L, int(self._blob.data_ptr()))
        _lib.check(self._L.y7t_dhn_init(_lib.ptr(self._blob), nbytes, packed.ctypes.data, self.max_h, self.max_w, _lib.stream_ptr()))

    @staticmethod
    def _release(L, address):
        try:
            L.y7t_dhn_release(address)
        except Exception:
            pass

    @property
    def ptr(self):
        return _lib.ptr(self._blob)

    def forward(self, D):
        """(h, w) float32 (numpy or tensor) -> (h, w) float32 device tensor"""
        d = torch.as_tensor(D).to(device="cuda", dtype=torch.float32).contiguous()
        h, w = d.shape
        out = torch.empty((h, w), dtype=torch.float32, device="cuda")
        _lib.check(self._L.y7t_dhn_forward_f32(self.ptr, _lib.ptr(d), h, w, _lib.ptr(out), _lib.stream_ptr()))
        return out

    __call__ = forward


class DeepMOT(BaseTracker):
    """deepmot.py:143-324.  opts: conf_thresh, track_buffer, kalman_format, img_size, dhn_path (+ the optional capacities of BaseTracker and dhn_max_tracks /
    dhn_max_dets, the largest pool x high-detection matrix the network's workspace is sized for: 256 x 128 = 32768 positions by default, 128 MiB).  dhn: a DeviceDHN to share."""
    _KIND = 7  # Y7T_TRACKER_DEEPMOT

    def __init__(self, opts, frame_rate=30, *args, dhn=None, **kwargs):
        super().__init__(opts, frame_rate=frame_rate)
        if dhn is None:
            path = getattr(opts, "dhn_path", None)
            if not path:
                raise _lib.Y7TError("DeepMOT needs opts.dhn_path: a Munkrs state dict file, or random:dhn[:seed[:scale]]")
            dhn = DeviceDHN(load_dhn_weights(path), min(self.cap_t, int(getattr(opts, "dhn_max_tracks", 256))), min(self.cap_d, int(getattr(opts, "dhn_max_dets", 128))))
        self.DHN = dhn
        self.low_conf_thresh = max(0.15, self.opts.conf_thresh - 0.3)
        self.filter_small_area = False
        self.use_apperance_model = False

    def _launch(self, det_results, out=None, img_shape=None, **kw):
        if det_results is None:
            return super()._launch(None, out=out)
        if img_shape is None:
            raise _lib.Y7TError("DeepMOT._launch needs img_shape=(h, w) of the frame (matching.ecu_iou_distance normalises by its diagonal)")
        d = det_results.detach() if isinstance(det_results, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(det_results, dtype=np.float32))
        d = d.to(device="cuda", dtype=torch.float32).contiguous().reshape(-1, 6)
        n = d.shape[0]
        if n > self.cap_d:
            raise _lib.Y7TError("%d detections exceed the pool capacity max_dets=%d" % (n, self.cap_d))
        self._det_keep = d
        optr, cptr = self._out_ptrs(out)
        self.frame_id += 1
        self._snap_cache = None
        _lib.check(self._L.y7t_tracker_step_deepmot(_lib.ptr(self._state), self.DHN.ptr, _lib.ptr(d), n, int(img_shape[0]), int(img_shape[1]), optr, self.cap_t, cptr,
                                                    self.threads, _lib.stream_ptr()))

    def update(self, det_results, ori_img=None):
        """(N,6) [x1,y1,x2,y2,conf,cls] + the frame (its shape[:2] is all that is read) -> list of tracks (deepmot.py:161-324)"""
        if ori_img is None:
            raise _lib.Y7TError("DeepMOT.update needs the frame (ori_img.shape[:2] normalises the centre distance)")
        self._launch(det_results, img_shape=tuple(ori_img.shape[:2]))
        return self._collect()
