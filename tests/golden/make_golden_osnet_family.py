"""tests/golden/make_golden_osnet_family.py -- regenerates the committed fixtures of the OSNet family (osnet_family_<name>.npz).

Runs ONLY in the build container (needs the reference sources): it imports the reference's own tracker/reid_models/OSNet.py through oracle/ref_harness.py,
constructs its osnet_x0_25, osnet_x0_5, osnet_x0_75, osnet_x1_0 and osnet_ibn_x1_0 with num_classes=1, pretrained=False, puts them in .eval().double(), loads
the seeded state dict of tracker/reid.py::random_state_dict (weights are never stored: only the seed and a digest of the state dict) and records the module's
float64 embeddings of seeded crops: 3 of 32 x 16, 2 of 16 x 16 and 1 of 128 x 64 (H x W; NHWC float32, already "resized and normalised").

    python tests/golden/make_golden_osnet_family.py
"""
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from yolov7_tracker_amd.tracker import reid  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 11
CROP_SETS = [("a", 3, 32, 16), ("b", 2, 16, 16), ("c", 1, 128, 64)]        # key, crops, H, W


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].numpy()).tobytes())
    return h.hexdigest()


def crops(key, n, H, W):
    rng = np.random.default_rng([SEED, ord(key)])
    return rng.normal(0.0, 1.0, (n, H, W, 3)).astype(np.float32)


def load_reference():
    with ref_harness._patched_modules([os.path.join(ref_harness.REF_ROOT, "tracker", "reid_models")]):
        sys.modules.pop("OSNet", None)
        mod = importlib.import_module("OSNet")
        sys.modules.pop("OSNet", None)
    return mod


def main():
    mod = load_reference()
    for name, (width, ibn) in reid.OSNET_NAMES.items():
        spec = reid.osnet_spec(width, ibn=ibn)
        sd = reid.random_state_dict(spec, SEED)
        net = getattr(mod, name)(num_classes=1, pretrained=False)
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        assert all(k.startswith("classifier.") or k.endswith("num_batches_tracked") for k in missing), missing
        net = net.eval().double()
        out = {"seed": np.int64(SEED), "digest": np.array(digest(sd)), "width": np.float64(width), "ibn": np.bool_(ibn)}
        with torch.no_grad():
            for key, n, H, W in CROP_SETS:
                x = crops(key, n, H, W)
                out["crops_" + key] = x
                out["emb_" + key] = net(torch.from_numpy(x).double().permute(0, 3, 1, 2)).numpy()
                assert out["emb_" + key].shape == (n, 512) and out["emb_" + key].dtype == np.float64
        path = os.path.join(HERE, "osnet_family_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%s: %d bytes, |emb| %.3f" % (path, os.path.getsize(path), float(np.abs(out["emb_c"]).mean())))


if __name__ == "__main__":
    main()
