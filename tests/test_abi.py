"""CPU: liby7t.so builds for gfx950, loads, and exports every symbol include/y7t.h declares (no compute calls --
there is no GPU here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from yolov7_tracker_amd import build, _lib
    build.build()
    return _lib.load()


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "y7t.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(y7t_[a-z0-9_]+)\s*\(", txt)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from yolov7_tracker_amd import _lib
    syms = header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), "liby7t.so does not export %s" % s
        assert s in _lib.SIGNATURES, "no ctypes signature for %s" % s
    for s in _lib.SIGNATURES:
        assert s in syms, "%s bound in _lib.py but not declared in include/y7t.h" % s


def test_hostsim_tracker_kinds_are_the_header_enumerators():
    """the names by which the host build (tests/_hostsim) selects a tracker program are the Y7T_TRACKER_* enumerators of include/y7t.h, by value"""
    from tests._hostsim import HostSimTracker
    txt = open(os.path.join(ROOT, "include", "y7t.h")).read()
    enum = {name.lower(): int(v) for name, v in re.findall(r"\bY7T_TRACKER_([A-Z_]+)\s*=\s*(\d+)", txt)}
    assert len(enum) == 8 and HostSimTracker.TRACKERS == enum


def test_version_and_error_string(lib):
    assert lib.y7t_version() >= 100
    assert isinstance(lib.y7t_last_error(), bytes)


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import types
    from yolov7_tracker_amd import _lib
    from yolov7_tracker_amd.tracker.bytetrack import ByteTrack
    with pytest.raises(_lib.Y7TError):
        ByteTrack(types.SimpleNamespace(conf_thresh=0.2, track_buffer=30, kalman_format="default", img_size=1280, iou_thresh=0.5))


def test_product_never_imports_oracle():
    """the oracle is test infrastructure: nothing under yolov7-tracker_amd/ may reference it."""
    pkg = os.path.join(ROOT, "yolov7-tracker_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)
                assert "_hostsim" not in txt or f.endswith((".h",)), os.path.join(dp, f)


def test_integration_doc_shows_every_entry_point():
    """INTEGRATION.md is where a maintainer of the reference finds the binding for each C entry point: none may be missing"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    syms = sorted(set(re.findall(r"\b(y7t_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "y7t.h")).read())))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert len(syms) >= 40 and not [s for s in syms if s not in doc]


def _strings(path):
    import re
    data = open(path, "rb").read()
    return [m.group().decode() for m in re.finditer(rb"[\x20-\x7e]{8,}", data)]


def test_the_product_library_carries_no_ablation_or_variant_instance():
    """lib/liby7t.so = the measured defaults only.  The timing-ablation instances ("wrong results": ABL template arguments of the weights-stationary,
    LDS-patch and ping-pong kernels), the tile / ring variants of the generic kernel (Y7T_CONV_VARIANT) and the code that reads experiment switches from the
    environment exist only in lib/liby7t_ablate.so (the same sources with -DY7T_ABLATE_BUILD; Y7T_LIB=<path>).  Checked on the kernel names the HIP runtime registers."""
    import re
    from yolov7_tracker_amd import build
    build.build()
    prod, abl = _strings(build.LIB), _strings(build.LIB_ABLATE)
    ablated = [r"k_conv3x3_c64_wsILi\dELi[1-9]", r"k_conv3x3_patchILi\d+ELi\d+ELi\d+ELi[1-9]", r"k_conv1x1_p8ILi\dELb[01]ELi[1-9]",
               r"k_conv_igemmILi256ELi256", r"k_conv_igemmILi128ELi128ELi64ELi3", r"k_conv_igemmILi128ELi128ELi32ELi[34]"]
    for pat in ablated:
        assert not [x for x in prod if re.search(pat, x)], pat
        assert [x for x in abl if re.search(pat, x)], pat                  # ... and the measuring build really has them
    exp = ["Y7T_CONV_VARIANT", "Y7T_CONV_ABLATE", "Y7T_WS_ABLATE", "Y7T_CONV_XCD", "Y7T_STEM_LINES", "Y7T_POOL_LDS", "Y7T_SPP3", "Y7T_CONV_NARROW", "Y7T_CONV_WS_WGS"]
    env_prod = sorted({x for x in prod if re.fullmatch(r"Y7T_[A-Z0-9_]+", x)})
    assert not set(exp) & set(env_prod), env_prod                          # experiment switches are not even named in the product library
    assert set(exp) <= {x for x in abl if re.fullmatch(r"Y7T_[A-Z0-9_]+", x)}
    assert env_prod == ["Y7T_CONV_WS_DYN", "Y7T_TRACKER_ARENA"], env_prod   # the two switches the product library itself reads


def test_readme_lists_the_product_switches():
    """... and the package's run-time switches are the ten of _lib.PRODUCT_SWITCHES, each named in README.md; any other Y7T_* variable is honoured by the lowering only
    beside the measuring build"""
    from yolov7_tracker_amd import _lib
    assert len(_lib.PRODUCT_SWITCHES) <= 10
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in _lib.PRODUCT_SWITCHES:
        assert name in readme, name
    old = os.environ.get("Y7T_LIB")
    try:
        os.environ.pop("Y7T_LIB", None)
        os.environ["Y7T_CONV_PATCH_MIN_PIX"] = "1"
        if not _lib.ablate_build():
            assert _lib.switch("Y7T_CONV_PATCH_MIN_PIX", "25600") == "25600"
        os.environ["Y7T_LIB"] = "/x/liby7t_ablate.so"
        assert _lib.switch("Y7T_CONV_PATCH_MIN_PIX", "25600") == "1"
    finally:
        os.environ.pop("Y7T_CONV_PATCH_MIN_PIX", None)
        os.environ.pop("Y7T_LIB", None)
        if old is not None:
            os.environ["Y7T_LIB"] = old
