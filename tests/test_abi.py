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


def test_weight_layouts_are_the_header_enumerators_and_each_has_one_packer():
    """detector/layout.py::WeightLayout is y7t_weight_layout of include/y7t.h by name and value (TWIN_TAIL aside: blob-only, no op carries it), Y7T_WL_COUNT counts the
    layouts an op may carry, and weights.PACKERS has one packer for every layout -- the blob-only one included"""
    from yolov7_tracker_amd.detector import weights
    from yolov7_tracker_amd.detector.layout import OP_LAYOUTS, WeightLayout
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "y7t.h")).read(), flags=re.S)
    enum = {name: int(v) for name, v in re.findall(r"\bY7T_WL_([A-Z0-9_]+)\s*=\s*(\d+)", txt)}
    count = enum.pop("COUNT")
    assert enum == {l.name: int(l) for l in OP_LAYOUTS} and count == len(OP_LAYOUTS) == 12
    assert [int(l) for l in OP_LAYOUTS] == list(range(count)) and WeightLayout.TWIN_TAIL == count
    assert sorted(weights.PACKERS) == sorted(WeightLayout) and all(callable(f) for f in weights.PACKERS.values())


def test_act_bits_of_the_single_layer_entry_point_are_pinned():
    """the second encoding of a layout, in y7t_conv2d_nhwc_f16's `act` argument: the table below is the ABI (bit 8 layout 1, bit 9 forces the patch kernel, bit 8 + L
    layout L); act_bits / layout_of are inverses on it, and of two layout bits the higher layout wins, as in the library's decoder"""
    from yolov7_tracker_amd.detector.layout import FORCE_PATCH, OP_LAYOUTS, WeightLayout, act_bits, layout_of
    pinned = {0: 0, 1: 256, 2: 1024, 3: 2048, 4: 4096, 5: 8192, 6: 16384, 7: 32768, 8: 65536, 9: 131072, 10: 262144, 11: 524288}
    assert {int(l): act_bits(l) for l in OP_LAYOUTS} == pinned and FORCE_PATCH == 512
    for l in OP_LAYOUTS:
        for force in (False, True):
            for act in (0, 1, 2):
                bits = act | act_bits(l, force)
                assert bits == act | pinned[l] | (512 if force else 0) and layout_of(bits) == (l, force) and isinstance(layout_of(bits)[0], WeightLayout)
    for lo in OP_LAYOUTS[1:]:
        for hi in OP_LAYOUTS[lo + 1:]:
            assert layout_of(1 | pinned[lo] | pinned[hi]) == (hi, False)
    with pytest.raises((AssertionError, ValueError)):
        act_bits(WeightLayout.TWIN_TAIL)
    # the C side of the same rule (the header's macro and decoder, nothing else checks Y7T_ACT_LAYOUT), compiled for the host: needs `cc` on PATH, like build()'s oracle
    import subprocess
    import tempfile
    src = ('#include <stdio.h>\n#include "y7t.h"\nint main(void) { for (int l = 0; l < Y7T_WL_COUNT; ++l) for (int h = l; h < Y7T_WL_COUNT; ++h) '
           'printf("%d %d %d %d\\n", l, h, Y7T_ACT_LAYOUT_BITS(l), Y7T_ACT_LAYOUT(2 | Y7T_ACT_FORCE_PATCH | Y7T_ACT_LAYOUT_BITS(l) | Y7T_ACT_LAYOUT_BITS(h))); return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.c"), "w").write(src)
        subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")], check=True)
        rows = [[int(v) for v in r.split()] for r in subprocess.run([os.path.join(tmp, "t")], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(rows) == 78 and all(bits == pinned[l] and got == h for l, h, bits, got in rows)


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
