"""The weight layouts of the conv kernels by name: the Python side of `y7t_weight_layout` in include/y7t.h (tests/test_abi.py compares the two).  A layout says how a
layer's [Cout_pad][K_pad] fp16 block is packed and therefore which kernel runs the op; `y7t_op.korder` and the `korder` of a wlayout entry hold one.  The packer of
each layout: weights.PACKERS (it sits beside the packers).  The values are ABI."""
import enum


class WeightLayout(enum.IntEnum):
    TAP_MAJOR = 0           # rows with k = (kh*KW + kw)*Cin + ci
    LINE_MAJOR = 1          # rows with k in (kh, 64-channel chunk, kw) order
    PATCH = 2               # LDS-patch panels
    PANEL_1X1 = 3           # per-K-step 1x1 panels
    PATCH_S2 = 4            # stride-2 LDS-patch panels
    WS64 = 5                # 64 -> 64 fragments
    WS128 = 6               # 128 -> 128 k fragments, stride 1 and 2
    P8 = 7                  # 256 x 64 ping-pong panels
    WS_S2 = 8               # 64 -> 128 stride-2 fragments
    PATCH_N64 = 9           # PATCH with 64-row panels
    PANEL_1X1_N64 = 10      # PANEL_1X1 with 64-row panels
    WS_S2_TWIN = 11         # WS_S2 followed by the twin 1x1 bank and its biases: one op, two wlayout entries (WS_S2, then TWIN_TAIL)
    TWIN_TAIL = 12          # blob-only: the twin 1x1 bank behind a WS_S2_TWIN op.  Never in an op -- the library refuses it


OP_LAYOUTS = tuple(l for l in WeightLayout if l is not WeightLayout.TWIN_TAIL)      # what an op may carry: Y7T_WL_COUNT of them
FORCE_PATCH = 512


def act_bits(layout, force_patch=False):
    """the bits of y7t_conv2d_nhwc_f16's `act` argument that choose `layout` (bit 8: layout 1; bit 8 + L: layout L = 2 .. 11) and force the patch kernel (bit 9)"""
    layout = WeightLayout(layout)
    assert layout in OP_LAYOUTS, layout
    return (0 if layout == 0 else 256 if layout == 1 else 256 << layout) | (FORCE_PATCH if force_patch else 0)


def layout_of(act):
    """-> (layout, force_patch) of an `act` argument; of several layout bits the highest layout wins"""
    return next((l for l in reversed(OP_LAYOUTS[2:]) if act & 256 << l), WeightLayout(act >> 8 & 1)), bool(act & FORCE_PATCH)
