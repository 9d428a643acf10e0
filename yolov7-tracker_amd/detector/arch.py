"""YOLOv7 graph specifications in the reference's layer-list form `[from, number, module, args]`
(/root/reference/models/yolo.py:443-520 consumes exactly this from cfg/*.yaml).

`yolov7_w6(nc)` / `yolov7_tiny(nc)` generate the lists programmatically (they are checked against the reference's
cfg/deploy/yolov7-w6.yaml and cfg/deploy/yolov7-tiny.yaml by tests/test_detector_graph.py where the reference is
present), and so do `yolov7` / `yolov7x` (P5, three Detect levels) and `yolov7_e6` / `yolov7_d6` / `yolov7_e6e` (P6, four levels;
tests/test_family_cpu.py); `load_yaml(path)` reads any cfg file of the same format (the CLI's --model_cfg)."""
import yaml

W6_ANCHORS = [[19, 27, 44, 40, 38, 94], [96, 68, 86, 152, 180, 137], [140, 301, 303, 264, 238, 542], [436, 615, 739, 380, 925, 792]]
P5_ANCHORS = [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]]
TINY_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]


def _conv(f, c, k=1, s=1, act=None):
    return [f, 1, "Conv", [c, k, s] if act is None else [c, k, s, None, 1, act]]


def yolov7_w6(nc=80, training=False):
    L = [[-1, 1, "ReOrg", []], _conv(-1, 64, 3, 1)]
    for c in (128, 256, 512, 768, 1024):            # five down-stages: 3x3/s2 + ELAN(4-way concat) + 1x1
        h = c // 2
        L += [_conv(-1, c, 3, 2), _conv(-1, h), _conv(-2, h)] + [_conv(-1, h, 3, 1) for _ in range(4)]
        L += [[[-1, -3, -5, -6], 1, "Concat", [1]], _conv(-1, c)]
    L.append([-1, 1, "SPPCSPC", [512]])              # 47

    def elan_h(c):                                   # head block: two 1x1, four chained 3x3 (c/2), 6-way concat, 1x1
        return [_conv(-1, c), _conv(-2, c)] + [_conv(-1, c // 2, 3, 1) for _ in range(4)] + \
            [[[-1, -2, -3, -4, -5, -6], 1, "Concat", [1]], _conv(-1, c)]
    for c, route in ((384, 37), (256, 28), (128, 19)):   # top-down
        L += [_conv(-1, c), [-1, 1, "nn.Upsample", [None, 2, "nearest"]], _conv(route, c), [[-1, -2], 1, "Concat", [1]]] + elan_h(c)
    for c, route in ((256, 71), (384, 59), (512, 47)):   # bottom-up
        L += [_conv(-1, c, 3, 2), [[-1, route], 1, "Concat", [1]]] + elan_h(c)
    L += [_conv(83, 256, 3, 1), _conv(93, 512, 3, 1), _conv(103, 768, 3, 1), _conv(113, 1024, 3, 1)]
    if training:       # cfg/training/yolov7-w6.yaml:156-162 -- what train_aux.py produces: four aux-head convs + IAuxDetect (models/yolo.py:111-158)
        L += [_conv(83, 320, 3, 1), _conv(71, 640, 3, 1), _conv(59, 960, 3, 1), _conv(47, 1280, 3, 1)]
        L.append([[114, 115, 116, 117, 118, 119, 120, 121], 1, "IAuxDetect", ["nc", "anchors"]])
    else:
        L.append([[114, 115, 116, 117], 1, "Detect", ["nc", "anchors"]])
    return {"nc": nc, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": W6_ANCHORS, "layers": L, "n_backbone": 47}


def yolov7_w6_training(nc=80):
    """the graph of the checkpoints the reference's training actually saves for w6 (README.md:101, cfg/training/yolov7-w6.yaml): at inference the aux
    branch is dead work (yolo.py:141-153 computes and discards it) and ImplicitA / ImplicitM fold into the main head's 1x1 convs"""
    return yolov7_w6(nc, training=True)


def yolov7_tiny(nc=80):
    A = "nn.LeakyReLU(0.1)"

    def c(f, ch, k=1, s=1):
        return _conv(f, ch, k, s, A)

    def elan_t(h, out):
        return [c(-1, h), c(-2, h), c(-1, h, 3, 1), c(-1, h, 3, 1), [[-1, -2, -3, -4], 1, "Concat", [1]], c(-1, out)]
    L = [c(-1, 32, 3, 2), c(-1, 64, 3, 2)] + elan_t(32, 64)
    for h, out in ((64, 128), (128, 256), (256, 512)):
        L += [[-1, 1, "MP", []]] + elan_t(h, out)
    L += [c(-1, 256), c(-2, 256), [-1, 1, "SP", [5]], [-2, 1, "SP", [9]], [-3, 1, "SP", [13]], [[-1, -2, -3, -4], 1, "Concat", [1]],
          c(-1, 256), [[-1, -7], 1, "Concat", [1]], c(-1, 256)]                                     # 29..37
    for ch, route, h in ((128, 21, 64), (64, 14, 32)):
        L += [c(-1, ch), [-1, 1, "nn.Upsample", [None, 2, "nearest"]], c(route, ch), [[-1, -2], 1, "Concat", [1]]] + elan_t(h, ch)
    for ch, route, h in ((128, 47, 64), (256, 37, 128)):
        L += [c(-1, ch, 3, 2), [[-1, route], 1, "Concat", [1]]] + elan_t(h, ch)
    L += [c(57, 128, 3, 1), c(65, 256, 3, 1), c(73, 512, 3, 1), [[74, 75, 76], 1, "Detect", ["nc", "anchors"]]]
    return {"nc": nc, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": TINY_ANCHORS, "layers": L, "n_backbone": 29}


def _elan(c, h, out, n, dense, again=False):
    """ELAN block: two 1x1 convs (c) of one tensor, n chained 3x3 convs (h), a Concat, a 1x1 (out).  dense: the Concat takes every conv of the block (the head blocks of
    yolov7 / e6 / d6 / e6e), else every second 3x3 and the two 1x1 (backbones; yolov7x throughout).  again: the block reads the tensor the block before it read (the
    second half of an e6e double block)"""
    f = -(n + 5) if again else -1
    cat = list(range(-1, -(n + 3), -1)) if dense else list(range(-1, -(n + 1), -2)) + [-(n + 1), -(n + 2)]
    return [_conv(f, c), _conv(f - 1, c)] + [_conv(-1, h, 3, 1) for _ in range(n)] + [[cat, 1, "Concat", [1]], _conv(-1, out)]


def _block(c, h, out, n, dense, double):
    """one ELAN block, or e6e's pair of them over the same input joined by a Shortcut (cfg/deploy/yolov7-e6e.yaml:20-40)"""
    L = _elan(c, h, out, n, dense)
    if double:
        L += _elan(c, h, out, n, dense, again=True) + [[[-1, -(n + 5)], 1, "Shortcut", [1]]]
    return L


def _p5(nc, stem, stages, spp, td, bu, head, n, dense_head, rep):
    """the P5 graphs (yolov7, yolov7x): stem convs, four backbone stages (the last three behind an MP / 3x3-stride-2 down-sampling pair), SPPCSPC, two top-down and two
    bottom-up head blocks, one 3x3 (yolov7: RepConv) per Detect level"""
    L = [_conv(-1, stem[0], 3, 1), _conv(-1, stem[1], 3, 2), _conv(-1, stem[1], 3, 1), _conv(-1, stem[2], 3, 2)]
    routes = []
    for i, (m, h, out) in enumerate(stages):
        if i:
            L += [[-1, 1, "MP", []], _conv(-1, m), _conv(-3, m), _conv(-1, m, 3, 2), [[-1, -3], 1, "Concat", [1]]]
        L += _elan(h, h, out, n, False)
        routes.append(len(L) - 1)
    nb = len(L)
    L.append([-1, 1, "SPPCSPC", [spp]])
    lat, outs = [len(L) - 1], []
    for (c, blk), route in zip(td, (routes[2], routes[1])):      # top-down
        L += [_conv(-1, c), [-1, 1, "nn.Upsample", [None, 2, "nearest"]], _conv(route, c), [[-1, -2], 1, "Concat", [1]]] + _elan(*blk, n, dense_head)
        lat.append(len(L) - 1)
    outs.append(lat.pop())
    for c, blk in bu:                                             # bottom-up
        L += [[-1, 1, "MP", []], _conv(-1, c), _conv(-3, c), _conv(-1, c, 3, 2), [[-1, -3, lat.pop()], 1, "Concat", [1]]] + _elan(*blk, n, dense_head)
        outs.append(len(L) - 1)
    L += [[o, 1, "RepConv", [c, 3, 1]] if rep else _conv(o, c, 3, 1) for o, c in zip(outs, head)]
    L.append([list(range(len(L) - 3, len(L))), 1, "Detect", ["nc", "anchors"]])
    return {"nc": nc, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": P5_ANCHORS, "layers": L, "n_backbone": nb}


def yolov7(nc=80):
    return _p5(nc, (32, 64, 128), ((0, 64, 256), (128, 128, 512), (256, 256, 1024), (512, 256, 1024)), 512,
               ((256, (256, 128, 256)), (128, (128, 64, 128))), ((128, (256, 128, 256)), (256, (512, 256, 512))), (256, 512, 1024), 4, True, True)


def yolov7x(nc=80):
    return _p5(nc, (40, 80, 160), ((0, 64, 320), (160, 128, 640), (320, 256, 1280), (640, 256, 1280)), 640,
               ((320, (256, 256, 320)), (160, (128, 128, 160))), ((160, (256, 256, 320)), (320, (512, 512, 640))), (320, 640, 1280), 6, False, False)


def _p6(nc, stem, widths, n, double):
    """the P6 graphs behind a DownC down-sampling (yolov7-e6, -d6, -e6e): ReOrg + stem conv, five DownC + ELAN stages, SPPCSPC, three top-down and three bottom-up head
    blocks of half-width 3x3 convs, one 3x3 per Detect level.  widths: the five stage widths; n: 3x3 convs per ELAN; double: e6e's Shortcut pairs"""
    L = [[-1, 1, "ReOrg", []], _conv(-1, stem, 3, 1)]
    routes = []
    for c, h in zip(widths, (64, 128, 256, 384, 512)):
        L += [[-1, 1, "DownC", [c]]] + _block(h, h, c, n, False, double)
        routes.append(len(L) - 1)
    nb = len(L)
    L.append([-1, 1, "SPPCSPC", [widths[4] // 2]])
    hb = lambda c, h: _block(h, h // 2, c, n, True, double)
    lat, outs = [len(L) - 1], []
    for c, h, route in ((widths[3] // 2, 384, routes[3]), (widths[2] // 2, 256, routes[2]), (widths[1] // 2, 128, routes[1])):      # top-down
        L += [_conv(-1, c), [-1, 1, "nn.Upsample", [None, 2, "nearest"]], _conv(route, c), [[-1, -2], 1, "Concat", [1]]] + hb(c, h)
        lat.append(len(L) - 1)
    outs.append(lat.pop())
    for c, h in ((widths[2] // 2, 256), (widths[3] // 2, 384), (widths[4] // 2, 512)):                                            # bottom-up
        L += [[-1, 1, "DownC", [c]], [[-1, lat.pop()], 1, "Concat", [1]]] + hb(c, h)
        outs.append(len(L) - 1)
    L += [_conv(o, c, 3, 1) for o, c in zip(outs, widths[1:])]
    L.append([list(range(len(L) - 4, len(L))), 1, "Detect", ["nc", "anchors"]])
    return {"nc": nc, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": W6_ANCHORS, "layers": L, "n_backbone": nb}


def yolov7_e6(nc=80):
    return _p6(nc, 80, (160, 320, 640, 960, 1280), 6, False)


def yolov7_d6(nc=80):
    return _p6(nc, 96, (192, 384, 768, 1152, 1536), 8, False)


def yolov7_e6e(nc=80):
    return _p6(nc, 80, (160, 320, 640, 960, 1280), 6, True)


def load_yaml(path, nc=None):
    with open(path) as f:
        d = yaml.safe_load(f)
    spec = {"nc": d["nc"] if nc is None else nc, "depth_multiple": d.get("depth_multiple", 1.0), "width_multiple": d.get("width_multiple", 1.0),
            "anchors": d["anchors"], "layers": list(d["backbone"]) + list(d["head"]), "n_backbone": len(d["backbone"])}
    return spec


ARCHS = {"yolov7-w6": yolov7_w6, "yolov7-tiny": yolov7_tiny, "yolov7-w6-training": yolov7_w6_training,
         "yolov7": yolov7, "yolov7x": yolov7x, "yolov7-e6": yolov7_e6, "yolov7-d6": yolov7_d6, "yolov7-e6e": yolov7_e6e}
