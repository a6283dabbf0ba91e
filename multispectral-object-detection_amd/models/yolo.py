"""Single-stream YOLOv5 model graph, MI355X-native: the reference's other model file, ``models/yolo.py`` (``Model`` :67-209,
``parse_model`` :211-263) - the RGB-only / IR-only baselines of its README tables and the class its pretrained ``yolov5*.pt``
weights are pickled as.  Same public surface:

    Model(cfg='yolov5s.yaml', ch=3, nc=None, anchors=None)     cfg = yaml path, dict, or a stock name (models/configs.py)
    model(x) -> (pred [B, sum(na*ny*nx), nc+5], [raw_i [B,na,ny_i,nx_i,nc+5]] * nl);  model.train(): the raw list
    model(x, augment=True) -> (pred of the three test-time-augmentation views merged, None)
    model.fuse(), .nms(), .info(), .stride, .names, .yaml, .save, state-dict keys ``model.<i>....`` (the reference's)

``Model`` here is a subclass of the two-stream ``yolo_test.Model``, which is the executor: the same ``LayerGraph`` (row 0 reads ``x``;
a one-input graph has no ``f == -4`` row, hence one lane and no side stream), the same plans, the same walk - ``forward_once`` hands
the parent's walk ``x2 = None`` - the same HIP-graph capture, weight-change tracking, ``fuse`` / ``nms`` / ``info``, the same kernels.
New here are the constructor with the single-stream parser's rules, the strides (derived from the layer graph: this package has no
CPU forward to measure them with) and test-time augmentation, whose image views and prediction merge are the two kernels of
``csrc/tta.hip``.
"""
import logging
import os
from copy import deepcopy
from pathlib import Path

import torch
import torch.nn as nn

from .. import ops
from .common import C3, NMS, SPP, Concat, Conv, Focus, Upsample
from .yolo_test import Detect, check_anchor_order, make_divisible  # noqa: F401  (Detect: ``models.yolo.Detect`` of a reference pickle)
from .yolo_test import Model as _Executor

logger = logging.getLogger(__name__)

# every class the stock models/yolov5{s,m,l,x}.yaml name; another name keeps parse_model's NotImplementedError
MODULES = {"Focus": Focus, "Conv": Conv, "C3": C3, "SPP": SPP, "nn.Upsample": Upsample, "Concat": Concat}
# the ``.type`` tags the reference derives from ``str(class)`` (models/yolo.py:266)
TYPE_NAMES = {"Focus": "models.common.Focus", "Conv": "models.common.Conv", "C3": "models.common.C3", "SPP": "models.common.SPP",
              "Concat": "models.common.Concat", "nn.Upsample": "torch.nn.modules.upsampling.Upsample", "Detect": "models.yolo.Detect"}

TTA_SCALES = (1, 0.83, 0.67)      # models/yolo.py:115-116
TTA_FLIPS = (None, 3, None)       # 3: left-right


def parse_model(d, ch, rows=None):
    """Model dict -> (nn.Sequential, save list) under the rules of the single-stream file (reference models/yolo.py:211-263), for the
    module set above: depth gain ``max(round(n * gd), 1)``, width gain ``make_divisible(c2 * gw, 8)`` except for the head's output
    width, every conv-like module - ``Focus`` too, which the two-stream file forces to 3 - takes ``ch[f]`` input channels, C3 gets ``n``
    as its third argument, each top-level module is tagged with ``.i / .f / .type / .np``.  A yaml that names another class raises.
    ``rows``: a list that receives one ``(i, f, n, np, type, args)`` per layer - the table the reference logs while it parses."""
    anchors, nc, gd, gw = d["anchors"], d["nc"], d["depth_multiple"], d["width_multiple"]
    na = (len(anchors[0]) // 2) if isinstance(anchors, list) else anchors
    no = na * (nc + 5)
    symbols = {"nc": nc, "anchors": anchors, "None": None, "False": False, "True": True}
    layers, save, c2 = [], [], ch[-1]
    for i, (f, n, name, args) in enumerate(d["backbone"] + d["head"]):
        if name not in MODULES and name != "Detect":
            raise NotImplementedError(f"module {name!r} (layer {i}) is outside the single-stream module set; supported: "
                                      f"{sorted(MODULES) + ['Detect']}")
        m = Detect if name == "Detect" else MODULES[name]
        args = [symbols.get(a, a) if isinstance(a, str) else a for a in args]
        n = max(round(n * gd), 1) if n > 1 else n
        if m in (Conv, SPP, Focus, C3):
            c1, c2 = ch[f], args[0]
            if c2 != no:
                c2 = make_divisible(c2 * gw, 8)
            args = [c1, c2, *args[1:]]
            if m is C3:
                args.insert(2, n)
                n = 1
        elif m is Concat:
            c2 = sum(ch[x] for x in f)
        elif m is Detect:
            args.append([ch[x] for x in f])
            if isinstance(args[1], int):
                args[1] = [list(range(args[1] * 2))] * len(f)
        else:
            c2 = ch[f]
        m_ = nn.Sequential(*[m(*args) for _ in range(n)]) if n > 1 else m(*args)
        np_ = sum(x.numel() for x in m_.parameters())
        m_.i, m_.f, m_.type, m_.np = i, f, TYPE_NAMES[name], np_
        if rows is not None:
            rows.append((i, f, n, np_, m_.type, args))
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        if i == 0:
            ch = []
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save)


def graph_strides(layers):
    """The stride of every Detect input, from the layer graph alone: the product of the strides along its path from the image.
    ``Focus`` halves (space-to-depth), a ``Conv`` divides by its conv's stride, ``nn.Upsample`` multiplies by its factor, C3 / SPP keep
    the size and the inputs of a ``Concat`` must agree.  The reference measures the same numbers with a 256 x 256 CPU forward
    (models/yolo.py:97-103)."""
    from fractions import Fraction
    from .layer_graph import LayerGraph
    g = LayerGraph(layers)
    size = []                                           # feature-map side per image pixel, per layer
    for i, m in enumerate(g.layers):
        srcs = [size[j] for j in g.sources[i]] or [Fraction(1)]
        if isinstance(m, Detect):
            size.append(None)
            continue
        if any(s != srcs[0] for s in srcs):
            raise ValueError(f"layer {i} ({type(m).__name__}) joins feature maps of different strides")
        s = srcs[0]
        if isinstance(m, Focus):
            s = s / (2 * m.conv.conv.stride[0])
        elif type(m) is Conv:
            s = s / m.conv.stride[0]
        elif isinstance(m, torch.nn.Upsample):
            s = s * Fraction(float(m.scale_factor))
        elif not isinstance(m, (C3, SPP, Concat)):
            raise NotImplementedError(f"graph_strides: layer {i} is a {type(m).__name__}")
        size.append(s)
    return [float(1 / size[j]) for j in g.sources[len(g.layers) - 1]]


class Model(_Executor):
    """The single-stream model (reference models/yolo.py:67-209): ``model(x)``.  The two-stream ``Model`` is its executor; the
    constructor is this file's own (its parser, its strides) and ``forward`` / ``forward_once`` take one image batch."""
    inputs = 1                              # image batches per forward (graph.CapturedForward keeps one static buffer each)

    def __init__(self, cfg="yolov5s.yaml", ch=3, nc=None, anchors=None):
        nn.Module.__init__(self)
        if isinstance(cfg, str) and not os.path.exists(cfg):        # a stock name where the reference's yaml files are not at hand
            from .configs import STOCK_YAMLS, stock_config
            name = os.path.basename(cfg)[:-5] if cfg.endswith(".yaml") else cfg
            if name in STOCK_YAMLS:
                cfg = stock_config(name)
        if isinstance(cfg, dict):
            self.yaml = deepcopy(cfg)
        else:
            import yaml
            self.yaml_file = Path(cfg).name
            with open(cfg) as fh:
                self.yaml = yaml.safe_load(fh)
        ch = self.yaml["ch"] = self.yaml.get("ch", ch)
        if nc and nc != self.yaml["nc"]:
            logger.info(f"Overriding model.yaml nc={self.yaml['nc']} with nc={nc}")
            self.yaml["nc"] = nc
        if anchors:
            logger.info(f"Overriding model.yaml anchors with anchors={anchors}")
            self.yaml["anchors"] = round(anchors)
        self.model, self.save = parse_model(deepcopy(self.yaml), [ch])
        self.names = [str(i) for i in range(self.yaml["nc"])]
        m = self.model[-1]
        if isinstance(m, Detect):
            m.stride = torch.tensor(graph_strides(self.model))      # the reference measures them with a CPU forward (:97-103)
            m.anchors /= m.stride.view(-1, 1, 1)
            check_anchor_order(m)
            self.stride = m.stride
            self._initialize_biases()
        self._graphs = {}
        self.compute_dtype = torch.bfloat16
        self.set_compute_dtype(torch.bfloat16)
        self.overlap_streams = True          # (a one-input graph has one lane: nothing to overlap)
        self.eval()

    # ---- reference-compatible API -----------------------------------------------------------
    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected one [B,3,H,W] image batch, got {tuple(x.shape)}")
        smax = int(self.stride.max()) if hasattr(self, "stride") else 32
        if x.shape[2] % smax or x.shape[3] % smax:
            raise ValueError(f"image height and width must be multiples of the largest stride ({smax}); got "
                             f"{x.shape[2]}x{x.shape[3]} (the reference letterboxes to such sizes, utils/datasets.py:1698-1728)")
        if x.dtype not in (torch.uint8, torch.float16, torch.float32):
            raise TypeError(f"images must be uint8, float16 or float32, got {x.dtype}")

    def forward(self, x, augment=False, profile=False):
        self._check_input(x)
        if augment:
            return self._forward_augment(x)
        return self._forward_one(x, profile)

    def _forward_one(self, x, profile=False):
        key = (tuple(x.shape), self.compute_dtype, x.dtype)
        g = None if (self.training or profile) else self._graphs.get(key)     # profile: per-layer events need eager launches
        if g is not None:
            if g.weights_key == self.weights_key():
                out = g.replay(x)
                return self.model[-1](out) if type(self.model[-1]) is NMS else out      # the graph ends at Detect (NMS syncs with the host)
            self._graphs.clear()            # weights changed since capture: the graph would replay the old ones
        return self.forward_once(x, profile)

    def forward_once(self, x, profile=False, until_detect=False):
        """One walk of the layer graph on an image batch: the executor's walk without a second image (reference models/yolo.py:132-153)."""
        return _Executor.forward_once(self, x, None, profile, until_detect)

    def _forward_augment(self, x):
        """Test-time augmentation (reference models/yolo.py:113-128): the image at scales 1 / 0.83 / 0.67, the middle view mirrored
        left-right, each view through the network, the boxes scaled and mirrored back, all rows concatenated.  ``cft_tta_view``
        builds views 1 and 2 (view 0 is the input itself, as in ``scale_img``), ``cft_tta_merge`` the result; the three forwards
        have three shapes, so a captured model replays three graphs."""
        if self.training or type(self.model[-1]) is NMS:
            raise RuntimeError("augmented inference takes a model in eval mode whose last layer is Detect (reference models/yolo.py:120 "
                               "indexes forward_once's (pred, raw) tuple)")
        gs = int(self.stride.max())
        B, _, H, W = x.shape
        keys = [((B, 3, H, W), x.dtype) if (si == 1 and not fi) else ((B, 3, *ops.tta_view_size(H, W, si, gs)[1]), torch.float32)
                for si, fi in zip(TTA_SCALES, TTA_FLIPS)]
        preds = []
        for k, (si, fi) in enumerate(zip(TTA_SCALES, TTA_FLIPS)):
            xi = x if (si == 1 and not fi) else ops.tta_view(x, si, gs, flip=fi == 3)
            p = self._forward_one(xi)[0]
            g = self._graphs.get((keys[k][0], self.compute_dtype, keys[k][1]))
            if g is not None and p is g.pred and keys[k] in keys[k + 1:]:
                p = p.clone()                      # a later view of the same shape replays this graph into the same static tensor
            preds.append(p)
        return ops.tta_merge(preds, TTA_SCALES, [fi == 3 for fi in TTA_FLIPS], x.shape[3]), None

    def capture_augment(self, batch, height, width, input_dtype=torch.float32):
        """``capture`` for the three shapes of ``forward(x, augment=True)``: the input's and the two fp32 views'."""
        gs = int(self.stride.max())
        graphs = [self.capture(batch, height, width, input_dtype)]
        for si in TTA_SCALES[1:]:
            _, (h, w) = ops.tta_view_size(height, width, si, gs)
            if ((batch, 3, h, w), self.compute_dtype, torch.float32) not in self._graphs:
                graphs.append(self.capture(batch, h, w, torch.float32))
        return graphs

    def autoshape(self):
        raise NotImplementedError("autoShape around a single-stream model is outside this package (DESIGN.md section 7)")
