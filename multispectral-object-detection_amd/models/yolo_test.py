"""Two-stream (RGB + thermal) YOLOv5/CFT model graph, MI355X-native.

Drop-in for the reference's ``models/yolo_test.py`` - which, despite its name, is the two-stream
*model definition* (SURVEY.md D1): ``Detect`` :25-64, ``Model`` :165-327, ``parse_model`` :479-555
(file:line = /root/reference/models/yolo_test.py).  Same public surface:

    Model(cfg, ch=3, nc=None, anchors=None)      cfg = yaml path or dict (reference yamls load unchanged)
    model(x, x2) -> (pred [B, sum(na*ny*nx), nc+5], [raw_i [B,na,ny_i,nx_i,nc+5]] * nl)
    model.fuse(), .stride, .names, .yaml, .save, state-dict keys ``model.<i>....``

What differs is underneath: every layer runs hand-written gfx950 kernels on NHWC activations
(``models/common.py`` here), the compute precision is a model property
(``set_compute_dtype(torch.bfloat16 | torch.float16 | torch.float32)``; ``model.half()`` selects fp16 like it
does in the reference's callers, test.py:66-68; images arrive fp32 / fp16 / uint8 NCHW at the boundary), and
the whole forward can be captured once into a HIP graph (``capture``) so that the ~600 kernel
launches of yolov5l+CFTx3 cost one graph launch.
"""
import logging
import math
from contextlib import nullcontext
from copy import deepcopy
from pathlib import Path

import torch
import torch.nn as nn

from .. import ops
from .common import (GPT, NMS, SPP, Add, Add2, Bottleneck, C3, Concat, Conv, Focus, PendingBilinear, PendingConv, Upsample, _Packed, autoShape, resolve,
                     ACT_NONE, invalidate_packed, myTransformerBlock)
from .layer_graph import LayerGraph, graph_key

logger = logging.getLogger(__name__)

# yaml module name -> class.  The reference resolves names with eval() inside
# ``from models.common import *`` (models/yolo_test.py:488); the hot-path classes are these.
MODULES = {
    "Conv": Conv, "Bottleneck": Bottleneck, "C3": C3, "SPP": SPP, "Focus": Focus, "Concat": Concat,
    "Add": Add, "Add2": Add2, "GPT": GPT, "nn.Upsample": Upsample, "Upsample": Upsample,
}


def make_divisible(x, divisor):  # reference utils/general.py:210-212
    return math.ceil(x / divisor) * divisor


class Detect(_Packed):
    """Detection head (reference models/yolo_test.py:25-64): per level a 1x1 conv (+bias) on the
    MFMA GEMM (fp32 logits), then one decode kernel writes both the permuted raw logits and the
    decoded rows of the concatenated prediction tensor."""
    stride = None
    export = False

    def __init__(self, nc=80, anchors=(), ch=()):
        super().__init__()
        self.nc = nc
        self.no = nc + 5
        self.nl = len(anchors)
        self.na = len(anchors[0]) // 2
        self.grid = [torch.zeros(1)] * self.nl          # kept for attribute parity; the kernel derives the grid
        a = torch.tensor(anchors).float().view(self.nl, -1, 2)
        self.register_buffer("anchors", a)
        self.register_buffer("anchor_grid", a.clone().view(self.nl, 1, -1, 1, 1, 2))
        self.m = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch)

    def _pack(self, dtype, device):
        anchors_px = self.anchor_grid.detach().to(device=device, dtype=torch.float32).view(self.nl, -1).contiguous()
        return [ops.pack_conv(m.weight, m.bias, dtype, device=device) for m in self.m], anchors_px

    def forward(self, x):
        if self.export:
            raise RuntimeError("Detect: the ONNX-export branch is outside the hot path")
        x = [resolve(t) for t in x]
        packed, anchors_px = self._packed(x[0].dtype, x[0].device)
        B = x[0].shape[0]
        dev = x[0].device
        rows = [self.na * t.shape[2] * t.shape[3] for t in x]
        pred = torch.empty((B, sum(rows), self.no), dtype=torch.float32, device=dev)
        raws, row0 = [], 0
        for i in range(self.nl):
            logits = ops.conv2d(x[i], packed[i], ACT_NONE, out_dtype=torch.float32)   # [B, pad8(na*no), ny, nx]
            ny, nx = logits.shape[2], logits.shape[3]
            raw = torch.empty((B, self.na, ny, nx, self.no), dtype=torch.float32, device=dev)
            ops.detect_decode(logits, raw, pred, anchors_px[i], self.na, self.no, float(self.stride[i]), row0)
            raws.append(raw)
            row0 += rows[i]
        return raws if self.training else (pred, raws)      # training: only the raw list (reference :59)


def check_anchor_order(m):
    """Flip the anchor levels if their area order disagrees with the stride order
    (reference utils/autoanchor.py:12-20)."""
    a = m.anchor_grid.prod(-1).view(-1)
    da = a[-1] - a[0]
    ds = m.stride[-1] - m.stride[0]
    if da.sign() != ds.sign():
        m.anchors[:] = m.anchors.flip(0)
        m.anchor_grid[:] = m.anchor_grid.flip(0)


def parse_model(d, ch):
    """Model dict -> (nn.Sequential, save list); same rules as reference models/yolo_test.py:479-555:
    depth gain max(round(n*gd),1), width gain make_divisible(c2*gw, 8), Focus forced to 3 input
    channels, C3 gets n as its 3rd argument, GPT width = channels of its first input, and each
    top-level module is tagged with .i/.f/.type/.np."""
    anchors, nc, gd, gw = d["anchors"], d["nc"], d["depth_multiple"], d["width_multiple"]
    na = (len(anchors[0]) // 2) if isinstance(anchors, list) else anchors
    no = na * (nc + 5)
    symbols = {"nc": nc, "anchors": anchors, "None": None, "False": False, "True": True}
    layers, save, c2 = [], [], ch[-1]
    for i, (f, n, m, args) in enumerate(d["backbone"] + d["head"]):
        name = m
        if isinstance(m, str):
            if m not in MODULES and m != "Detect":
                raise NotImplementedError(f"module {m!r} (layer {i}) is outside the CFT hot path; supported: "
                                          f"{sorted(MODULES) + ['Detect']}")
            m = Detect if m == "Detect" else MODULES[m]
        args = [symbols.get(a, a) if isinstance(a, str) else a for a in args]
        n = max(round(n * gd), 1) if n > 1 else n
        if m in (Conv, Bottleneck, SPP, Focus, C3):
            c1 = 3 if m is Focus else ch[f]
            c2 = args[0]
            if c2 != no:
                c2 = make_divisible(c2 * gw, 8)
            args = [c1, c2, *args[1:]]
            if m is C3:
                args.insert(2, n)
                n = 1
        elif m is Concat:
            c2 = sum(ch[x] for x in f)
        elif m is Add:
            c2 = ch[f[0]]
            args = [c2]
        elif m is Add2:
            c2 = ch[f[0]]
            args = [c2, args[1]]
        elif m is GPT:
            c2 = ch[f[0]]
            args = [c2]
        elif m is Detect:
            args.append([ch[x] for x in f])
            if isinstance(args[1], int):
                args[1] = [list(range(args[1] * 2))] * len(f)
        else:
            c2 = ch[f]
        m_ = nn.Sequential(*[m(*args) for _ in range(n)]) if n > 1 else m(*args)
        t = name if isinstance(name, str) else m.__name__
        np_ = sum(x.numel() for x in m_.parameters())
        m_.i, m_.f, m_.type, m_.np = i, f, t, np_
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        if i == 0:
            ch = []
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save)


class Model(nn.Module):
    def __init__(self, cfg="yolov5s.yaml", ch=3, nc=None, anchors=None):
        super().__init__()
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
        self.model, self.save = parse_model(deepcopy(self.yaml), ch=[ch])
        self.names = [str(i) for i in range(self.yaml["nc"])]
        m = self.model[-1]
        if isinstance(m, Detect):
            m.stride = torch.Tensor([8.0, 16.0, 32.0])      # hard-coded by the reference (:201)
            m.anchors /= m.stride.view(-1, 1, 1)
            check_anchor_order(m)
            self.stride = m.stride
            self._initialize_biases()
        self._graphs = {}
        self.compute_dtype = torch.bfloat16
        self.set_compute_dtype(torch.bfloat16)   # the Focus modules (where the network's precision is set) mirror it
        self.overlap_streams = True      # run the RGB and the IR backbone on two HIP streams
        self.eval()

    def __setstate__(self, state):
        """Un-pickling a checkpoint written by the reference restores only the reference's attributes."""
        super().__setstate__(state)
        self.__dict__.setdefault("_graphs", {})
        if "compute_dtype" not in self.__dict__:     # a reference pickle: compute in the precision its weights carry
            p = next(self.parameters(), None)       # (checkpoints are saved .half(), train.py:852; attempt_load then .float()s)
            self.__dict__["compute_dtype"] = p.dtype if p is not None and p.dtype in ops.COMPUTE_DTYPES else torch.float32
        self.__dict__.setdefault("overlap_streams", True)
        self.set_compute_dtype(self.compute_dtype)   # Focus.compute_dtype always mirrors Model.compute_dtype

    # ---- weight-change tracking: a captured graph replays the packed buffers of capture time -------
    def invalidate_packed(self):
        """Forget packed weights and captured graphs; call after editing weights through ``.data``."""
        invalidate_packed(self)
        return self

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        invalidate_packed(self)
        return out

    def _apply(self, fn, *args, **kwargs):
        """``.to()/.cuda()/.half()/.float()`` move or cast the parameters: packed copies and graphs are stale."""
        out = super()._apply(fn, *args, **kwargs)
        invalidate_packed(self)
        return out

    def half(self):
        """Reference callers switch to fp16 inference with ``model.half()`` (test.py:66-68, detect_twostream.py:
        40-41): parameters become fp16 as in ``nn.Module.half`` and the kernels compute in fp16 (fp32 accumulate)."""
        super().half()
        return self.set_compute_dtype(torch.float16)

    def float(self):
        """``attempt_load(...).float()``: fp32 parameters; a model put into fp16 by ``half()`` returns to fp32 compute."""
        super().float()
        if self.compute_dtype == torch.float16:
            self.set_compute_dtype(torch.float32)
        return self

    def bfloat16(self):
        super().bfloat16()
        return self.set_compute_dtype(torch.bfloat16)

    # ---- reference-compatible API -----------------------------------------------------------
    def forward(self, x, x2, augment=False, profile=False):
        if augment:
            raise NotImplementedError("augmented inference is broken for two-stream models in the reference "
                                      "(models/yolo_test.py:215-230 calls forward_once with one input)")
        if x.shape != x2.shape or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected two [B,3,H,W] image batches of equal shape, got {tuple(x.shape)} and {tuple(x2.shape)}")
        smax = int(self.stride.max()) if hasattr(self, "stride") else 32
        if x.shape[2] % smax or x.shape[3] % smax:
            raise ValueError(f"image height and width must be multiples of the largest stride ({smax}); got "
                             f"{x.shape[2]}x{x.shape[3]} (the reference letterboxes to such sizes, utils/datasets.py:1698-1728)")
        key = (tuple(x.shape), self.compute_dtype, x.dtype)
        g = None if (self.training or profile) else self._graphs.get(key)     # profile: per-layer events need eager launches
        if g is not None:
            if g.weights_key == self.weights_key():
                out = g.replay(x, x2)
                return self.model[-1](out) if type(self.model[-1]) is NMS else out      # the graph ends at Detect (NMS syncs with the host)
            self._graphs.clear()            # weights changed since capture: the graph would replay the old ones
        return self.forward_once(x, x2, profile)

    def weights_key(self):
        """Cheap fingerprint (~0.15 ms) of every parameter/buffer's in-place version counter, compared at replay
        time.  Re-allocations (``.to()``, ``.half()``, ``load_state_dict``, ``fuse()``) go through
        ``invalidate_packed`` instead, which also drops the cached tensor list used here."""
        ws = self.__dict__.get("_wlist")
        if ws is None:
            ws = self.__dict__["_wlist"] = list(self.parameters()) + list(self.buffers())
        return hash(tuple(t._version for t in ws))

    # ---- layer graph and plans (models/layer_graph.py) ------------------------------------------------------------------
    def layer_graph(self):
        """The ``LayerGraph`` of the current layer list: rebuilt, with every plan, whenever ``self.model`` holds other layers."""
        g = self.__dict__.get("_layer_graph")
        if g is None or g.key != graph_key(self.model):
            g = self.__dict__["_layer_graph"] = LayerGraph(self.model)
        return g

    def stream_lanes(self):
        """Lane (HIP stream) of every layer: the IR backbone - everything reachable from an ``f == -4``
        entry through single-input edges, plus ``Add2(index=1)`` whose base input is the IR feature - is
        lane 1; joins (GPT, Add, Concat, Detect) and the RGB backbone/head are lane 0."""
        return list(self.layer_graph().lanes)

    def concat_plan(self):
        """{producer layer index: (concat layer index, channel offset, channels, total channels)} for every Concat
        source that is a Conv / C3 / Add (they take ``out=``); such a producer's output tensor then IS a channel
        slice of the concat buffer and ``Concat`` skips its copy.  Upsample sources stay deferred copies."""
        return self.layer_graph().concat_plan

    def chain_plan(self):
        """Indices of the ``Conv`` layers whose output is read by exactly one layer, the ``C3`` right behind them (``f == -1``): yaml
        rows 1, 3, 6, 8, 13, 15 of the x3 configs (the convs in front of SPP or Concat do not qualify).  Such a conv is handed to its
        C3 un-run (``PendingConv``); the C3's launch plan (``C3.launch_plan``) issues both as one kernel when ``cft_conv2d_chain_ok``
        accepts the pair (a conv of 128 or 256 output channels: rows 1, 3, 6, 8 of yolov5l), else it runs the conv itself."""
        return self.layer_graph().chain_plan

    def cft_fusion_plan(self):
        """{index of the first Add2 behind a GPT block: (GPT index, index of the second Add2, index of the Add that consumes both
        or None)} - yaml rows 10-12 + 29 (17-19 + 30, 26-28 + 31) of the x3 configs.  The pattern is matched structurally; a config
        without it (add-fusion, 4-GPT variants with other wiring) simply has no entries."""
        return self.layer_graph().cft_fusion_plan

    def prefix_segments(self, max_rows=None):
        """[(i0, i1)]: maximal runs of layers that depend on ONE image batch only - a ``Focus`` fed by ``x`` (row 0) or ``x2`` (``f == -4``)
        followed by ``f == -1`` Conv / C3 rows whose outputs have exactly one reader, the next row - cut to ``max_rows`` layers and
        to end on a C3 (a trailing Conv would be a ``PendingConv`` of a C3 outside the segment).  x3 configs: rows 0-4 and 5-9."""
        return list(self.layer_graph().prefix_segments(max_rows))

    # Executor switches that change WHICH launches a walk issues: a captured graph replays the launches of capture time, so every
    # setter drops the graphs (an A/B flipped after capture() used to compare a path against itself).  ``push``: (sub-module
    # type, attribute) - an on/off switch whose value the sub-modules of that type carry as well.
    def _switch(name, default, doc, push=None):      # noqa: N805 - class-body helper
        def get(self):
            return self.__dict__.get("_" + name, default)

        def set_(self, v):
            if push is not None:
                v = bool(v)
                for m in self.modules():
                    if isinstance(m, push[0]):
                        setattr(m, push[1], v)
            self.__dict__["_" + name] = v
            self.__dict__.get("_graphs", {}).clear()
        return property(get, set_, doc=doc)

    chain_convs = _switch("chain_convs", True,
                          "Run producer / pointwise-consumer layer pairs as one ``cft_conv2d_chain`` kernel where eligible (default): the Conv handed to "
                          "the C3 behind it (``chain_plan``) and, inside a C3 without shortcuts, ``Bottleneck[j].cv2`` + ``Bottleneck[j+1].cv1``.  ``False`` "
                          "runs every layer as its own launch (A/B; bit-identical results).", push=(C3, "chain"))
    chain_pairs = _switch("chain_pairs", True,
                          "The chains inside a C3 on their own: ``Bottleneck[j].cv2`` (+ shortcut) + ``Bottleneck[j+1].cv1`` as one kernel where "
                          "``C3.launch_plan`` finds the pair eligible (default).  ``False`` leaves only the Conv + cv1|cv2 chains (A/B; bit-identical results).",
                          push=(C3, "chain_pairs"))
    splitk = _switch("splitk", True,
                     "Run the CFT blocks' out_proj / fc2 GEMMs as split-K launches where ``ops.splitk_choice`` splits them (default; the LayerNorm that "
                     "follows folds the fp32 partial sums into the residual stream in a fixed order).  ``False``: one launch per GEMM with the residual "
                     "add in its epilogue (A/B; results differ by fp32 summation order only).", push=(myTransformerBlock, "splitk"))
    fuse_cft_outputs = _switch("fuse_cft_outputs", True, "Run the two Add2 layers behind a GPT block and the Add that sums them as one kernel (cft_fusion_plan).")
    plan_concats = _switch("plan_concats", True, "Let Conv / C3 / Add layers that feed a head Concat write straight into their slice of its buffer (concat_plan).")
    depth_first = _switch("depth_first", None,
                          "None, or (chunks, rows): run the image-only prefix of each backbone (Focus -> Conv -> C3 -> ..., ``prefix_segments``) "
                          "DEPTH-FIRST over ``chunks`` sub-batches - all of its (at most ``rows``) layers for pairs [0, B/chunks), then for the next "
                          "sub-batch, ... - so that a layer reads what its producer just wrote while those bytes are still in the 256-MiB Infinity "
                          "Cache instead of HBM (at 64 pairs the P1 / P2 tensors are 420 - 840 MB each).  Per-image arithmetic is unchanged: "
                          "bit-identical outputs.  Inference only (BatchNorm batch statistics span the batch).")
    del _switch

    def _run_segment(self, g, seg, img, cbufs, chunks):
        """Layers ``seg = (i0, i1)`` depth-first over ``chunks`` sub-batches of the image batch ``img``; returns the last layer's output
        for the whole batch (each sub-batch's C3 writes its batch slice of it)."""
        i0, i1 = seg
        layers = g.layers
        B = img.shape[0]
        full = None
        for c in range(chunks):
            b0, b1 = B * c // chunks, B * (c + 1) // chunks
            if b1 == b0:
                continue
            x = layers[i0](img[b0:b1])
            for i in range(i0 + 1, i1):
                x = self._run_layer(g, layers[i], x, cbufs)
            shape = x.shape                                   # (PendingConv knows its output shape without running)
            if full is None:
                c2 = layers[i1].cv3.conv.out_channels
                dt = x.x.dtype if isinstance(x, PendingConv) else x.dtype
                full = ops.new_nhwc(B, shape[2], shape[3], c2, dt, img.device)
            layers[i1](x, out=full[b0:b1])
        return full

    @staticmethod
    def _concat_slice(g, i, cbufs, B, H, W, dtype, device):
        """Layer ``i``'s planned channel slice of its consumer's concat buffer (allocated [B, total, H, W] at the first request of a
        walk), or None: no walk buffers, ``i`` is not planned, or the buffer has another geometry."""
        tgt = g.concat_plan.get(i) if cbufs is not None else None
        if tgt is None:
            return None
        cidx, off, c, total = tgt
        buf = cbufs.get(cidx)
        if buf is None:
            buf = cbufs[cidx] = ops.new_nhwc(B, H, W, total, dtype, device)
        return buf[:, off:off + c] if tuple(buf.shape) == (B, total, H, W) else None

    def _fused_cft_outputs(self, g, m, x, y, cbufs):
        """Layer ``m`` is the first Add2 of a planned group and its GPT input is still deferred: run the dual de-tokeniser
        (``cft_gpt_upsample_add2``) and return {layer index: output} for the group, else None."""
        ent = g.cft_fusion_plan.get(m.i)
        if ent is None or not isinstance(x, (list, tuple)) or not isinstance(x[1], (list, tuple)):
            return None
        i, j2, k = ent
        p0, p1 = x[1][0], x[1][1]
        if not (isinstance(p0, PendingBilinear) and isinstance(p1, PendingBilinear) and p0.tokens is p1.tokens):
            return None
        if not ops.gpt_dual_tokens_ok(p0.tokens):        # the dual kernel is specialised for 2 x 64 fp32 tokens (8 x 8 anchors)
            return None
        m2 = g.layers[j2]
        base_m = resolve(x[0])
        base_o = y[g.sources[j2][0]]
        if base_o is None or not base_m.is_cuda:
            return None
        base_o = resolve(base_o)
        bases = [None, None]
        bases[m.index], bases[m2.index] = base_m, base_o
        sum_out = None
        if k is not None:                             # the Add's planned concat slice (what _run_layer would hand to Add.forward)
            B, _, H, W = base_m.shape
            sum_out = self._concat_slice(g, k, cbufs, B, H, W, base_m.dtype, base_m.device)
        o0, o1, osum = ops.gpt_upsample_add_dual(p0.tokens, bases[0], bases[1], p0.H, p0.W, p0.dtype, sum_out=sum_out, want_sum=k is not None)
        outs = {m.i: (o0, o1)[m.index], j2: (o0, o1)[m2.index]}
        if k is not None:
            outs[k] = osum
        return outs

    def _run_layer(self, g, m, x, cbufs, chain=True):
        """One layer on its gathered input ``x`` (an image batch for the rows that consume one).  ``chain=False`` (profiling walks): every
        layer issues its own launches, so the per-layer table charges a Conv's time to the Conv and not to the C3 that would otherwise
        run it."""
        if g.image[m.i] == 1 or (m.i == 0 and isinstance(m, Focus)):
            return m(x)
        if cbufs is not None and m.i in g.concat_plan:
            t = x[0] if isinstance(x, (list, tuple)) else x
            shape = t.shape if isinstance(t, PendingConv) else None     # (stays un-run: only its geometry is needed here)
            t = t.x if isinstance(t, PendingConv) else resolve(t)
            if isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4:
                B, _, H, W = shape or t.shape
                if type(m) is Conv:
                    H, W = ops.conv_out_size(H, W, m.conv.kernel_size[0], m.conv.stride[0])
                out = self._concat_slice(g, m.i, cbufs, B, H, W, t.dtype, t.device)
                if out is not None:
                    return m(x, out=out)
        if cbufs is not None and isinstance(m, Concat) and m.i in cbufs:
            return m(x, out=cbufs[m.i])
        if (chain and cbufs is not None and not self.training and m.i in g.chain_plan and self.chain_convs
                and isinstance(x, torch.Tensor) and x.dtype in (torch.bfloat16, torch.float16)):
            return PendingConv(m, x)                 # left to the C3 behind it (one kernel for the conv and the C3's cv1|cv2)
        return m(x)

    def forward_once(self, x, x2, profile=False, until_detect=False):
        """Graph walk of reference models/yolo_test.py:235-272: ``f == -1`` previous output, int /
        list = saved outputs, ``f == -4`` = this layer consumes the IR image ``x2``.
        ``until_detect``: stop in front of a trailing ``NMS`` module (HIP-graph capture: NMS reads its counts on the host).

        The two backbones are independent between fusion points, so with ``overlap_streams`` they are
        enqueued on two HIP streams (fork/join by stream waits; inside a HIP-graph capture this becomes
        two parallel branches of the graph).  Every tensor that crosses lanes is a saved layer output
        and stays referenced (``keep``) until the lanes have joined, so the caching allocator cannot recycle it
        under a kernel of the other stream.  A one-lane walk (``lanes is None``) has no side stream, no waits and keeps nothing."""
        g = self.layer_graph()
        layers = g.layers
        if until_detect and layers and type(layers[-1]) is NMS:
            layers = layers[:-1]
        lanes = g.lanes if (self.overlap_streams and x.is_cuda and not profile) else None
        if lanes is not None and 1 not in lanes:
            lanes = None
        fused = {}                                                    # outputs of a CFT output group still to be handed to their layers
        fuse_cft = x.is_cuda and self.fuse_cft_outputs and not profile      # profile: one launch group per layer (the reference's per-layer table)
        cbufs = {} if (x.is_cuda and self.plan_concats) else None   # planned concat buffers of this walk
        # depth-first prefix (Model.depth_first): {first row: (i0, i1)} and the rows a segment covers
        seg_at, seg_rows, df = {}, set(), self.depth_first
        if df and x.is_cuda and not self.training and not profile and cbufs is not None and x.shape[0] >= 2 * int(df[0]) > 0:
            for sg in g.prefix_segments(df[1] if len(df) > 1 else None):
                seg_at[sg[0]] = sg
                seg_rows.update(range(sg[0], sg[1] + 1))
        on_lane = lambda i: nullcontext()      # noqa: E731
        if lanes is not None:
            main = torch.cuda.current_stream(x.device)
            side = self.__dict__.get("_side_stream")
            if side is None or side.device != x.device:
                side = self.__dict__["_side_stream"] = torch.cuda.Stream(device=x.device)
            streams, keep = (main, side), []             # keep every output alive until both lanes have joined
            on_lane = lambda i: torch.cuda.stream(streams[lanes[i]])      # noqa: E731
            side.wait_stream(main)                       # fork: the side lane starts after everything queued so far
        if profile:     # reference :252-260,270-271: per-layer time / GFLOPS / params / type.  One stream, HIP events around
            flog, prev_log, marks = [], ops._launch_log, []      # every layer, GFLOPS from the algorithmic FLOPs of its GEMM launches
            ops.set_launch_log(flog)
        y, seg_end = [], None
        try:
            for i, m in enumerate(layers):
                if i in seg_rows:                             # depth-first prefix: the whole segment runs at its first row, on its lane
                    if i in seg_at:
                        with on_lane(i):
                            x = self._run_segment(g, seg_at[i], x2 if g.image[i] else x, cbufs, int(df[0]))
                        seg_end = seg_at[i][1]
                        if lanes is not None:
                            keep.append(x)
                    y.append(x if (i == seg_end and i in self.save) else None)
                    continue
                if lanes is not None and any(lanes[j] != lanes[i] for j in g.sources[i]):
                    streams[lanes[i]].wait_stream(streams[1 - lanes[i]])
                if g.image[i] is None:
                    x = g.inputs(i, x, y)
                elif g.image[i]:
                    x = x2                           # (row 0: x is still the RGB image; no other reference to it is kept)
                if profile:
                    e0, e1, n0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), len(flog)
                    e0.record()
                with on_lane(i):
                    if i in fused:
                        x = fused.pop(i)         # produced by the group's kernel, maybe on the other lane: the cross-lane wait above orders it
                    else:
                        grp = self._fused_cft_outputs(g, m, x, y, cbufs) if fuse_cft else None
                        if grp is not None:
                            x = grp.pop(i)
                            fused.update(grp)
                        else:
                            x = self._run_layer(g, m, x, cbufs, chain=not profile)
                if profile:
                    e1.record()
                    marks.append((m, e0, e1, sum(rec[1] for rec in flog[n0:])))
                if lanes is not None:
                    keep.append(x)
                y.append(x if i in self.save else None)
        finally:
            if profile:
                ops.set_launch_log(prev_log)
        if lanes is not None:
            main.wait_stream(side)                       # join
        if profile:
            torch.cuda.synchronize(x[0].device if isinstance(x, (tuple, list)) else x.device)
            self.profile_ms = [(m.i, m.type, e0.elapsed_time(e1), fl / 1e9, m.np) for m, e0, e1, fl in marks]
            logger.info(f"{'time (ms)':>10s} {'GFLOPS':>10s} {'params':>10s}  {'module'}")
            for i, t, ms, gf, np_ in self.profile_ms:
                logger.info(f"{ms:10.2f} {gf:10.2f} {np_:10.0f}  {t}")
            logger.info('%.1fms total' % sum(r[2] for r in self.profile_ms))
        return x

    def _initialize_biases(self, cf=None):  # reference :274-282
        m = self.model[-1]
        for mi, s in zip(m.m, m.stride):
            b = mi.bias.view(m.na, -1)
            b.data[:, 4] += math.log(8 / (640 / s) ** 2)
            b.data[:, 5:] += math.log(0.6 / (m.nc - 0.99)) if cf is None else torch.log(cf / cf.sum())
            mi.bias = torch.nn.Parameter(b.view(-1), requires_grad=True)

    def _print_biases(self):  # reference :284-289
        m = self.model[-1] if isinstance(self.model[-1], Detect) else self.model[-2]
        for mi in m.m:
            b = mi.bias.detach().view(m.na, -1).T
            logger.info(("%6g Conv2d.bias:" + "%10.3g" * 6) % (mi.weight.shape[1], *b[:5].mean(1).tolist(), b[5:].mean()))

    def nms(self, mode=True):
        """Add or remove the NMS module behind ``Detect`` (reference :306-318): with it ``model(x, x2)`` returns the per-image
        detection lists.  The module runs ``cft_nms``; a captured HIP graph covers the layers in front of it."""
        present = type(self.model[-1]) is NMS
        if mode and not present:
            logger.info("Adding NMS... ")
            m = NMS()
            m.f = -1
            m.i = self.model[-1].i + 1
            m.type, m.np = "models.common.NMS", 0
            self.model.add_module(name="%s" % m.i, module=m)
            self.eval()
        elif not mode and present:
            logger.info("Removing NMS... ")
            self.model = self.model[:-1]
        self._graphs.clear()
        return self

    def autoshape(self):
        """Wrap the model for raw image input (reference :320-324); see ``models.common.autoShape`` (two-stream form)."""
        logger.info("Adding autoShape... ")
        return autoShape(self)

    def fuse(self):
        """Fold every BatchNorm into its conv (reference :296-304, utils/torch_utils.py:181-201).
        The kernels always execute the folded form, so this only changes the stored parameters
        (``conv.weight``/``conv.bias``, no ``bn``) exactly like the reference does."""
        for m in self.model.modules():
            if type(m) is Conv and hasattr(m, "bn"):
                w, b = ops.fold_bn(m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var, m.bn.eps)
                c = m.conv
                fused = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, bias=True)
                fused = fused.requires_grad_(False).to(c.weight.device)
                fused.weight.copy_(w.detach())
                fused.bias.copy_(b.detach())
                m.conv = fused
                delattr(m, "bn")
        invalidate_packed(self)
        return self

    def info(self, verbose=False, img_size=640):
        n_p = sum(x.numel() for x in self.parameters())
        logger.info(f"Model Summary: {len(list(self.modules()))} layers, {n_p} parameters")

    # ---- MI355X-specific ---------------------------------------------------------------------
    def set_compute_dtype(self, dtype):
        """bf16 (default) or fp16 - both with fp32 accumulation, fp32 CFT residual stream and fp32 logits; fp16 is
        the reference's own GPU precision and the 16-bit type that meets the 1e-2 parity bound - or
        fp32 (exact-fp32 MFMA path used for the 1e-3 tolerance configuration)."""
        if dtype not in ops.COMPUTE_DTYPES:
            raise TypeError("compute dtype must be torch.bfloat16, torch.float16 or torch.float32")
        if dtype != self.compute_dtype:
            self._graphs.clear()
        self.compute_dtype = dtype
        for m in self.modules():
            if isinstance(m, Focus):
                m.compute_dtype = dtype
        return self

    def prepare(self):
        """Pack every layer's weights for the current device/dtype now (otherwise done lazily)."""
        dev = next(self.parameters()).device
        for m in self.modules():
            if isinstance(m, _Packed):
                m._packed(self.compute_dtype, dev)
        return self

    def capture(self, batch, height, width, input_dtype=torch.float32):
        """Record the forward for a fixed input shape into a HIP graph; later ``model(x, x2)`` calls
        with that shape replay it (inputs are copied into static buffers, outputs are static
        tensors that the next replay overwrites)."""
        from ..graph import CapturedForward
        key = ((batch, 3, height, width), self.compute_dtype, input_dtype)
        self._graphs[key] = CapturedForward(self, batch, height, width, input_dtype=input_dtype)
        return self._graphs[key]

    def release_graphs(self):
        self._graphs.clear()
