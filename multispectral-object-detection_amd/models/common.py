"""Module library of the two-stream YOLOv5 + CFT detector, MI355X-native.

Drop-in for the hot-path classes of the reference's ``models/common.py`` (same class names,
constructor signatures, sub-module/parameter names and therefore state-dict keys):

    Conv :36-50   Bottleneck :99-109   C3 :131-143   SPP :154-165   Focus :168-179
    Concat :211-219   Add :222-229   Add2 :232-243
    SelfAttention :430-513   myTransformerBlock :516-546   GPT :549-639

(``file:line`` = /root/reference/models/common.py).  The parameters are ordinary fp32
``nn.Parameter``s, so ``load_state_dict`` from a reference model is loss-free; the forward of
every class, however, launches hand-written gfx950 kernels through ``libcft_hip.so`` (see
``include/cft_hip.h``) on NHWC tensors instead of calling ATen:

* Conv        one implicit-GEMM kernel with BatchNorm folded in and bias+SiLU fused;
* Bottleneck  the residual add is the epilogue of its 3x3 conv;
* C3          cv1|cv2 run as ONE GEMM into the concat buffer, the bottleneck chain ends in the
              same buffer, so ``torch.cat`` disappears;
* SPP         cv1 writes slice 0 of the 4-way concat buffer, one kernel fills the 3 pooled slices;
* GPT         fp32 residual stream, LayerNorm -> fused QKV GEMM -> single-tile MFMA attention ->
              out-proj(+residual) -> LayerNorm -> fc1(+GELU) -> fc2(+residual); the bilinear
              upsampling is deferred and fused with the Add2 that consumes it.

``model.eval()`` (the default, the benchmarked path): BatchNorm folded into the conv weights, dropout the identity.
``model.train()``: the training-mode FORWARD of the reference: BatchNorm with batch
statistics and running-stat updates (``cft_batchnorm_train`` after an un-folded conv), dropout in GPT / SelfAttention /
MLP (``cft_dropout``, counter-based masks), ``Detect`` returning the raw list.  No autograd graph is built.
"""
import math
from collections import namedtuple

import torch
import torch.nn as nn

from .. import ops
from ..ops import ACT_GELU, ACT_NONE, ACT_SILU

BN_EPS = 1e-3  # reference utils/torch_utils.py:150 (initialize_weights)


def autopad(k, p=None):  # reference models/common.py:24-28
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


# ------------------------------------------------------------------------------ lazy tensors
class _Pending:
    """A value whose producing kernel is deferred so that the consumer can fuse it."""

    def materialize(self):
        raise NotImplementedError


class PendingBilinear(_Pending):
    """GPT output stream ``s``: bilinear(tokens va x ha -> HxW), ``grid`` = (va, ha).  ``Add2`` fuses it with its add."""

    def __init__(self, tokens, s, H, W, dtype, grid=ops.ANCHOR_GRID):
        self.tokens, self.s, self.H, self.W, self.dtype, self.grid = tokens, s, H, W, dtype, tuple(grid)

    def materialize(self, base=None):
        return ops.gpt_upsample_add(self.tokens, self.s, base, self.H, self.W, self.dtype, grid=self.grid)

    @property
    def shape(self):
        return torch.Size((self.tokens.shape[0], self.tokens.shape[2], self.H, self.W))


class PendingUpsample(_Pending):
    """nearest 2^up upsampling of ``x``; ``Concat`` writes it straight into its buffer."""

    def __init__(self, x, up):
        self.x, self.up = x, up

    def materialize(self):
        B, C, H, W = self.x.shape
        out = ops.new_nhwc(B, H << self.up, W << self.up, C, self.x.dtype, self.x.device)
        return ops.copy_channels(self.x, out, self.up)

    @property
    def shape(self):
        B, C, H, W = self.x.shape
        return torch.Size((B, C, H << self.up, W << self.up))


class PendingConv(_Pending):
    """Output of a ``Conv`` whose only consumer is the ``C3`` behind it (``Model.chain_plan``): that C3 runs the conv and its own
    packed cv1|cv2 as ONE kernel (``ops.conv2d_chain``) when the pair is eligible, and the conv's output tensor never exists."""

    def __init__(self, conv, x):
        self.conv, self.x = conv, x

    def materialize(self):
        return self.conv(self.x)

    @property
    def shape(self):
        B, _, H, W = self.x.shape
        return torch.Size((B, self.conv.conv.out_channels, *ops.conv_out_size(H, W, self.conv.conv.kernel_size[0], self.conv.conv.stride[0])))


def resolve(x):
    return x.materialize() if isinstance(x, _Pending) else x


def _cache_key(module, dtype, device):
    """Identity of the packed weights: dtype, device and, per parameter/buffer, (storage address, in-place
    version).  ``load_state_dict``, ``.to()``, ``.half()`` and optimiser-style in-place updates all change it;
    edits through ``tensor.data`` do not bump ``_version`` - call ``invalidate_packed`` after those."""
    vers = tuple((int(p.data_ptr()), int(p._version)) for p in module.parameters()) \
        + tuple((int(b.data_ptr()), int(b._version)) for b in module.buffers())
    return (dtype, str(device), vers)


def invalidate_packed(root):
    """Drop the kernel-side weight copies of every module under ``root`` (they are rebuilt on the next forward)
    and, if ``root`` owns captured HIP graphs, those too - a graph replays the weight buffers it was captured
    with."""
    for m in root.modules():
        m.__dict__.pop("_cft_cache", None)
        m.__dict__.pop("_cft_cache_train", None)
        m.__dict__.pop("_plan_cache", None)
        if "_graphs" in m.__dict__:
            m.__dict__["_graphs"].clear()
        m.__dict__.pop("_wlist", None)


class _Packed(nn.Module):
    """Mixin: lazily packed kernel-side weights, rebuilt when dtype/device/parameters change."""

    def _packed(self, dtype, device, train=False):
        """Kernel-side weights for the inference form (BatchNorm folded) or, ``train=True``, the training form
        (``_pack_train``: un-folded conv weights)."""
        key = (train,) + _cache_key(self, dtype, device)
        slot = "_cft_cache_train" if train else "_cft_cache"
        cache = self.__dict__.get(slot)
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key, self._pack_train(dtype, device) if train else self._pack(dtype, device))
            self.__dict__[slot] = cache
        return cache[1]

    def _pack_train(self, dtype, device):
        raise NotImplementedError(f"{type(self).__name__} has no training-mode form")

    def _pack(self, dtype, device):
        raise NotImplementedError


def _folded(conv_module):
    """(weight, bias) of a Conv with BatchNorm folded, or of an already fused conv."""
    conv = conv_module.conv
    if hasattr(conv_module, "bn"):
        bn = conv_module.bn
        return ops.fold_bn(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    bias = conv.bias.float() if conv.bias is not None else torch.zeros(conv.out_channels, device=conv.weight.device)
    return conv.weight.float(), bias


def _f32(t, device):
    """Contiguous fp32 device copy of a parameter/buffer that a kernel reads through a raw float pointer."""
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _act_code(act):
    if isinstance(act, nn.SiLU):
        return ACT_SILU
    if isinstance(act, nn.Identity):
        return ACT_NONE
    raise NotImplementedError(f"activation {type(act).__name__} has no fused epilogue (SiLU / Identity only)")


# ------------------------------------------------------------------------------ Conv family
class Conv(_Packed):
    """Standard convolution: SiLU(BN(conv(x))) (reference models/common.py:36-50)."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        if g != 1:
            raise NotImplementedError("grouped convolution is not used by any CFT config")
        if autopad(k, p) != k // 2:
            raise NotImplementedError("only 'same' padding (k//2) is implemented")
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=BN_EPS, momentum=0.03)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())

    def _pack(self, dtype, device, cin_pad=None):
        w, b = _folded(self)
        return ops.pack_conv(w, b, dtype, s=self.conv.stride[0], cin_pad=cin_pad or self.cin_pad, device=device)

    cin_pad = None      # Focus sets 16 on its inner Conv (space-to-depth output is padded to 16 channels)

    def _pack_train(self, dtype, device):
        return ops.pack_conv(self.conv.weight.float(), None, dtype, s=self.conv.stride[0], cin_pad=self.cin_pad, device=device)

    def forward(self, x, residual=None, out=None):
        x = resolve(x)
        if self.training and hasattr(self, "bn") and self.bn.training:
            # act(bn(conv(x))) with batch statistics (reference :45-47): fp32 conv output, then cft_batchnorm_train
            pk = self._packed(x.dtype, x.device, train=True)
            y32 = ops.conv2d(x, pk, ACT_NONE, out_dtype=torch.float32)
            return ops.batchnorm_train(y32, pk.n_valid, self.bn, _act_code(self.act), residual=residual, out=out, out_dtype=x.dtype)
        return ops.conv2d(x, self._packed(x.dtype, x.device), _act_code(self.act), residual=residual, out=out)

    fuseforward = forward  # the kernel always runs the folded form (reference :49-50)


class Bottleneck(nn.Module):
    """x + cv2(cv1(x)) (reference models/common.py:99-109); the add is cv2's epilogue."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2

    def forward(self, x, out=None):
        x = resolve(x)
        if x.is_cuda and not self.training:
            a1, a2 = _act_code(self.cv1.act), _act_code(self.cv2.act)
            pk1, pk2 = self.cv1._packed(x.dtype, x.device), self.cv2._packed(x.dtype, x.device)
            aliased = out is not None and out.data_ptr() == x.data_ptr()   # in-place: the fused kernel reads a halo of x
            if ops.bottleneck_fusable(x, pk1, pk2, a1, a2) and not aliased:
                return ops.bottleneck(x, pk1, pk2, self.add, out=out)      # 64-channel stage: one kernel, no hidden tensor
        return self.cv2(self.cv1(x), residual=x if self.add else None, out=out)


# C3.launch_plan.  front: "chained" (the Conv handed over and cv1|cv2 as one ops.conv2d_chain kernel), "separate" (that conv, then cv1|cv2) or
# None (no conv was handed over); split: cv1 and cv2 as two launches (training); steps: (form, j) over the Bottlenecks m[j], with y the
# input (and shortcut) of the current Bottleneck and h its cv1 output:
#   "block"     y = m[j](y)                               the Bottleneck's own forward (it picks the patch-resident kernel where it can)
#   "cv1"       h = m[j].cv1(y)
#   "cv2"       y = m[j].cv2(h) (+ y)                     the last one writes the concat buffer's first half
#   "pair"      h = m[j + 1].cv1(m[j].cv2(h))             one kernel (ops.conv2d_chain); neither Bottleneck has a shortcut
#   "pair_res"  y = m[j].cv2(h) + y; h = m[j + 1].cv1(y)  one kernel (ops.conv2d_chain_res)
C3Plan = namedtuple("C3Plan", "front split steps")


class C3(_Packed):
    """CSP bottleneck with 3 convolutions (reference models/common.py:131-143):
    cv3(cat(m(cv1(x)), cv2(x))).  cv1 and cv2 read the same input, so they run as one GEMM whose
    output IS the concat buffer; the last Bottleneck writes its result back into the first half."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*[Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)])

    def _pack(self, dtype, device):
        w1, b1 = _folded(self.cv1)
        w2, b2 = _folded(self.cv2)
        return ops.pack_conv(torch.cat([w1, w2], 0), torch.cat([b1, b2], 0), dtype, device=device)

    chain = True                   # Model.chain_convs switches it (A/B)
    chain_pairs = True             # the Bottleneck-pair chains (3x3 of Bottleneck j + 1x1 of Bottleneck j + 1) on their own (Model.chain_pairs; bench.py --no-pair-chain)

    def launch_plan(self, B, H, W, dtype, front=None, ld_in=None):
        """The ``C3Plan`` of a forward on a [B, *, H, W] tensor of ``dtype`` with ``ld_in`` channels per pixel (None: dense); ``front``: the
        ``Conv`` left to this C3 as a ``PendingConv`` - the tensor is then THAT conv's input.  Decided from the geometry and the packed
        weights' shapes alone (a CPU-resident module answers too) and cached: the key holds everything the decision reads."""
        key = (front, B, H, W, ld_in, dtype, self.training, self.chain, self.chain_pairs, ops.CHAIN_RES_MIN_ROWS)
        cache = self.__dict__.setdefault("_plan_cache", {})          # (invalidate_packed drops it)
        if key not in cache:
            if len(cache) > 16:
                cache.clear()
            cache[key] = self._plan(B, H, W, dtype, front, ld_in)
        return cache[key]

    def _plan(self, B, H, W, dtype, front, ld_in):
        n = len(self.m)
        blocks = tuple(("block", j) for j in range(n))
        if self.training:        # batch statistics are per BatchNorm: cv1 and cv2 run separately into the concat buffer
            return C3Plan(None if front is None else "separate", True, blocks)
        dev = self.cv1.conv.weight.device
        how = None
        if front is not None:    # chained: SiLU and a pair cft_conv2d_chain_ok takes with the source's real ld
            ok = _act_code(front.act) == ACT_SILU and ops.conv2d_chain_ok_geometry(B, H, W, dtype, front._packed(dtype, dev), self._packed(dtype, dev), ldx=ld_in)
            how = "chained" if ok else "separate"
            H, W = ops.conv_out_size(H, W, front.conv.kernel_size[0], front.conv.stride[0])
        if not (self.chain and self.chain_pairs and n >= 2 and dtype in (torch.bfloat16, torch.float16)):
            return C3Plan(how, False, blocks)
        pks = [(b.cv1._packed(dtype, dev), b.cv2._packed(dtype, dev)) for b in self.m]
        acts = [(_act_code(b.cv1.act), _act_code(b.cv2.act)) for b in self.m]
        # 64 / 128 channels: the patch-resident kernel of Bottleneck.forward is the better fusion, such a Bottleneck is never chained
        y = torch.empty((B, self.cv1.conv.out_channels, H, W), dtype=dtype, device="meta")       # (its shape and type are all that is read)
        own = [ops.bottleneck_fusable(y, *pk, *act) for pk, act in zip(pks, acts)]
        # WITH shortcuts (backbone C3s, 256 channels): Bottleneck j's output is the next shortcut AND the input of Bottleneck j + 1's 1x1 -
        # cv2[j] (+ shortcut) and cv1[j + 1] run as one launch: n + 1 launches instead of 2 n, no re-read of y.  All pairs or none; h and
        # y1 are dense tensors of this pixel grid
        if (all(b.add for b in self.m) and all(a == (ACT_SILU, ACT_SILU) for a in acts) and not any(own)
                and all(ops.conv2d_chain_res_ok_geometry(B, H, W, dtype, pks[j][1], pks[j + 1][0]) for j in range(n - 1))):
            return C3Plan(how, False, (("cv1", 0),) + tuple(("pair_res", j) for j in range(n - 1)) + (("cv2", n - 1),))
        # Without shortcuts a Bottleneck's output has ONE reader, the next Bottleneck's 1x1 (reference models/common.py:108-109, :142): cv2[j] +
        # cv1[j + 1] then run as one launch and the tensor between the two Bottlenecks never exists.  Decided pair by pair
        can = [j + 1 < n and not (self.m[j].add or self.m[j + 1].add or own[j]) and acts[j][1] == ACT_SILU
               and ops.conv2d_chain_ok_geometry(B, H, W, dtype, pks[j][1], pks[j + 1][0]) for j in range(n)]
        steps = []
        for j in range(n):
            entered = j > 0 and can[j - 1]          # cv1[j] already ran, in the chained launch of Bottleneck j - 1
            if entered or can[j]:
                steps += ([] if entered else [("cv1", j)]) + [("pair" if can[j] else "cv2", j)]
            else:
                steps.append(("block", j))
        return C3Plan(how, False, tuple(steps))

    def forward(self, x, out=None):
        c_ = self.cv1.conv.out_channels
        act = _act_code(self.cv1.act)
        if act != _act_code(self.cv2.act):
            raise NotImplementedError("C3.cv1 and C3.cv2 must share an activation")
        front = x.conv if isinstance(x, PendingConv) else None
        x = resolve(x.x if front is not None else x)
        B, _, H, W = x.shape
        dt, dev = x.dtype, x.device
        plan = self.launch_plan(B, H, W, dt, front, x.stride(3) if (x.stride(1) == 1 and x.stride(3) >= x.shape[1]) else None)
        if plan.front == "chained":
            cat = ops.conv2d_chain(x, front._packed(dt, dev), self._packed(dt, dev), act)    # one kernel for the Conv in front and cv1|cv2
        else:
            if front is not None:
                x = front(x)
            if plan.split:
                B, _, H, W = x.shape
                cat = ops.new_nhwc(B, H, W, 2 * c_, dt, dev)
                self.cv1(x, out=cat[:, :c_])
                self.cv2(x, out=cat[:, c_:])
            else:
                cat = ops.conv2d(x, self._packed(dt, dev), act)     # [B, 2c_, H, W]
        head = cat[:, :c_]
        y, h, last = head, None, len(self.m) - 1
        for form, j in plan.steps:
            blk, dst = self.m[j], (head if j == last else None)
            if form == "block":
                y = blk(y, out=dst)
            elif form == "cv1":
                h = blk.cv1(y)
            elif form == "cv2":
                y = blk.cv2(h, residual=y if blk.add else None, out=dst)
            else:
                nxt = self.m[j + 1].cv1
                pk2, pk1, act1 = blk.cv2._packed(dt, dev), nxt._packed(dt, dev), _act_code(nxt.act)
                if form == "pair":
                    h = ops.conv2d_chain(h, pk2, pk1, act1)
                else:
                    y, h = ops.conv2d_chain_res(h, pk2, y, pk1, act1)
        return self.cv3(cat, out=out)


class SPP(nn.Module):
    """Spatial pyramid pooling (reference models/common.py:154-165)."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * (len(k) + 1), c2, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])
        self.k = tuple(k)

    def forward(self, x):
        x = resolve(x)
        ks = tuple(int(mp.kernel_size) for mp in self.m)   # (not self.k: un-pickled reference modules lack it)
        if len(ks) != 3 or list(ks) != sorted(ks):
            raise NotImplementedError("SPP kernel implements exactly three ascending pooling sizes")
        c_ = self.cv1.conv.out_channels
        B, _, H, W = x.shape
        cat = ops.new_nhwc(B, H, W, 4 * c_, x.dtype, x.device)
        self.cv1(x, out=cat[:, :c_])
        ops.spp_maxpool(cat, c_, ks)
        return self.cv2(cat)


class Focus(_Packed):
    """Focus wh information into c-space (reference models/common.py:168-179): 2x2 space-to-depth
    then Conv.  Takes the fp32 image batch [B,3,H,W] (NCHW) and emits NHWC activations in
    ``compute_dtype`` - this module is where the compute precision of the whole network is set."""

    compute_dtype = None   # None: the precision of the parameters (fp32 -> exact fp32 path, .half() -> fp16), like torch;
                           # Model.set_compute_dtype() sets it explicitly (its default is bf16)

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = Conv(c1 * 4, c2, k, s, p, g, act)
        self.conv.cin_pad = 16

    def _pack(self, dtype, device):
        if self.conv.conv.in_channels != 12:
            raise NotImplementedError("Focus kernel is specialised for 3-channel images")
        return self.conv._pack(dtype, device, cin_pad=16)

    def forward(self, x):
        x = resolve(x)
        dtype = self.compute_dtype or self.conv.conv.weight.dtype
        if self.training:      # space-to-depth, then the Conv's training form (batch statistics)
            self.conv.cin_pad = 16
            return self.conv(ops.focus_s2d(x, dtype))
        return ops.focus_conv(x, self._packed(dtype, x.device), _act_code(self.conv.act), dtype)


class Upsample(nn.Upsample):
    """``nn.Upsample(None, 2, 'nearest')`` of the head (yaml rows 33/37).  Returns a deferred value
    that ``Concat`` writes directly into its buffer."""

    def forward(self, x):
        x = resolve(x)
        sf = self.scale_factor
        if self.mode != "nearest" or self.size is not None or float(sf) not in (2.0, 4.0, 8.0):
            raise NotImplementedError("only nearest-neighbour upsampling by 2/4/8 is implemented")
        return PendingUpsample(x, int(math.log2(float(sf))))


class Concat(nn.Module):
    """Channel concatenation (reference models/common.py:211-219)."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension

    def forward(self, x, out=None):
        """``out``: a pre-allocated concat buffer (Model's concat plan); sources that their producer already wrote
        into their slice of it are not copied again."""
        if self.d != 1:
            raise NotImplementedError("Concat is implemented along channels only")
        shapes = [t.shape for t in x]
        B, _, H, W = shapes[0]
        first = x[0].x if isinstance(x[0], PendingUpsample) else resolve(x[0])
        total = sum(s[1] for s in shapes)
        if out is None:
            out = ops.new_nhwc(B, H, W, total, first.dtype, first.device)
        elif tuple(out.shape) != (B, total, H, W):
            raise ValueError(f"Concat: planned buffer {tuple(out.shape)} does not match the inputs {(B, total, H, W)}")
        off = 0
        for t, s in zip(x, shapes):
            dst = out[:, off:off + s[1]]
            if isinstance(t, PendingUpsample):
                ops.copy_channels(t.x, dst, t.up)
            else:
                t = resolve(t)
                if not (t.data_ptr() == dst.data_ptr() and t.stride() == dst.stride()):   # else: already in place
                    ops.copy_channels(t, dst, 0)
            off += s[1]
        return out


class Add(nn.Module):
    """Sum of two feature maps (reference models/common.py:222-229)."""

    def __init__(self, arg):
        super().__init__()
        self.arg = arg

    def forward(self, x, out=None):
        return ops.add(resolve(x[0]), resolve(x[1]), out=out)


class Add2(nn.Module):
    """x[0] + transformer_output[index] (reference models/common.py:232-243); when the transformer
    output is still deferred the bilinear upsampling and the add are one kernel."""

    def __init__(self, c1, index):
        super().__init__()
        self.index = index

    def forward(self, x):
        if self.index not in (0, 1):
            raise ValueError("Add2 index must be 0 or 1")
        base, t = resolve(x[0]), x[1][self.index]
        if isinstance(t, PendingBilinear):
            return t.materialize(base)
        return ops.add(base, resolve(t))


# ------------------------------------------------------------------------------ CFT block
class _ResidualStream:
    """The fp32 residual stream ``x`` [rows, d] of the CFT blocks (``dtype``: what the GEMMs compute in).  It is updated in place by the
    epilogue of the GEMM that adds to it - or, where ``split`` allows (each block sets it from its own switch: inference on the GPU) and
    ``ops.splitk_choice`` splits that GEMM, the fp32 partial sums [s, rows, d] stay ``pending`` and the next LayerNorm folds them in, in a
    fixed order (``ops.layernorm_reduce``: the next block's ln_input, or ln_f)."""

    def __init__(self, x, dtype):
        self.x, self.dtype, self.split, self.pending = x, dtype, False, None

    def norm(self, gamma, beta, eps, out_dtype):
        """LayerNorm(x) in ``out_dtype``, after folding what is pending into x."""
        parts, self.pending = self.pending, None
        if parts is not None:
            return ops.layernorm_reduce(self.x, parts, gamma, beta, out_dtype, eps)
        return ops.layernorm(self.x, gamma, beta, out_dtype, eps)

    def add_linear(self, inp, pk, drop_p=0.0):
        """x += dropout(linear(inp, pk))."""
        if drop_p > 0:
            z = ops.linear(inp, pk, out_dtype=torch.float32)
            ops.dropout_(z, drop_p)
            ops.add_rows_(self.x, z)
        elif self.split and (splits := ops.splitk_choice(inp.shape[0], pk, inp.dtype)) > 1:
            self.pending = ops.linear_splitk(inp, pk, splits)
        else:
            ops.linear(inp, pk, residual=self.x, out=self.x, out_dtype=torch.float32)


class SelfAttention(_Packed):
    """Multi-head self-attention (reference models/common.py:430-513).  q/k/v projections run as
    one GEMM; heads are laid out at a padded width ``dkp`` so the attention kernel needs no tails."""

    def __init__(self, d_model, d_k, d_v, h, attn_pdrop=.1, resid_pdrop=.1):
        super().__init__()
        assert d_k % h == 0
        self.d_model = d_model
        self.d_k = d_model // h
        self.d_v = d_model // h
        self.h = h
        self.que_proj = nn.Linear(d_model, h * self.d_k)
        self.key_proj = nn.Linear(d_model, h * self.d_k)
        self.val_proj = nn.Linear(d_model, h * self.d_v)
        self.out_proj = nn.Linear(h * self.d_v, d_model)
        self.attn_drop = nn.Dropout(attn_pdrop)
        self.resid_drop = nn.Dropout(resid_pdrop)
        for m in (self.que_proj, self.key_proj, self.val_proj, self.out_proj):  # reference :459-473
            nn.init.normal_(m.weight, std=0.001)
            nn.init.constant_(m.bias, 0)

    @staticmethod
    def padded_head(dk, dtype):
        step = 16 if dtype == torch.float32 else 32
        return ((dk + step - 1) // step) * step

    def _pack(self, dtype, device):
        h, dk, d = self.h, self.d_k, self.d_model
        dkp = self.padded_head(dk, dtype)
        ws, bs = [], []
        for lin in (self.que_proj, self.key_proj, self.val_proj):
            w = torch.zeros((h, dkp, d), dtype=torch.float32, device=device)
            b = torch.zeros((h, dkp), dtype=torch.float32, device=device)
            w[:, :dk] = lin.weight.detach().float().to(device).view(h, dk, d)
            b[:, :dk] = lin.bias.detach().float().to(device).view(h, dk)
            ws.append(w.view(h * dkp, d))
            bs.append(b.view(h * dkp))
        qkv = ops.pack_conv(torch.cat(ws, 0), torch.cat(bs, 0), dtype, device=device, n_true=3 * h * dk)
        wo = torch.zeros((d, h, dkp), dtype=torch.float32, device=device)
        wo[:, :, :dk] = self.out_proj.weight.detach().float().to(device).view(d, h, dk)
        out = ops.pack_conv(wo.view(d, h * dkp), self.out_proj.bias, dtype, device=device)
        out.flops_per_row = 2.0 * d * h * dk
        return qkv, out, dkp

    def forward(self, x, attention_mask=None, attention_weights=None, stream=None, ntok=128):
        """x: [B*ntok, d] in the compute dtype (``ntok`` tokens per image: 2 * vert_anchors * horz_anchors of the GPT).  Returns out_proj(attn); with
        ``stream`` (the transformer block's ``_ResidualStream``) resid_drop(out_proj(attn)) is added to the stream instead and nothing is returned."""
        if attention_mask is not None or attention_weights is not None:
            raise NotImplementedError("attention_mask / attention_weights are unused by GPT (reference :497-500)")
        qkv_w, out_w, dkp = self._packed(x.dtype, x.device)
        B = x.shape[0] // ntok
        qkv = ops.linear(x, qkv_w)
        att = ops.attention(qkv, B, self.h, self.d_k, dkp, pdrop=self.attn_drop.p if self.training else 0.0, T=ntok)
        if stream is None:
            return ops.linear(att, out_w)
        stream.add_linear(att, out_w, self.resid_drop.p if self.training else 0.0)


class myTransformerBlock(_Packed):
    """Pre-LN transformer block (reference models/common.py:516-546).  ``x`` is the fp32 residual
    stream [B*ntok, d]; it is updated in place by the two GEMM epilogues."""

    def __init__(self, d_model, d_k, d_v, h, block_exp, attn_pdrop, resid_pdrop):
        super().__init__()
        self.ln_input = nn.LayerNorm(d_model)
        self.ln_output = nn.LayerNorm(d_model)
        self.sa = SelfAttention(d_model, d_k, d_v, h, attn_pdrop, resid_pdrop)
        self.mlp = nn.Sequential(
            nn.Linear(d_model, block_exp * d_model),
            nn.GELU(),
            nn.Linear(block_exp * d_model, d_model),
            nn.Dropout(resid_pdrop),
        )

    def _pack(self, dtype, device):
        fc1 = ops.pack_conv(self.mlp[0].weight, self.mlp[0].bias, dtype, device=device)
        fc2 = ops.pack_conv(self.mlp[2].weight, self.mlp[2].bias, dtype, device=device)
        ln = [_f32(t, device) for t in (self.ln_input.weight, self.ln_input.bias, self.ln_output.weight, self.ln_output.bias)]
        return fc1, fc2, ln

    splitk = True        # inference: out_proj / fc2 as split-K GEMMs where ops.splitk_choice splits them (GPT.splitk switches all blocks; A/B)

    def forward(self, stream, ntok=128):
        """x += sa(LN(x)); x += mlp(LN(x)) on the ``_ResidualStream`` of ``GPT.forward``."""
        fc1, fc2, ln = self._packed(stream.dtype, stream.x.device)
        stream.split = self.splitk and not self.training and stream.x.is_cuda
        self.sa(stream.norm(ln[0], ln[1], self.ln_input.eps, stream.dtype), stream=stream, ntok=ntok)
        hid = ops.linear(stream.norm(ln[2], ln[3], self.ln_output.eps, stream.dtype), fc1, act=ACT_GELU)
        stream.add_linear(hid, fc2, self.mlp[3].p if (self.training and len(self.mlp) > 3) else 0.0)


class GPT(_Packed):
    """Cross-modality fusion transformer (reference models/common.py:549-639)."""

    def __init__(self, d_model, h=8, block_exp=4, n_layer=8, vert_anchors=8, horz_anchors=8,
                 embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1):
        super().__init__()
        self.n_embd = d_model
        self.vert_anchors = vert_anchors
        self.horz_anchors = horz_anchors
        d_k = d_model
        d_v = d_model
        self.pos_emb = nn.Parameter(torch.zeros(1, 2 * vert_anchors * horz_anchors, self.n_embd))
        self.trans_blocks = nn.Sequential(*[myTransformerBlock(d_model, d_k, d_v, h, block_exp, attn_pdrop, resid_pdrop)
                                            for _ in range(n_layer)])
        self.ln_f = nn.LayerNorm(self.n_embd)
        self.drop = nn.Dropout(embd_pdrop)
        self.avgpool = nn.AdaptiveAvgPool2d((self.vert_anchors, self.horz_anchors))
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(module):  # reference :582-591
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    def _pack(self, dtype, device):   # fp32 copies of what the kernels read through raw pointers (fp16 after model.half())
        return _f32(self.pos_emb, device), _f32(self.ln_f.weight, device), _f32(self.ln_f.bias, device)

    def check_supported(self, C=None):
        """Raise NotImplementedError, naming the limit, for a configuration outside what the kernels take: 1 <= vert_anchors,
        horz_anchors, vert_anchors * horz_anchors <= 1024 (T <= 2048 tokens), head width d_model / h <= 256, and (grids other than the
        8 x 8 default) d_model <= 2048."""
        grid = (int(self.vert_anchors), int(self.horz_anchors))
        if grid != (self.vert_anchors, self.horz_anchors):
            raise NotImplementedError(f"anchor grid {self.vert_anchors}x{self.horz_anchors}: vert_anchors / horz_anchors must be integers")
        ops._grid(grid)
        blk = self.trans_blocks[0] if len(self.trans_blocks) else None
        if blk is not None and blk.sa.d_k > 256:
            raise NotImplementedError(f"GPT head width d_model / h = {blk.sa.d_k}: the attention kernels take head widths <= 256")
        C = self.n_embd if C is None else C
        if grid != ops.ANCHOR_GRID and C > 2048:
            raise NotImplementedError(f"GPT d_model = {C} on a {grid[0]}x{grid[1]} anchor grid: the kernels take d_model <= 2048")
        return grid

    def forward(self, x):
        grid = self.check_supported()
        T = 2 * grid[0] * grid[1]
        rgb, ir = resolve(x[0]), resolve(x[1])
        assert rgb.shape[0] == ir.shape[0]
        if rgb.shape != ir.shape or rgb.dtype != ir.dtype:
            raise ValueError("GPT: the two streams must have the same shape and dtype")
        B, C, H, W = rgb.shape
        dtype = rgb.dtype
        pos_emb, lnf_w, lnf_b = self._packed(dtype, rgb.device)
        tok = ops.gpt_tokenize(rgb, ir, pos_emb, grid=grid)      # fp32 [B,T,C], pos_emb added
        if self.training:
            ops.dropout_(tok, self.drop.p)                       # self.drop(pos_emb + token_embeddings), reference :611
        stream = _ResidualStream(tok.view(B * T, C), dtype)
        for blk in self.trans_blocks:
            blk(stream, ntok=T)
        tok_f = stream.norm(lnf_w, lnf_b, self.ln_f.eps, torch.float32).view(B, T, C)
        tok_f.anchor_grid = grid                                 # ops.token_grid: the consumers (Model's fused dual de-tokeniser) read it
        return PendingBilinear(tok_f, 0, H, W, dtype, grid), PendingBilinear(tok_f, 1, H, W, dtype, grid)


# ------------------------------------------------------------------------------ names outside the hot path
# The reference's graph file does ``from models.common import *`` and names these classes in its parse_model
# membership tests (models/yolo_test.py:496-531), so they must EXIST for that file to run over this module
# (strict form); no CFT / two-stream yaml instantiates them (SURVEY.md 2, rows marked OUT).
def _outside(name, where):
    def __init__(self, *a, **k):
        raise NotImplementedError(f"{name} (reference {where}) is outside the two-stream CFT hot path; "
                                  "no fusion yaml uses it (SURVEY.md section 2)")
    return type(name, (nn.Module,), {"__init__": __init__, "__doc__": f"Placeholder for the reference's {name} ({where})."})


def DWConv(c1, c2, k=1, s=1, act=True):  # reference models/common.py:31-33 (depthwise: grouped conv, not in any CFT yaml)
    raise NotImplementedError("DWConv (grouped convolution) is outside the two-stream CFT hot path")


TransformerLayer = _outside("TransformerLayer", "models/common.py:53-67")
TransformerBlock = _outside("TransformerBlock", "models/common.py:70-96")
BottleneckCSP = _outside("BottleneckCSP", "models/common.py:112-128")
C3TR = _outside("C3TR", "models/common.py:146-151")
Contract = _outside("Contract", "models/common.py:183-194")
Expand = _outside("Expand", "models/common.py:197-208")


class NMS(nn.Module):
    """Non-maximum-suppression module (reference models/common.py:247-257): what ``Model.nms()`` appends behind ``Detect``.
    ``forward(x)`` takes Detect's ``(pred, raw)`` and returns the per-image detection list of ``non_max_suppression`` -
    here ONE batched HIP kernel (``cft_nms``) instead of a Python loop around ``torchvision.ops.nms``."""
    conf = 0.25      # confidence threshold
    iou = 0.45       # IoU threshold
    classes = None   # (optional list) filter by class

    def forward(self, x):
        from ..utils.general import non_max_suppression
        return non_max_suppression(x[0], conf_thres=self.conf, iou_thres=self.iou, classes=self.classes)


class autoShape(nn.Module):
    """Input-robust wrapper (reference models/common.py:260-327) in the TWO-STREAM form the reference never finished: its
    ``autoShape.forward`` hands ONE image batch to a ``Model`` whose ``forward(x, x2)`` needs two (the call raises for every
    fusion yaml).  Here ``forward(rgb, ir, size=640)`` takes, per stream, one image or a list of images - HWC uint8 numpy arrays or
    tensors in RGB order (``cv2.imread(...)[:, :, ::-1]``, ``np.asarray(PIL.Image)``), or CHW - or two ready BCHW float tensors
    (passed straight to the model like the reference does, :283-285).  Pre-processing follows :288-309 (common inference
    shape = the largest scaled image rounded up to the stride, ``letterbox(auto=False)``, BHWC -> BCHW, / 255) with the letterbox on
    the device (``cft_letterbox_u8``) and the / 255 fused into Focus; post-processing :317-320 (``non_max_suppression`` =
    ``cft_nms``, ``scale_coords`` back to every original image).  Returns the list of per-image ``[n, 6]`` (xyxy, conf, cls)
    tensors in ORIGINAL-image pixels; with ``detections=True`` that list wrapped in ``Detections`` (below), as the reference returns it."""
    conf = 0.25
    iou = 0.45
    classes = None

    def __init__(self, model):
        super().__init__()
        self.model = model.eval()
        for k in ("yaml", "nc", "hyp", "names", "stride"):          # copy_attr(m, self, include=(...)) of reference :312-313
            if hasattr(model, k):
                setattr(self, k, getattr(model, k))

    def autoshape(self):
        return self      # already wrapped (reference :271-273)

    @staticmethod
    def _hwc_u8(im, device):
        import numpy as np
        if isinstance(im, torch.Tensor):
            t = im
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(im)))
        if t.dim() == 2:
            t = t[:, :, None].expand(-1, -1, 3)
        if t.shape[0] < 5:                                          # CHW -> HWC (reference :298-299)
            t = t.permute(1, 2, 0)
        t = t[:, :, :3]
        if t.dtype != torch.uint8:
            raise TypeError("autoShape: images must be uint8 (or pass two BCHW float tensors)")
        return t.contiguous().to(device)

    @torch.no_grad()
    def forward(self, rgb, ir, size=640, augment=False, profile=False, detections=False):
        from ..models.yolo_test import make_divisible
        from ..utils.datasets import letterbox
        from ..utils.general import non_max_suppression, scale_coords
        p = next(self.model.parameters())
        if isinstance(rgb, torch.Tensor) and rgb.dim() == 4:        # ready batches: straight to the model
            return self.model(rgb.to(p.device), ir.to(p.device), augment, profile)
        rgbs = list(rgb) if isinstance(rgb, (list, tuple)) else [rgb]
        irs = list(ir) if isinstance(ir, (list, tuple)) else [ir]
        if len(rgbs) != len(irs):
            raise ValueError("autoShape: the two streams must hold the same number of images")
        rgbs = [self._hwc_u8(im, p.device) for im in rgbs]
        irs = [self._hwc_u8(im, p.device) for im in irs]
        shape0 = [tuple(int(v) for v in im.shape[:2]) for im in rgbs]
        if any(tuple(b.shape[:2]) != s for b, s in zip(irs, shape0)):
            raise ValueError("autoShape: an RGB / IR pair must have the same height and width (aligned pairs)")
        smax = int(self.stride.max()) if hasattr(self, "stride") else 32
        shape1 = [max(s[d] * (size / max(s)) for s in shape0) for d in (0, 1)]
        shape1 = [make_divisible(v, smax) for v in shape1]          # one inference shape for the batch (:304)
        n = len(rgbs)
        batch = torch.empty((n, 6, shape1[0], shape1[1]), dtype=torch.uint8, device=p.device)
        for i in range(n):                                          # BGR->RGB flip is not wanted here (inputs are RGB): HWC out, then permute
            a, _, _ = letterbox(rgbs[i], new_shape=shape1, auto=False)
            b, _, _ = letterbox(irs[i], new_shape=shape1, auto=False)
            batch[i, :3] = a.permute(2, 0, 1)
            batch[i, 3:] = b.permute(2, 0, 1)
        y = self.model(batch[:, :3], batch[:, 3:])[0]               # uint8 views: Focus normalises (/255) while it reads
        y = non_max_suppression(y, conf_thres=self.conf, iou_thres=self.iou, classes=self.classes)
        for i in range(n):
            scale_coords(shape1, y[i][:, :4], shape0[i])
        if detections:
            files = [f"image{i}.jpg" for i in range(n)]
            return Detections(rgbs, y, files, names=getattr(self, "names", None), shape=tuple(batch[:, :3].shape), imgs_ir=irs)
        return y


class Detections:
    """The reference's ``Detections`` (models/common.py:330-414) for two streams: ``imgs`` / ``imgs_ir`` are the original images as HWC
    uint8 CUDA tensors (RGB), ``pred`` the per-image ``[n, 6]`` (xyxy, conf, cls) tensors in original-image pixels.  ``render`` draws
    every box with its ``name conf`` label into both streams' images with one ``cft_detect_render`` launch (this project's raster,
    include/cft_hip.h; boxes rounded and painted as detect_twostream.py does, the most confident on top) and returns them; ``save`` and
    ``crop`` write files with PIL; ``show`` needs a display and raises."""

    def __init__(self, imgs, pred, files, times=None, names=None, shape=None, imgs_ir=None):
        from ..utils.general import xyxy2xywh
        d = pred[0].device
        gn = [torch.tensor([*[im.shape[i] for i in [1, 0, 1, 0]], 1., 1.], device=d) for im in imgs]
        self.imgs = imgs
        self.imgs_ir = imgs_ir
        self.pred = pred
        self.names = names
        self.files = files
        self.xyxy = pred
        self.xywh = [xyxy2xywh(x) for x in pred]
        self.xyxyn = [x / g for x, g in zip(self.xyxy, gn)]
        self.xywhn = [x / g for x, g in zip(self.xywh, gn)]
        self.n = len(self.pred)
        self.t = tuple((times[i + 1] - times[i]) * 1000 / self.n for i in range(3)) if times is not None else (0.0, 0.0, 0.0)
        self.s = shape
        self._rendered = False

    def _names(self):
        nc = 1 + max([int(p[:, 5].max()) for p in self.pred if len(p)] or [0])
        return list(self.names) if self.names is not None else [str(i) for i in range(nc)]

    def _boxes(self):
        """``cft_detect_boxes`` on the predictions (already in original-image pixels: gain 1, no padding)."""
        from ..ops import detect_boxes
        from ..utils.metrics import _pack_dets, _to_device
        d = self.pred[0].device
        dets, counts = _pack_dets(list(self.pred), None, d)
        geom = torch.tensor([[im.shape[0], im.shape[1], 1.0, 0.0, 0.0] for im in self.imgs], dtype=torch.float32)
        return detect_boxes(dets.contiguous(), counts, _to_device(geom, d), len(self._names()))

    def _strings(self):
        out = []
        for i, (im, pred) in enumerate(zip(self.imgs, self.pred)):
            s = f'image {i + 1}/{len(self.pred)}: {im.shape[0]}x{im.shape[1]} '
            for c in pred[:, -1].unique().tolist():
                n = int((pred[:, -1] == c).sum())
                s += f"{n} {self._names()[int(c)]}{'s' * (n > 1)}, "
            out.append(s.rstrip(', '))
        return out

    def print(self):
        for s in self._strings():
            print(s)
        print(f'Speed: %.1fms pre-process, %.1fms inference, %.1fms NMS per image at shape {tuple(self.s)}' % self.t)

    def show(self):
        raise NotImplementedError("Detections.show needs a display; use render() or save()")

    def render(self, line_thickness=3, atlas=None):
        from ..utils.plots import BoxRenderer
        if not self._rendered:
            boxes, _, _ = self._boxes()
            r = BoxRenderer(self._names(), boxes.device, line_thickness, hide_labels=False, hide_conf=False, atlas=atlas)
            r(boxes, self.imgs, self.imgs_ir)
            self._rendered = True
        return self.imgs if self.imgs_ir is None else (self.imgs, self.imgs_ir)

    def save(self, save_dir='runs/hub/exp'):
        from PIL import Image
        from ..utils.general import increment_path
        save_dir = increment_path(save_dir, exist_ok=save_dir != 'runs/hub/exp', mkdir=True)
        self.render()
        for i, f in enumerate(self.files):
            Image.fromarray(self.imgs[i].cpu().numpy()).save(save_dir / f)
            if self.imgs_ir is not None:
                stem, _, ext = str(f).rpartition('.')
                Image.fromarray(self.imgs_ir[i].cpu().numpy()).save(save_dir / f'{stem}_ir.{ext}')
            print(f"{'Saved' * (i == 0)} {f}", end=',' if i < self.n - 1 else f' to {save_dir}\n')

    def crop(self, save_dir='runs/hub/exp'):
        """One file per detection under ``save_dir/crops/<class>/``: the reference's rectangle of the UNROUNDED box (``crop_rectangle``),
        cut from the RGB original on the host.  Crop before ``render`` / ``save``: they draw into the images."""
        from ..utils.general import crop_rectangle, increment_path, save_one_box
        if self._rendered:
            raise RuntimeError("Detections.crop: the images have been drawn into; crop before render() / save()")
        save_dir = increment_path(save_dir, exist_ok=save_dir != 'runs/hub/exp', mkdir=True)
        names = self._names()
        for i, im in enumerate(self.imgs):
            host = im.cpu().numpy()
            for *box, conf, cls in self.pred[i].tolist():
                save_one_box(box, host, file=save_dir / 'crops' / names[int(cls)] / self.files[i], rect=crop_rectangle(box, host.shape))
        print(f'Saved results to {save_dir}\n')

    def pandas(self):
        """A copy whose xyxy / xyxyn / xywh / xywhn are lists of pandas DataFrames with the reference's column names."""
        import pandas as pd
        from copy import copy
        new = copy(self)
        ca = 'xmin', 'ymin', 'xmax', 'ymax', 'confidence', 'class', 'name'
        cb = 'xcenter', 'ycenter', 'width', 'height', 'confidence', 'class', 'name'
        names = self._names()
        for k, c in zip(['xyxy', 'xyxyn', 'xywh', 'xywhn'], [ca, ca, cb, cb]):
            a = [[x[:5] + [int(x[5]), names[int(x[5])]] for x in x.tolist()] for x in getattr(self, k)]
            setattr(new, k, [pd.DataFrame(x, columns=c) for x in a])
        return new

    def tolist(self):
        """One Detections per image, its list attributes replaced by that image's element."""
        x = [Detections([self.imgs[i]], [self.pred[i]], [self.files[i]], names=self.names, shape=self.s,
                        imgs_ir=None if self.imgs_ir is None else [self.imgs_ir[i]]) for i in range(self.n)]
        for d in x:
            for k in ['imgs', 'pred', 'xyxy', 'xyxyn', 'xywh', 'xywhn']:
                setattr(d, k, getattr(d, k)[0])
        return x

    def __len__(self):
        return self.n

Classify = _outside("Classify", "models/common.py:417-427")
