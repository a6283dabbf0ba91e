"""The reference's ``ComputeLoss`` (``utils/loss.py:88-216``) on the GPU, with its gradient (``csrc/loss.hip``).

    compute_loss = ComputeLoss(model)                 # model.hyp, model.gr and the Detect module, as in the reference
    loss, loss_items = compute_loss(pred, targets)    # pred: Detect's raw list; targets [nt, 6] normalised
    loss.backward()                                   # when any pred[i] requires grad: dL/dpred[i] by a HIP kernel

``__call__`` never synchronises with the host: build_targets, the matched entries, the dense objectness BCE, the
scalars and (with ``autobalance``) the balance update all run on the device.  Only reading ``balance`` as a list and
``check()`` synchronise.

Targets the reference would raise on are skipped instead and recorded in a device-side flag: an image index outside
``[0, B)``, and with ``nc > 1`` a class outside ``[0, nc)``, on a target that passes the anchor test.  ``check()``
synchronises once, raises if any such target was seen since the last ``check()``, and clears the flag.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _require_cuda, _stream

ERR_IMAGE, ERR_CLASS = 1, 2


def smooth_BCE(eps=0.1):
    """Positive and negative label-smoothing BCE targets (https://arxiv.org/pdf/1902.04103.pdf eqn 3)."""
    return 1.0 - 0.5 * eps, 0.5 * eps


def _is_parallel(model):
    return type(model) in (torch.nn.parallel.DataParallel, torch.nn.parallel.DistributedDataParallel)


def _to_device(t, device):
    if t.device == device:
        return t
    if t.device.type != "cpu":
        return t.to(device)
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


class _Call:
    """One forward's geometry and workspace; the backward reads the workspace the forward filled."""

    def __init__(self, cl, p, targets):
        self.cl = cl
        self.B, self.na = p[0].shape[0], p[0].shape[1]
        self.ny, self.nx = _ints([t.shape[2] for t in p]), _ints([t.shape[3] for t in p])
        self.nt = targets.shape[0]
        lib = _lib.load()
        nbytes = lib.cft_loss_workspace_bytes(cl.nl, self.B, self.na, self.ny, self.nx, cl.nc, self.nt)
        if nbytes < 0:
            raise ValueError(f"ComputeLoss: unsupported sizes (B {self.B}, na {self.na}, nc {cl.nc}, nt {self.nt})")
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=targets.device)

    def forward(self, p, targets):
        cl, lib = self.cl, _lib.load()
        loss = torch.empty((1,), dtype=torch.float32, device=targets.device)
        items = torch.empty((4,), dtype=torch.float32, device=targets.device)
        st = lib.cft_loss_forward(cl.nl, _ptrs(p), self.B, self.na, self.ny, self.nx, cl.nc,
                                  targets.data_ptr() if self.nt else None, self.nt, cl._anchors.data_ptr(), cl._hyp_arr,
                                  cl._balance.data_ptr(), int(cl.autobalance), cl.ssi, self.ws.data_ptr(), self.ws.numel(),
                                  loss.data_ptr(), items.data_ptr(), cl._err.data_ptr(), _stream())
        _lib.check(st, "cft_loss_forward")
        return loss, items

    def backward(self, p, grad_loss):
        cl, lib = self.cl, _lib.load()
        grads = [torch.empty_like(t) for t in p]
        st = lib.cft_loss_backward(cl.nl, _ptrs(p), self.B, self.na, self.ny, self.nx, cl.nc, self.nt, cl._anchors.data_ptr(),
                                   cl._hyp_arr, grad_loss.data_ptr(), _ptrs(grads), self.ws.data_ptr(), self.ws.numel(), _stream())
        _lib.check(st, "cft_loss_backward")
        return grads


class _LossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call, targets, *p):
        loss, items = call.forward(p, targets)
        ctx.call = call
        ctx.save_for_backward(*p)
        ctx.mark_non_differentiable(items)
        return loss, items

    @staticmethod
    def backward(ctx, grad_loss, grad_items):
        p = ctx.saved_tensors
        if grad_loss is None:
            grad_loss = torch.zeros((1,), dtype=torch.float32, device=p[0].device)
        grads = ctx.call.backward(p, grad_loss.float().contiguous())
        return (None, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:])])


def skipped_targets_message(err, nc):
    """The message of ComputeLoss.check() for the device error bits ``err`` (ERR_IMAGE | ERR_CLASS), or None when err is 0."""
    what = []
    if err & ERR_IMAGE:
        what.append("an image index outside [0, batch size)")
    if err & ERR_CLASS:
        what.append(f"a class outside [0, {nc})")
    if err & ~(ERR_IMAGE | ERR_CLASS):
        what.append(f"unknown error bits {err & ~(ERR_IMAGE | ERR_CLASS):#x}")
    return "ComputeLoss: targets with " + " and ".join(what) + " were skipped" if what else None


def validate_inputs(p, targets, nl, na, nc):
    """The host-side checks of ComputeLoss.__call__ (shapes, dtype, contiguity; no device access)."""
    if not isinstance(p, (list, tuple)) or len(p) != nl:
        raise ValueError(f"ComputeLoss: expected a list of {nl} head tensors, got {type(p).__name__} of length {len(p) if hasattr(p, '__len__') else '?'}")
    B = None
    for i, t in enumerate(p):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"ComputeLoss: p[{i}] is not a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"ComputeLoss: p[{i}] must be float32, got {t.dtype} (the reference casts with .float())")
        if not t.is_contiguous():
            raise ValueError(f"ComputeLoss: p[{i}] must be contiguous")
        if t.dim() != 5:
            raise ValueError(f"ComputeLoss: p[{i}] must be [B, na, ny, nx, no], got {tuple(t.shape)}")
        if t.shape[4] != nc + 5:
            raise ValueError(f"ComputeLoss: p[{i}] has no = {t.shape[4]}, expected nc + 5 = {nc + 5}")
        if t.shape[1] != na:
            raise ValueError(f"ComputeLoss: p[{i}] has {t.shape[1]} anchors, expected {na}")
        if B is None:
            B = t.shape[0]
        elif t.shape[0] != B:
            raise ValueError(f"ComputeLoss: p[{i}] has batch {t.shape[0]}, p[0] has {B}")
        if t.numel() == 0:
            raise ValueError(f"ComputeLoss: p[{i}] is empty")
    if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.shape[1] != 6:
        raise ValueError(f"ComputeLoss: targets must be an [nt, 6] tensor (image, class, x, y, w, h), got {getattr(targets, 'shape', type(targets))}")


class ComputeLoss:
    """The reference's ComputeLoss: same constructor, attributes and return value; the work is done by HIP kernels."""

    def __init__(self, model, autobalance=False):
        device = next(model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("ComputeLoss: the model must be on the GPU (this package has no CPU path)")
        h = model.hyp
        self.cp, self.cn = smooth_BCE(eps=h.get('label_smoothing', 0.0))
        det = model.module.model[-1] if _is_parallel(model) else model.model[-1]
        balance = {3: [4.0, 1.0, 0.4]}.get(det.nl, [4.0, 1.0, 0.25, 0.06, .02])
        self.ssi = list(det.stride).index(16) if autobalance else 0
        self.gr, self.hyp, self.autobalance = model.gr, h, autobalance
        for k in 'na', 'nc', 'nl', 'anchors':
            setattr(self, k, getattr(det, k))
        if not 1 <= self.nl <= 5:
            raise ValueError(f"ComputeLoss: {self.nl} detection levels (1 to 5 supported)")
        if len(balance) < self.nl:
            raise ValueError(f"ComputeLoss: no balance for {self.nl} levels")
        self.device = device
        self._balance = _to_device(torch.tensor(balance[:self.nl], dtype=torch.float64), device)
        self._anchors = self.anchors.detach().to(device=device, dtype=torch.float32).reshape(self.nl, self.na, 2).contiguous()
        self._err = torch.zeros((1,), dtype=torch.int32, device=device)

    @property
    def balance(self):
        """The per-level objectness weights as a list (reads the device: synchronises)."""
        return self._balance.tolist()

    @balance.setter
    def balance(self, values):
        values = [float(v) for v in values]
        if len(values) != self.nl:
            raise ValueError(f"ComputeLoss: balance needs {self.nl} values, got {len(values)}")
        self._balance.copy_(_to_device(torch.tensor(values, dtype=torch.float64), self.device))

    @property
    def _hyp_arr(self):
        h = self.hyp
        vals = (h['box'], h['obj'], h['cls'], h['cls_pw'], h['obj_pw'], h['anchor_t'], h['fl_gamma'], self.cp, self.cn, self.gr)
        return (ctypes.c_double * len(vals))(*[float(v) for v in vals])

    def _validate(self, p, targets):
        validate_inputs(p, targets, self.nl, self.na, self.nc)
        for i, t in enumerate(p):
            _require_cuda(t, "ComputeLoss")
            if t.device != self.device:
                raise ValueError(f"ComputeLoss: p[{i}] is on {t.device}, the model on {self.device}")
        return _to_device(targets.float(), self.device).contiguous()

    def __call__(self, p, targets):
        """Returns ``(loss * bs [1], (lbox, lobj, lcls, loss) [4])`` on the device, without a host synchronisation."""
        targets = self._validate(p, targets)
        call = _Call(self, p, targets)
        if torch.is_grad_enabled() and any(t.requires_grad for t in p):
            return _LossFunction.apply(call, targets, *p)
        return call.forward(p, targets)

    def loss_and_grads(self, p, targets, grad_loss=None):
        """Forward and backward in one call, without an autograd graph: ``(loss, items, [dL/dp_i])`` with L = loss * grad_loss
        (grad_loss: a device float32 [1], default 1).  The same kernels as ``__call__`` + ``loss.backward()``; this form is the
        one to capture in a ``torch.cuda.graph`` together with the rest of a step."""
        targets = self._validate(p, targets)
        call = _Call(self, p, targets)
        p = [t.detach() for t in p]
        loss, items = call.forward(p, targets)
        if grad_loss is None:
            grad_loss = torch.ones((1,), dtype=torch.float32, device=self.device)
        return loss, items, call.backward(p, grad_loss.float().contiguous())

    def build_targets(self, p, targets):
        """The reference's build_targets output ``(tcls, tbox, indices, anch)`` as the GPU computes it (for inspection: runs the
        forward without updating balance, then reads the candidate counts, which synchronises)."""
        targets = self._validate(p, targets)
        call = _Call(self, p, targets)
        ab, self.autobalance = self.autobalance, False
        try:
            call.forward(p, targets)
        finally:
            self.autobalance = ab
        off = (ctypes.c_long * 4)()
        cap = _lib.load().cft_loss_workspace_offsets(self.nl, call.B, call.na, call.ny, call.nx, self.nc, call.nt, off)
        ws = call.ws
        view = lambda o, n, dt: ws[o:o + n * 4].view(dt)  # noqa: E731
        counts = view(off[3], self.nl, torch.int32).tolist()
        tcls, tbox, indices, anch = [], [], [], []
        for i in range(self.nl):
            n = counts[i]
            cell = view(off[0] + i * cap * 4, cap, torch.int32)[:n].long()
            ny, nx = call.ny[i], call.nx[i]
            gi, r = cell % nx, cell // nx
            gj, r = r % ny, r // ny
            a, b = r % call.na, r // call.na
            indices.append((b, a, gj, gi))
            tcls.append(view(off[1] + i * cap * 4, cap, torch.int32)[:n].long())
            tbox.append(view(off[2] + i * cap * 16, cap * 4, torch.float32)[:n * 4].reshape(n, 4))
            anch.append(self._anchors[i][a])
        return tcls, tbox, indices, anch

    def check(self):
        """Synchronise once; raise if a target was skipped since the last check (bad image index or class), then clear."""
        err = int(self._err.item())
        if err:
            self._err.zero_()
            raise ValueError(skipped_targets_message(err, self.nc))
