"""The optimiser half of a training step on the GPU: the reference's three parameter groups, warm-up and ``optim.SGD``
(``train.py:545-563, 735-744, 769``), the update as ONE HIP launch over every parameter (``csrc/optim.hip``).

    optimizer = build_optimizer(model, hyp)                       # train.py:557-563
    scheduler = lr_scheduler.LambdaLR(optimizer, lr_lambda=one_cycle(1, hyp['lrf'], epochs))
    ...
    accumulate = warmup(optimizer, ni, nw, epoch, lf, hyp, nbs, total_batch_size)     # train.py:735-744
    scaler.step(optimizer); scaler.update(); optimizer.zero_grad()                    # train.py:769-771

``SGD.step()`` consumes ``.grad`` tensors, whoever filled them, and never synchronises with the host.  The tensors are described
to the kernel by a table in device memory (one row per parameter, then the chunks the rows are cut into); the table is rebuilt and
uploaded only when a pointer, a size or the set of parameters that have a gradient changes, the per-group lr / momentum /
weight_decay / nesterov travel in the kernel arguments, so the warm-up's per-iteration edits of ``param_groups`` cost nothing.

The kernel writes the parameters through raw pointers; ``step()`` then bumps their version counters, which is what ``Model`` reads to
decide that its packed weights and captured graphs are stale.
"""
import ctypes

import numpy as np
import torch
from torch._prims_common import is_non_overlapping_and_dense

from .. import _lib

CHUNK = _lib._consts["CFT_OPTIM_CHUNK"]             # elements per work row
MAX_GROUPS = _lib._consts["CFT_OPTIM_MAX_GROUPS"]


def param_groups(model):
    """``(pg0, pg1, pg2)`` = (BatchNorm2d weights: no decay, other weights: decay, biases), the reference's rule over
    ``model.named_modules()``: a module whose ``.bias`` is an ``nn.Parameter`` gives it to pg2; an ``nn.BatchNorm2d`` gives its
    ``.weight`` to pg0; any other module whose ``.weight`` is an ``nn.Parameter`` gives it to pg1.

    A parameter that is neither a ``weight`` nor a ``bias`` of its module is in no group and is therefore never trained: in the CFT
    networks that is ``GPT.pos_emb``, which the reference leaves at its initial value as well.  This is kept, not repaired."""
    pg0, pg1, pg2 = [], [], []
    for _, m in model.named_modules():
        bias, weight = getattr(m, "bias", None), getattr(m, "weight", None)
        if isinstance(bias, torch.nn.Parameter):
            pg2.append(bias)
        if isinstance(m, torch.nn.BatchNorm2d):
            pg0.append(m.weight)
        elif isinstance(weight, torch.nn.Parameter):
            pg1.append(weight)
    return pg0, pg1, pg2


def work_rows(counts, chunk=CHUNK):
    """The canonical cut of segments of ``counts`` elements into chunks: int64 [nwork, 2] = (segment, first element) - the
    ``cft_optim_work_t`` rows (``{int seg; int pad = 0; long start}``, little endian)."""
    counts = np.asarray(counts, dtype=np.int64)
    per = (counts + (chunk - 1)) // chunk
    seg = np.repeat(np.arange(len(counts), dtype=np.int64), per)
    first = np.repeat(np.cumsum(per) - per, per)
    return np.stack([seg, (np.arange(int(per.sum()), dtype=np.int64) - first) * chunk], axis=1)


class DeviceTable:
    """Segment rows + work rows in one device buffer, with the host copy that decides whether it is still current."""

    def __init__(self, chunk=CHUNK):
        self.chunk, self.rows, self.device, self.uploads = int(chunk), None, None, 0
        self.host = self.dev = None
        self.nseg = self.nwork = 0

    def sync(self, table, device):
        """``table`` = (rows, counts): the segment rows, int64 [nseg, width], and their column of element counts.  Uploads (from
        pinned memory, not blocking) only when the rows differ from the last call's; returns whether it did."""
        rows, counts = table
        if self.rows is not None and self.device == device and rows.shape == self.rows.shape and np.array_equal(rows, self.rows):
            return False
        work = work_rows(counts, self.chunk)
        host = torch.empty((rows.size + work.size,), dtype=torch.int64).pin_memory()
        flat = host.numpy()
        flat[:rows.size] = rows.reshape(-1)
        flat[rows.size:] = work.reshape(-1)
        self.host, self.dev = host, host.to(device, non_blocking=True)
        self.rows, self.device, self.nseg, self.nwork = rows, device, rows.shape[0], work.shape[0]
        self.uploads += 1
        return True


def _check_tensor(t, like, what, name):
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if t.is_sparse or t.layout != torch.strided:
        raise ValueError(f"{what}: {name} must be a dense strided tensor")
    if like is None:
        if not (t.is_contiguous() or is_non_overlapping_and_dense(t)):
            raise ValueError(f"{what}: {name} must be contiguous or dense (no gaps, no overlap); strides {tuple(t.stride())}")
        return
    if t.shape != like.shape:
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(like.shape)}")
    if t.device != like.device:
        raise ValueError(f"{what}: {name} is on {t.device}, expected {like.device}")
    if not ((t.is_contiguous() and like.is_contiguous()) or t.stride() == like.stride()):
        raise ValueError(f"{what}: {name} must have the memory layout of its partner (strides {tuple(t.stride())} / {tuple(like.stride())})")


def _flag(t, device, what, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != device:
        raise ValueError(f"{what}: {name} must be one float32 on {device}")
    return t.data_ptr()


class SGD(torch.optim.Optimizer):
    """``torch.optim.SGD`` (dampening = 0, maximize = False) whose ``step()`` is one HIP launch.

    Same constructor names, same ``param_groups`` and ``state[p]['momentum_buffer']`` layout: ``state_dict()`` loads into
    ``torch.optim.SGD`` and the other way round, ``add_param_group`` and ``lr_scheduler.LambdaLR`` work as with torch's.
    ``torch.amp.GradScaler.step(optimizer)`` hands ``grad_scale`` / ``found_inf`` over and the kernel reads them on the device.

    One difference from torch: momentum buffers are created zero-filled on the first ``step()`` (a zero buffer gives
    ``buf = grad``, torch's ``clone``), so a first step that ``found_inf`` skips leaves zero buffers in ``state`` where torch leaves
    none.  The next step computes the same values either way."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, chunk=CHUNK,
                 max_blocks=0):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        foreach=None, differentiable=False, fused=None)
        self._check_group(defaults)
        super().__init__(params, defaults)
        self._table, self._max_blocks = DeviceTable(chunk), int(max_blocks)

    @staticmethod
    def _check_group(g):
        if g.get("dampening", 0) != 0:
            raise ValueError("SGD: dampening = 0 only (the kernel has no dampening term)")
        if g.get("maximize", False):
            raise ValueError("SGD: maximize = False only")
        if g.get("nesterov", False) and g.get("momentum", 0) <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:         # a state dict of an older torch, e.g. a reference checkpoint's
            g.setdefault("nesterov", False)
            g.setdefault("maximize", False)
            g.setdefault("dampening", 0)
            g.setdefault("weight_decay", 0)
        if "_table" not in self.__dict__:
            self._table, self._max_blocks = DeviceTable(), 0

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"SGD: at most {MAX_GROUPS} param groups (their hyper-parameters travel in the kernel arguments)")

    @property
    def table_uploads(self):
        """How often the table went to the device (a step with unchanged tensors uploads nothing)."""
        return self._table.uploads

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        hyper = (ctypes.c_float * (4 * len(groups)))()
        rows, stepped, device = [], [], None
        for j, g in enumerate(groups):
            self._check_group(g)
            momentum = float(g["momentum"])
            hyper[4 * j:4 * j + 4] = [float(g["lr"]), momentum, float(g["weight_decay"]), 1.0 if g["nesterov"] else 0.0]
            for p in g["params"]:
                grad = p.grad
                if grad is None:
                    continue
                _check_tensor(p, None, "SGD", "a parameter")
                _check_tensor(grad, p, "SGD", "a gradient")
                if device is None:
                    device = p.device
                    if device.type != "cuda":
                        raise ValueError(f"SGD: parameters are on {device}; this package runs on the GPU only (torch.optim.SGD works on these tensors)")
                elif p.device != device:
                    raise ValueError(f"SGD: parameters on {device} and {p.device}; one device per optimizer")
                bptr = 0
                if momentum != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    else:
                        _check_tensor(buf, p, "SGD", "a momentum buffer")
                    bptr = buf.data_ptr()
                rows.append((p.data_ptr(), grad.data_ptr(), bptr, p.numel(), j))
                stepped.append(p)
        if not rows:
            return loss
        what = "SGD.step"
        grad_scale = _flag(getattr(self, "grad_scale", None), device, what, "grad_scale")
        found_inf = _flag(getattr(self, "found_inf", None), device, what, "found_inf")
        rows = np.array(rows, dtype=np.int64)
        self._table.sync((rows, rows[:, 3]), device)
        self._last = (hyper, len(groups))
        self._launch(hyper, len(groups), grad_scale, found_inf)
        torch.autograd.graph.increment_version(stepped)      # the kernel wrote through raw pointers: Model's caches key on _version
        return loss

    def _launch(self, hyper, ngroups, grad_scale=None, found_inf=None):
        """The launch alone, on the table as it is (tools/optim_bench.py times it back to back with ``_last``)."""
        t = self._table
        with torch.cuda.device(t.device):
            st = _lib.load().cft_sgd_step(t.dev.data_ptr(), t.host.data_ptr(), t.nseg, t.nwork, t.chunk, self._max_blocks, hyper, ngroups,
                                          grad_scale, found_inf, torch.cuda.current_stream(t.device).cuda_stream)
        _lib.check(st, "cft_sgd_step")


def build_optimizer(model, hyp, adam=False):
    """The optimiser of ``train.py:557-563``: SGD with Nesterov momentum over the BatchNorm weights, then the decayed weights with
    ``hyp['weight_decay']`` and the biases as two more groups."""
    if adam:
        raise NotImplementedError("build_optimizer: the Adam form has no HIP kernel here; torch.optim.Adam(pg0, lr=hyp['lr0'], "
                                  "betas=(hyp['momentum'], 0.999)) works on these tensors")
    pg0, pg1, pg2 = param_groups(model)
    optimizer = SGD(pg0, lr=hyp["lr0"], momentum=hyp["momentum"], nesterov=True)
    optimizer.add_param_group({"params": pg1, "weight_decay": hyp["weight_decay"]})
    optimizer.add_param_group({"params": pg2})
    return optimizer


def warmup(optimizer, ni, nw, epoch, lf, hyp, nbs, total_batch_size):
    """The warm-up of ``train.py:735-744`` at integrated batch ``ni`` of ``nw`` warm-up batches: every group's lr rises linearly from
    0 (biases, group 2: falls from ``hyp['warmup_bias_lr']``) to ``initial_lr * lf(epoch)``, momentum from ``hyp['warmup_momentum']`` to
    ``hyp['momentum']``.  Returns ``accumulate``, the batches to accumulate before a step (1 at ``ni = 0`` up to ``nbs / total_batch_size``).
    Past ``nw`` nothing is touched and the final ``accumulate`` is returned."""
    full = nbs / total_batch_size
    if ni > nw:
        return max(round(full), 1)
    span = [0, nw]
    for j, g in enumerate(optimizer.param_groups):
        start = hyp["warmup_bias_lr"] if j == 2 else 0.0
        g["lr"] = np.interp(ni, span, [start, g["initial_lr"] * lf(epoch)])
        if "momentum" in g:
            g["momentum"] = np.interp(ni, span, [hyp["warmup_momentum"], hyp["momentum"]])
    return max(1, np.interp(ni, span, [1, full]).round())
