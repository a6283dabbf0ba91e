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

``Adam`` / ``AdamW`` (the reference's ``--adam``, ``build_adam_optimizer``) work the same way through ``cft_adam_step``; their per-
parameter step counts stay on the device.  ``step()`` itself is written once, in ``_TableOptimizer``: an optimiser adds only its
hyper-parameter row, its state tensors and its entry point, and ``DeviceTable.call`` is the one place that calls the library
(``ModelEMA`` uses it too).

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

    def call(self, entry, max_blocks, *args):
        """The library call ``entry`` on the table as it is: the six table arguments, ``args``, the current stream of its device."""
        with torch.cuda.device(self.device):
            st = getattr(_lib.load(), entry)(self.dev.data_ptr(), self.host.data_ptr(), self.nseg, self.nwork, self.chunk, max_blocks, *args,
                                             torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(st, entry)


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


def _one_device(device, t, errors):
    """The one device of a table, for a tensor ``t`` that is not on ``device``: the first tensor fixes it (``device`` is None) and
    must be on a GPU, any other is an error.  ``errors``: the texts for a first tensor elsewhere (``{0}``: where) and for a second
    device (``{0}`` and ``{1}``)."""
    if device is not None:
        raise ValueError(errors[1].format(device, t.device))
    if t.device.type != "cuda":
        raise ValueError(errors[0].format(t.device))
    return t.device


def _flag(t, device, what, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != device:
        raise ValueError(f"{what}: {name} must be one float32 on {device}")
    return t.data_ptr()


class _TableOptimizer(torch.optim.Optimizer):
    """What ``SGD`` and ``Adam`` share: the table and the whole of ``step()``.  A subclass names itself (``_name``) and its entry
    point (``_entry``), gives the ctypes type and width of one group's hyper-parameter row (``_hyper_type``, ``_hyper_width``), the
    group keys an older state dict may lack (``_group_defaults``), and supplies ``_check_group(g)``, ``hyper_row(g)``,
    ``_state_ptrs(p, g, total)`` and, where the entry takes more arguments, ``_extra()``."""

    _step_supports_amp_scaling = True

    def __init__(self, params, defaults, chunk, max_blocks):
        self._check_group(defaults)
        super().__init__(params, defaults)
        self._reset(chunk, max_blocks)

    def _reset(self, chunk=CHUNK, max_blocks=0):
        self._table, self._max_blocks = DeviceTable(chunk), int(max_blocks)

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:         # a state dict of an older torch, e.g. a reference checkpoint's
            for k, v in self._group_defaults.items():
                g.setdefault(k, v)
        if "_table" not in self.__dict__:
            self._reset()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"{self._name}: at most {MAX_GROUPS} param groups (their hyper-parameters travel in the kernel arguments)")

    @property
    def table_uploads(self):
        """How often the table went to the device (a step with unchanged tensors uploads nothing)."""
        return self._table.uploads

    def _zeros_state(self, st, p, key, name):
        """Device address of ``st[key]``, ``st = state[p]``: created zero-filled in the layout of ``p`` on first use, checked against
        ``p`` after."""
        t = st.get(key)
        if t is None:
            t = st[key] = torch.zeros_like(p, memory_format=torch.preserve_format)
        else:
            _check_tensor(t, p, self._name, name)
        return t.data_ptr()

    def _extra(self):
        """The entry's arguments between ``ngroups`` and ``grad_scale``."""
        return ()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups, what, width = self.param_groups, self._name, self._hyper_width
        errors = (f"{what}: parameters are on {{}}; this package runs on the GPU only (torch.optim.{what} works on these tensors)",
                  f"{what}: parameters on {{}} and {{}}; one device per optimizer")
        hyper = (self._hyper_type * (width * len(groups)))()
        rows, stepped, device, state_ptrs = [], [], None, self._state_ptrs
        total = sum(len(g["params"]) for g in groups)
        for j, g in enumerate(groups):
            self._check_group(g)
            hyper[width * j:width * (j + 1)] = self.hyper_row(g)
            for p in g["params"]:
                grad = p.grad
                if grad is None:
                    continue
                _check_tensor(p, None, what, "a parameter")
                _check_tensor(grad, p, what, "a gradient")
                if p.device != device:
                    device = _one_device(device, p, errors)
                rows.append((p.data_ptr(), grad.data_ptr(), *state_ptrs(p, g, total), p.numel(), j))
                stepped.append(p)
        if not rows:
            return loss
        what = what + ".step"
        grad_scale = _flag(getattr(self, "grad_scale", None), device, what, "grad_scale")
        found_inf = _flag(getattr(self, "found_inf", None), device, what, "found_inf")
        rows = np.array(rows, dtype=np.int64)
        self._table.sync((rows, rows[:, -2]), device)
        self._last = (hyper, len(groups))
        self._launch(hyper, len(groups), grad_scale, found_inf)
        torch.autograd.graph.increment_version(stepped)      # the kernels wrote through raw pointers: Model's caches key on _version
        return loss

    def _launch(self, hyper, ngroups, grad_scale=None, found_inf=None):
        """The library call alone, on the table as it is (tools/optim_bench.py times it back to back with ``_last``; for Adam every
        call counts one more step)."""
        self._table.call(self._entry, self._max_blocks, hyper, ngroups, *self._extra(), grad_scale, found_inf)


class SGD(_TableOptimizer):
    """``torch.optim.SGD`` (dampening = 0, maximize = False) whose ``step()`` is one HIP launch.

    Same constructor names, same ``param_groups`` and ``state[p]['momentum_buffer']`` layout: ``state_dict()`` loads into
    ``torch.optim.SGD`` and the other way round, ``add_param_group`` and ``lr_scheduler.LambdaLR`` work as with torch's.
    ``torch.amp.GradScaler.step(optimizer)`` hands ``grad_scale`` / ``found_inf`` over and the kernel reads them on the device.

    One difference from torch: momentum buffers are created zero-filled on the first ``step()`` (a zero buffer gives
    ``buf = grad``, torch's ``clone``), so a first step that ``found_inf`` skips leaves zero buffers in ``state`` where torch leaves
    none.  The next step computes the same values either way."""

    _name, _entry = "SGD", "cft_sgd_step"
    _hyper_type, _hyper_width = ctypes.c_float, 4
    _group_defaults = dict(nesterov=False, maximize=False, dampening=0, weight_decay=0)

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
        super().__init__(params, defaults, chunk, max_blocks)

    @staticmethod
    def _check_group(g):
        if g.get("dampening", 0) != 0:
            raise ValueError("SGD: dampening = 0 only (the kernel has no dampening term)")
        if g.get("maximize", False):
            raise ValueError("SGD: maximize = False only")
        if g.get("nesterov", False) and g.get("momentum", 0) <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    @staticmethod
    def hyper_row(g):
        return [float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), 1.0 if g["nesterov"] else 0.0]

    def _state_ptrs(self, p, g, total):
        return (self._zeros_state(self.state[p], p, "momentum_buffer", "a momentum buffer") if float(g["momentum"]) != 0 else 0,)


class Adam(_TableOptimizer):
    """``torch.optim.Adam`` (amsgrad = False, maximize = False) whose ``step()`` is one library call: ``cft_adam_step``, two HIP
    launches over every parameter.

    Same constructor names, same ``param_groups`` keys and the same ``state[p] = {'step', 'exp_avg', 'exp_avg_sq'}`` layout:
    ``state_dict()`` loads into ``torch.optim.Adam`` and the other way round.  ``foreach`` / ``capturable`` / ``differentiable`` /
    ``fused`` are kept in the groups for that and mean nothing here; ``decoupled_weight_decay`` selects AdamW's decay per group.

    The step counts live on the device, one float32 per parameter in a vector this optimiser owns (``GradScaler`` may skip a step
    and only the device knows): ``state[p]['step']`` is a 0-dim view of the parameter's slot.  After ``load_state_dict`` the entry may
    be anything torch accepts (a CPU tensor, a number, a tensor of another optimiser); the next ``step()`` copies its value into the
    slot and puts the view back - a copy after a load only.  A parameter is counted only in steps in which it has a gradient, as
    in torch.  Moments are created zero-filled on a parameter's first step, also when ``found_inf`` skips it."""

    _name, _entry = "Adam", "cft_adam_step"
    _hyper_type, _hyper_width = ctypes.c_double, 6
    _group_defaults = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                           decoupled_weight_decay=False)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=None, chunk=CHUNK, max_blocks=0):
        if decoupled_weight_decay is None:
            decoupled_weight_decay = self._group_defaults["decoupled_weight_decay"]
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults, chunk, max_blocks)

    def _reset(self, *table):
        super()._reset(*table)
        self._steps, self._slot, self._coef = None, {}, None

    def _check_group(self, g):
        if g.get("amsgrad", False):
            raise ValueError(f"{self._name}: amsgrad = False only (the kernel keeps no running maximum)")
        if g.get("maximize", False):
            raise ValueError(f"{self._name}: maximize = False only")
        if not 0.0 <= g["lr"]:
            raise ValueError(f"Invalid learning rate: {g['lr']}")
        if not 0.0 <= g["eps"]:
            raise ValueError(f"Invalid epsilon value: {g['eps']}")
        if not 0.0 <= g["weight_decay"]:
            raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")
        betas = g["betas"]
        if len(betas) != 2:
            raise ValueError(f"Invalid betas: {betas}")
        for k in (0, 1):
            if not 0.0 <= betas[k] < 1.0:
                raise ValueError(f"Invalid beta parameter at index {k}: {betas[k]}")

    @staticmethod
    def hyper_row(g):
        beta1, beta2 = g["betas"]
        return [float(g["lr"]), float(beta1), float(beta2), float(g["eps"]), float(g["weight_decay"]), 1.0 if g["decoupled_weight_decay"] else 0.0]

    def _step_slot(self, p, device, total):
        """Device address of the step counter of ``p`` (one of ``total`` parameters in the groups); ``state[p]['step']`` is (again)
        the 0-dim view of it."""
        if self._steps is None or self._steps.device != device or self._steps.numel() < total:
            # the first step, or parameters were added: a new vector; the old views are adopted below like any foreign value
            self._steps = torch.zeros(total, dtype=torch.float32, device=device)
        i = self._slot.get(p)
        if i is None:
            i = self._slot[p] = len(self._slot)
            if i >= self._steps.numel():
                raise ValueError(f"{self._name}: more parameters than the groups hold")
        ptr = self._steps.data_ptr() + 4 * i
        st = self.state[p]
        have = st.get("step")
        if isinstance(have, torch.Tensor) and have.dtype == torch.float32 and have.dim() == 0 and have.data_ptr() == ptr:
            return ptr
        slot = self._steps[i]
        if have is None:
            slot.zero_()
        elif isinstance(have, torch.Tensor):
            if have.numel() != 1:
                raise ValueError(f"{self._name}: state['step'] must hold one value, got shape {tuple(have.shape)}")
            slot.copy_(have.detach().reshape(()))
        else:
            slot.fill_(float(have))
        st["step"] = slot
        return ptr

    def _state_ptrs(self, p, g, total):
        st = self.state[p]
        return (self._zeros_state(st, p, "exp_avg", "exp_avg"), self._zeros_state(st, p, "exp_avg_sq", "exp_avg_sq"), self._step_slot(p, p.device, total))

    def _extra(self):
        t = self._table
        if self._coef is None or self._coef.device != t.device or self._coef.shape[0] < t.nseg:
            self._coef = torch.empty((t.nseg, 2), dtype=torch.float32, device=t.device)      # per tensor: step_size, sqrt(bias correction 2)
        return (self._coef.data_ptr(),)


class AdamW(Adam):
    """``torch.optim.AdamW``: ``Adam`` with ``weight_decay = 1e-2`` and the decay decoupled from the gradient
    (``p *= 1 - lr * weight_decay`` before the update) by default."""

    _name = "AdamW"
    _group_defaults = dict(Adam._group_defaults, decoupled_weight_decay=True)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)


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


def build_adam_optimizer(model, hyp, decoupled=False):
    """The optimiser of ``train.py:557-563`` with ``opt.adam``: ``Adam(pg0, lr=hyp['lr0'], betas=(hyp['momentum'], 0.999))`` over the
    BatchNorm weights, then the decayed weights with ``hyp['weight_decay']`` and the biases as two more groups.  ``decoupled=True``
    gives ``AdamW`` with the same groups (group 0 without decay, as in the reference's list).

    ``build_optimizer(..., adam=True)`` still refuses and names ``torch.optim.Adam``: that text is pinned by a test and is left
    as it is; this function is the HIP form of what it describes.  The groups have no ``'momentum'`` key, so ``warmup()`` moves
    only their lr and beta1 is not warmed up - the reference's behaviour."""
    pg0, pg1, pg2 = param_groups(model)
    cls = AdamW if decoupled else Adam
    optimizer = cls(pg0, lr=hyp["lr0"], betas=(hyp["momentum"], 0.999), weight_decay=0)
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
