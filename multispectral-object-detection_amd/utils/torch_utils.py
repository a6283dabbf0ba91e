"""``intersect_dicts`` / ``load_pretrained`` (the weight transfer of the reference's train.py:514-525), ``ModelEMA`` of the reference (``utils/torch_utils.py:269-303``) with the update as ONE HIP launch (``csrc/optim.hip``), and the
copy of a model that such an average - and a checkpoint - needs: parameters, buffers and attributes, not kernel-side caches."""
import ctypes
import logging
import math
from copy import deepcopy

import numpy as np
import torch

from ..models.common import invalidate_packed
from .optim import CHUNK, DeviceTable, _check_tensor, _one_device

logger = logging.getLogger(__name__)

_DEVICE_ERRORS = ("ModelEMA: the model is on {}; this package runs on the GPU only", "ModelEMA: tensors on {} and {}")

# what Model and its modules keep in __dict__ besides their state: packed weights, launch plans, captured graphs, the tensor list of
# weights_key, the layer graph, the side stream.  None of it can or should be copied; all of it is rebuilt on demand.
_CACHES = ("_cft_cache", "_cft_cache_train", "_plan_cache", "_graphs", "_wlist", "_layer_graph", "_side_stream")


def is_parallel(model):
    return type(model) in (torch.nn.parallel.DataParallel, torch.nn.parallel.DistributedDataParallel)


def de_parallel(model):
    return model.module if is_parallel(model) else model


def copy_attr(a, b, include=(), exclude=()):
    """Copy the attributes of ``b`` to ``a``: only those in ``include`` if given, never private ones or those in ``exclude``."""
    for k, v in b.__dict__.items():
        if (len(include) and k not in include) or k.startswith("_") or k in exclude:
            continue
        setattr(a, k, v)


def detached_copy(model):
    """``deepcopy(model)`` without the caches: works on a model that holds packed weights, plans and captured HIP graphs (a graph
    cannot be copied), leaves ``model`` as it was, and returns a copy that packs and captures for itself."""
    held = []
    for m in model.modules():
        h = {k: m.__dict__.pop(k) for k in _CACHES if k in m.__dict__}
        if h:
            held.append((m, h))
    try:
        copy = deepcopy(model)
    finally:
        for m, h in held:
            m.__dict__.update(h)
    for src, dst in zip(model.modules(), copy.modules()):
        if "_graphs" in src.__dict__:
            dst.__dict__["_graphs"] = {}
    invalidate_packed(copy)
    return copy


def intersect_dicts(da, db, exclude=()):
    """The entries of ``da`` whose key is in ``db`` with the same shape and holds none of the ``exclude`` substrings (the values are
    ``da``'s): the reference's helper of the same name (utils/torch_utils.py:139-141)."""
    return {k: v for k, v in da.items() if k in db and v.shape == db[k].shape and not any(x in k for x in exclude)}


def load_pretrained(model, ckpt_or_path, exclude=('anchor',)):
    """Start ``model`` - two-stream or single-stream - from pretrained weights, the statements of the reference's train.py:514-525:
    the checkpoint's model in fp32, its state dict intersected with the target's by key and shape (``exclude``: train.py leaves the
    anchors out when the target comes from a cfg), loaded non-strictly.  ``ckpt_or_path``: a checkpoint file (a single-stream
    ``yolov5*.pt`` un-pickles through ``compat.install_reference_aliases``), the loaded dict, a model, or a state dict.  Returns the
    list of transferred keys; packed weights and captured graphs of ``model`` are dropped (``invalidate_packed``)."""
    ckpt = ckpt_or_path
    if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, "__fspath__"):
        from ..compat import install_reference_aliases
        install_reference_aliases()
        ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    if isinstance(ckpt, dict) and isinstance(ckpt.get("model"), torch.nn.Module):
        ckpt = ckpt["model"]
    if isinstance(ckpt, torch.nn.Module):
        ckpt = {k: (v.float() if v.is_floating_point() else v) for k, v in ckpt.state_dict().items()}      # train.py:521 .float()
    target = de_parallel(model)
    state = intersect_dicts(ckpt, target.state_dict(), exclude=tuple(exclude))
    target.load_state_dict(state, strict=False)
    invalidate_packed(target)
    logger.info('Transferred %g/%g items' % (len(state), len(target.state_dict())))
    return list(state)


class ModelEMA:
    """Exponential moving average of everything in the model's state dict (parameters and buffers), the model the reference
    validates and ships.  ``ema`` is an fp32 eval copy that needs no grad; ``update(model)`` is one kernel launch over every
    floating-point entry (integer buffers such as ``num_batches_tracked`` are left alone, as in the reference) and does not
    synchronise with the host.  The table of tensor pairs is cached like ``SGD``'s."""

    def __init__(self, model, decay=0.9999, updates=0):
        self.ema = detached_copy(de_parallel(model)).eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / 2000))     # ramps up, so that early updates follow the model
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self._table, self._max_blocks = DeviceTable(CHUNK), 0

    @torch.no_grad()
    def update(self, model):
        self.updates += 1
        d = self.decay(self.updates)
        msd = de_parallel(model).state_dict(keep_vars=True)
        rows, written, device = [], [], None
        for k, v in self.ema.state_dict(keep_vars=True).items():
            if not v.dtype.is_floating_point:
                continue
            m = msd[k]
            _check_tensor(v, None, "ModelEMA", f"ema {k}")
            _check_tensor(m, v, "ModelEMA", f"model {k}")
            if v.device != device:
                device = _one_device(device, v, _DEVICE_ERRORS)
            rows.append((v.data_ptr(), m.data_ptr(), v.numel()))
            written.append(v)
        if not rows:
            return
        rows = np.array(rows, dtype=np.int64)
        self._table.sync((rows, rows[:, 2]), device)
        self._launch(d)
        torch.autograd.graph.increment_version(written)      # raw-pointer writes: the copy's packed weights and graphs are stale

    def _launch(self, d):
        """The launch alone, on the table as it is.  d and 1 - d are each computed in double, then rounded to float: what
        ``v *= d; v += (1. - d) * msd[k]`` does with Python scalars."""
        self._table.call("cft_ema_update", self._max_blocks, ctypes.c_float(d), ctypes.c_float(1. - d))

    def update_attr(self, model, include=(), exclude=('process_group', 'reducer')):
        copy_attr(self.ema, model, include, exclude)
