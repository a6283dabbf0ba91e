"""Float64 oracle of the optimiser step and the EMA update (``csrc/optim.hip``), the small seeded module their fixtures are recorded
on, and the per-element error bound the tests hold the kernels to.

One SGD step and one EMA update are restated in float64 from float32 state, with the hyper-parameters rounded to float32 first, as
the kernel (and torch, which casts a Python scalar to the tensor's dtype) receives them.

Bound: ``|got - ref64| <= 8 * 2^-24 * T`` per element, T = the sum of the absolute values of the terms that enter the element.
Derivation: the value is a sum of products of at most a handful of float32 numbers; evaluated in float32, fused or not, it takes at
most 8 roundings (unscale, decay, momentum, Nesterov and update, each a multiply and an add when not fused; fewer here), and each
rounding errs by at most half an ulp of its result, which is at most 2^-24 times a partial sum of the |terms|, so at most 2^-24 * T.
torch's own unfused CPU step stays within 0.41 of this bound and the reference's two-statement EMA within 0.28 (measured on
200 001-element vectors spanning seven decades); a wrong sign, a dropped decay, dampening taken for momentum or the other Nesterov
form exceed it by orders of magnitude.
"""
import numpy as np
import torch
import torch.nn as nn

EPS = 8.0 * 2.0 ** -24


def f32(x):
    return float(np.float32(x))


def _f64(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def sgd_step(p, g, b, lr, momentum, weight_decay, nesterov, grad_scale=None):
    """One step from float32 ``p``, ``g``, ``b`` (``None``: the zero buffer of a first step).  Returns float64
    ``(p1, b1, bound_p, bound_b)``; with ``momentum == 0`` ``b1`` is the (unstored) update direction."""
    lr, m, wd = f32(lr), f32(momentum), f32(weight_decay)
    p, g = _f64(p), _f64(g)
    b = np.zeros_like(p) if b is None else _f64(b)
    g0 = g * f32(1.0 / float(grad_scale)) if grad_scale is not None else g
    g1 = g0 + wd * p
    t_g1 = np.abs(g0) + wd * np.abs(p)
    b1 = m * b + g1
    t_b1 = m * np.abs(b) + t_g1
    if nesterov:
        d, t_d = g1 + m * b1, t_g1 + m * t_b1
    else:
        d, t_d = b1, t_b1
    p1 = p - lr * d
    return p1, b1, EPS * (np.abs(p) + lr * t_d), EPS * t_b1


def ema_update(e, m, d):
    """One EMA update from float32 ``e`` (average) and ``m`` (model) with decay ``d`` (a Python float).  Float64 ``(e1, bound)``."""
    d32, omd32 = f32(d), f32(1.0 - d)
    e, m = _f64(e), _f64(m)
    return d32 * e + omd32 * m, EPS * (d32 * np.abs(e) + omd32 * np.abs(m))


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0): at most 1 when the bound holds."""
    err = np.abs(_f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max()) if q.size else 0.0


class SmallNet(nn.Module):
    """conv + BatchNorm2d + linear, 4 673 elements in its state dict: every kind of entry the rule and the EMA tell apart (weights
    with and without decay, biases, running statistics, the integer ``num_batches_tracked``)."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 16, 3)
        self.bn = nn.BatchNorm2d(16)
        self.fc = nn.Linear(64, 64)

    def forward(self, x):
        return self.fc(self.bn(self.conv(x)).mean(1).reshape(x.shape[0], -1)[:, :64])


def seeded_state(net, k):
    """State ``k`` of a SmallNet: values spread over four decades, positive variances, ``num_batches_tracked = k``."""
    rng = np.random.default_rng(1000 + k)
    out = {}
    for name, v in net.state_dict().items():
        if not v.dtype.is_floating_point:
            out[name] = torch.full_like(v, k)
            continue
        a = rng.standard_normal(tuple(v.shape)) * 10.0 ** rng.uniform(-3, 1, tuple(v.shape))
        if name.endswith("running_var"):
            a = np.abs(a) + 0.1
        out[name] = torch.from_numpy(a.astype(np.float32))
    return out


def seeded_grads(net, k):
    """Gradient set ``k`` for the parameters of a SmallNet, by name."""
    rng = np.random.default_rng(2000 + k)
    return {name: torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 10.0 ** rng.uniform(-3, 0, tuple(p.shape))).astype(np.float32))
            for name, p in net.named_parameters()}


def group_names(model, groups):
    """The names of the parameters in each of ``groups`` (lists of parameters of ``model``)."""
    name_of = {id(p): n for n, p in model.named_parameters()}
    return [[name_of[id(p)] for p in g] for g in groups]
