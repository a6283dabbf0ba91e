"""Float64 oracle of the Adam / AdamW step (``cft_adam_step``, ``csrc/optim.hip``) and the per-element error bound the tests hold the
kernel to.

One step is restated in float64 from float32 state, with the constants rounded to float32 exactly as the C entry and the prepare
kernel form them from the doubles of ``param_groups``:

    w1 = f32(1 - beta1)   b2 = f32(beta2)   w2 = f32(1 - beta2)   eps = f32(eps)   wd = f32(wd)   decay = f32(1 - lr * wd)
    step_size = f32(lr / (1 - beta1 ** step))        bc2_sqrt = f32(sqrt(1 - beta2 ** step))

    g0  = g * f32(1 / grad_scale)                      (with a GradScaler)
    g1  = g0 + wd * p,  p0 = p                         (Adam's L2 term, wd != 0)
    p0  = p * decay,    g1 = g0                        (AdamW's decoupled decay, wd != 0)
    m1  = m + w1 * (g1 - m)
    v1  = b2 * v + w2 * g1 * g1
    den = sqrt(v1) / bc2_sqrt + eps
    q   = step_size * m1 / den;   p1 = p0 - q

Bound: first order, propagated through the statements above, u = 2^-24 (half an ulp of a float32 result relative to it), T = the sum
of the absolute values of the terms, as in ``optim_ref``.  Every rounding of the float32 evaluation errs by at most u times its
result; an input error dx passes through f as |f'| dx.

    dg   = u |g0|  (the unscale multiply)  +  2u (|g0| + wd |p|)  (the L2 multiply and add, fused or not)
    dm   = w1 dg + 3u (|m| + w1 (T_g1 + |m|))                   (subtract, multiply, add)
    dv   = 2 w2 |g1| dg + 4u v1                                 (w2 * g1, * g1, b2 * v, the add; every term is >= 0, so T = v1)
    ds   = dv / (2 sqrt(v1)) + u sqrt(v1)                       (first term 0 where v1 = 0: then g1 = 0 and dv = 0)
    dden = ds / bc2_sqrt + 3u den                               (divide, add, and the float32 rounding of bc2_sqrt itself)
    dq   = step_size dm / den + |q| dden / den + 4u |q|         (the product, the quotient, step_size's own rounding, slack for pow)
    dp   = 2u |p0| (AdamW: decay's rounding and the multiply) + dq + 2u (|p0| + |q|)      (the final add)

The bound assumes no float32 underflow in ``g1 * g1``: test gradients are exactly 0 or at least 1e-12 in magnitude
(``log_uniform`` below gives magnitudes, not a normal distribution with a tail towards 0).  The device's double ``pow`` may differ from
libm's in the last bit: 2^-53 relative, far inside the 4u |q| term.

torch's own float32 CPU step (``foreach=False``) stays within 0.50 (parameters), 0.65 (``exp_avg``) and 0.50 (``exp_avg_sq``) of the
bound on 200 001-element vectors spanning seven decades; the tests assert at most 1 against float64 and at most 1 against twice the
bound between two float32 implementations.
"""
import math

import numpy as np
import torch

from optim_ref import f32, worst  # noqa: F401  (worst: the ratio the tests assert on)

U = 2.0 ** -24


def _f64(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def adam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale=None):
    """One step from float32 ``p``, ``g``, ``m``, ``v`` (``None``: the zero moments of a first step); ``step`` is the count this
    step brings the tensor to (1 for the first).  Returns float64 ``(p1, m1, v1, bound_p, bound_m, bound_v)``."""
    lr, beta1, beta2, step = float(lr), float(beta1), float(beta2), float(step)
    w1, b2, w2 = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2)
    epsf, wd, decay = f32(eps), f32(weight_decay), f32(1.0 - lr * float(weight_decay))
    step_size = f32(lr / (1.0 - beta1 ** step))
    bc2_sqrt = f32(math.sqrt(1.0 - beta2 ** step))
    p, g = _f64(p), _f64(g)
    m = np.zeros_like(p) if m is None else _f64(m)
    v = np.zeros_like(p) if v is None else _f64(v)
    if grad_scale is not None:
        g0 = g * f32(1.0 / float(grad_scale))
        dg = U * np.abs(g0)
    else:
        g0, dg = g, np.zeros_like(g)
    g1, t_g1, p0, dp = g0, np.abs(g0), p, np.zeros_like(p)
    if wd != 0.0:
        if decoupled:
            p0 = p * decay
            dp = 2 * U * np.abs(p0)
        else:
            g1 = g0 + wd * p
            t_g1 = np.abs(g0) + wd * np.abs(p)
            dg = dg + 2 * U * t_g1
    m1 = m + w1 * (g1 - m)
    dm = w1 * dg + 3 * U * (np.abs(m) + w1 * (t_g1 + np.abs(m)))
    v1 = b2 * v + w2 * g1 * g1
    dv = 2 * w2 * np.abs(g1) * dg + 4 * U * v1
    s = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(v1 > 0, dv / (2 * s), 0.0) + U * s
    den = s / bc2_sqrt + epsf
    dden = ds / bc2_sqrt + 3 * U * den
    q = step_size * m1 / den
    dq = step_size * dm / den + np.abs(q) * dden / den + 4 * U * np.abs(q)
    dp = dp + dq + 2 * U * (np.abs(p0) + np.abs(q))
    return p0 - q, m1, v1, dp, dm, dv


def log_uniform(rng, n, lo, hi):
    """``n`` float32 values of random sign whose magnitudes are 10 ** uniform(lo, hi): no value nearer to 0 than 10 ** lo."""
    return torch.from_numpy((rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32))


def step_grads(rng, n, k):
    """Gradient ``k`` of the test sequences: magnitudes 1e-6 .. 10, step 1 with a block of exact zeros, step 2 tiny (1e-10 .. 1e-8,
    where ``den`` is near ``eps``)."""
    if k == 2:
        return log_uniform(rng, n, -10, -8)
    g = log_uniform(rng, n, -6, 1)
    if k == 1:
        g[n // 4:n // 2 + 1] = 0.0
    return g
