"""Float64 per-element oracles of the HIP kernels (a plain module, imported by the tests that use it).

``helpers.rel_err`` divides the largest error by the largest reference value, so an error that is small against the tensor's
maximum (a rounding-mode mistake, a wrong bias on a low-magnitude channel, one bad row at a tile edge) passes it.  The helpers
here hold every element to its own bound instead:

    |got - ref64| <= ulp_out(ref64) + c * sqrt(K) * 2^-24 * sum_k |a_k w_k| + act_err(v) (+ 2^-24 |v| per fp32 rounding)

and measure, for 16-bit outputs, the fraction of elements that equal RNE(ref64) (the correct-rounding rate).  A kernel that
rounds correctly from an fp32 accumulator close to the exact value lands there almost always; truncation or a double rounding
do not.  The references are computed from the operands the kernel actually sees (already rounded to the storage dtype).

Also here: a host replica of ``cft_hash32`` (csrc/cft_common.h) that rebuilds the dropout masks of ``cft_dropout`` and of the
attention kernel exactly.
"""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
_MANT = {torch.bfloat16: (8, -125), torch.float16: (11, -13)}     # significant bits, smallest exponent e of a normal m * 2^e, m in [0.5, 1)
GEMM_C = 2.0          # the c of the accumulation term: fp32 sums of K products, rounding errors of random sign


# ------------------------------------------------------------------------------ rounding
def _as64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def ulp(x, dtype):
    """One unit in the last place of ``dtype`` at |x| (float64 array); 0 for fp32 (its rounding is an explicit 2^-24 |v| term)."""
    x = _as64(x)
    if dtype == torch.float32:
        return np.zeros_like(x)
    bits, emin = _MANT[dtype]
    _, e = np.frexp(x)
    e = np.where(x == 0, emin, e)
    return np.ldexp(1.0, np.maximum(e, emin) - bits)


def rne(x, dtype):
    """float64 -> nearest ``dtype`` value, ties to even, in ONE rounding (float64 result).  numpy's round() is ties-to-even and
    x / ulp is exact (ulp is a power of two), so this is the correctly rounded conversion, subnormals included."""
    x = _as64(x)
    if dtype == torch.float32:
        return x.astype(np.float32).astype(np.float64)
    u = ulp(x, dtype)
    return np.round(x / u) * u


def rtz(x, dtype):
    """float64 -> ``dtype`` by truncation (the rounding-mode mistake the rate check must catch)."""
    x = _as64(x)
    u = ulp(x, dtype)
    return np.trunc(x / u) * u


# ------------------------------------------------------------------------------ error model
def act_err(v, act):
    """Documented approximation bound of the fused activations at pre-activation v (float64 array): SiLU = v * rcp(1 + __expf(-v))
    (a few fp32 ulps of the result plus the exp argument's rounding, |v|^2 s(1-s) 2^-24 <= 0.45 * 2^-24); GELU by A&S 7.1.26
    (|erf error| <= 1.5e-7, so 0.5 |v| 1.5e-7) plus a few fp32 ulps."""
    v = np.abs(_as64(v))
    if act == 1:
        return 8 * U24 * v + U24
    if act == 2:
        return 0.5 * v * 1.5e-7 + 8 * U24 * v + U24
    return np.zeros_like(v)


ACT_SLOPE = {0: 1.0, 1: 1.1, 2: 1.13}     # max |act'(v)|: how far an accumulation error moves the activated value


def gemm_bound(ref, absacc, K, dtype_out, act=0, v=None, fp32_roundings=2):
    """Per-element bound of one GEMM + bias + act (+ residual) output (see the module docstring)."""
    ref = _as64(ref)
    b = ulp(ref, dtype_out) + ACT_SLOPE[act] * GEMM_C * math.sqrt(K) * U24 * _as64(absacc)
    if act:
        b = b + act_err(v, act)
    if dtype_out == torch.float32:
        b = b + fp32_roundings * U24 * np.abs(ref)
    return b


def check(got, ref, bound, dtype):
    """-> dict(n, bad = #elements over their bound, worst = max |err| / bound, rate = fraction equal to RNE(ref) (16-bit only))."""
    got, ref, bound = _as64(got), _as64(ref), _as64(bound)
    err = np.abs(got - ref)
    out = {"n": int(got.size), "bad": int((err > bound).sum()), "worst": float((err / np.maximum(bound, 1e-300)).max()) if got.size else 0.0}
    if dtype != torch.float32:
        out["rate"] = float((got == rne(ref, dtype)).mean())
    return out


def passes(got, ref, bound, dtype, floor=None):
    r = check(got, ref, bound, dtype)
    return r["bad"] == 0 and (floor is None or r.get("rate", 1.0) >= floor)


def assert_close(got, ref, bound, dtype, floor=None, what=""):
    r = check(got, ref, bound, dtype)
    print(f"[oracle] {what}: n={r['n']} bad={r['bad']} worst={r['worst']:.3f}" + (f" rate={r['rate']:.5f} floor={floor}" if "rate" in r else ""))
    assert r["bad"] == 0, f"{what}: {r['bad']} of {r['n']} elements outside their bound (worst {r['worst']:.2f} x bound)"
    if floor is not None and "rate" in r:
        assert r["rate"] >= floor, f"{what}: correct-rounding rate {r['rate']:.5f} < floor {floor}"
    return r


# ------------------------------------------------------------------------------ convolution / linear
def sample_rows(B, Ho, Wo, n_random=3000, seed=0, tiles=(64, 128, 192, 208, 224, 256), border_images=2):
    """Output rows (m = (b * Ho + y) * Wo + x) where a GEMM goes wrong first: first and last row of every M tile of each tile height
    the kernels launch, the ragged last rows, border-tap rows (of the first and last ``border_images`` images) and random rows."""
    M = B * Ho * Wo
    m = np.arange(M)
    keep = m >= M - 64
    for t in tiles:
        keep |= (m % t == 0) | (m % t == t - 1)
    img, rem = m // (Ho * Wo), m % (Ho * Wo)
    y, x = rem // Wo, rem % Wo
    edge = (y == 0) | (y == Ho - 1) | (x == 0) | (x == Wo - 1)
    keep |= edge & ((img < border_images) | (img >= B - border_images))
    rng = np.random.RandomState(seed)
    keep[rng.randint(0, M, size=min(n_random, M))] = True
    return np.nonzero(keep)[0]


def conv_ref(x, w, bias, stride, rows=None):
    """Float64 conv2d (padding k // 2) on output rows ``rows`` (None: all).  x [B,C,H,W], w [N,C,k,k] (already in the storage
    dtype's values), bias [N] or None -> (ref [R, N], sum_k |a_k w_k| [R, N], rows)."""
    x64, w64 = x.detach().double().cpu(), w.detach().double().cpu()
    B, C, H, W = x64.shape
    N, _, k, _ = w64.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    if rows is None:
        rows = np.arange(B * Ho * Wo)
    rows = torch.as_tensor(rows, dtype=torch.long)
    xp = torch.nn.functional.pad(x64, (p, p, p, p))
    bi, rem = rows // (Ho * Wo), rows % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    ky = torch.arange(k)
    yy = (oy * stride)[:, None, None] + ky[None, :, None]
    xx = (ox * stride)[:, None, None] + ky[None, None, :]
    patches = xp[bi[:, None, None], :, yy, xx].reshape(len(rows), k * k * C)     # [R, k, k, C]: advanced indices first
    wm = w64.permute(0, 2, 3, 1).reshape(N, k * k * C)
    ref = patches @ wm.T
    absacc = patches.abs() @ wm.abs().T
    if bias is not None:
        b64 = bias.detach().double().cpu()
        ref = ref + b64
        absacc = absacc + b64.abs()
    return ref.numpy(), absacc.numpy(), rows.numpy()


def act64(v, act):
    v = torch.as_tensor(v, dtype=torch.float64)
    if act == 1:
        return torch.nn.functional.silu(v).numpy()
    if act == 2:      # 0.5 v erfc(-v / sqrt 2): torch's 0.5 v (1 + erf(v / sqrt 2)) cancels to 0 below v ~ -6 even in float64
        return (0.5 * v * torch.special.erfc(-v * 0.7071067811865476)).numpy()
    return v.numpy()


def nhwc_rows(y, rows, n):
    """Rows ``rows`` of a device / CPU [B,C,H,W] output as a float64 [R, n] array (first n channels)."""
    y = y.detach()
    B, C, H, W = y.shape
    flat = y.permute(0, 2, 3, 1).reshape(B * H * W, C)
    idx = torch.as_tensor(rows, dtype=torch.long, device=flat.device)
    return flat.index_select(0, idx)[:, :n].double().cpu().numpy()


# ------------------------------------------------------------------------------ CFT tokeniser / de-tokeniser
def _bilinear_taps(size):
    """PyTorch align_corners=False source taps of an 8 -> size upsample in float64: (i0, i1, weight of i1) per output index."""
    src = np.maximum((np.arange(size) + 0.5) * (8.0 / size) - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, 7)
    return i0, i1, src - i0


def upsample_ref(grid, H, W):
    """grid [B, C, 8, 8] -> (bilinear [B, C, H, W] float64, the same of |grid| (the magnitude the fp32 blend works on), the largest
    |grid| among the four taps (what an fp32 rounding of the source coordinate, ~16 2^-24 per axis, moves the value by))."""
    g = torch.as_tensor(_as64(grid))
    y0, y1, ly = _bilinear_taps(H)
    x0, x1, lx = _bilinear_taps(W)
    ly, lx = torch.as_tensor(ly)[:, None], torch.as_tensor(lx)[None, :]

    def blend(t):
        r = t[:, :, y0] * (1 - ly) + t[:, :, y1] * ly            # [B, C, H, 8]
        return r[..., x0] * (1 - lx) + r[..., x1] * lx

    a = g.abs()
    taps = torch.maximum(torch.maximum(a[:, :, y0][..., x0], a[:, :, y0][..., x1]), torch.maximum(a[:, :, y1][..., x0], a[:, :, y1][..., x1]))
    return blend(g).numpy(), blend(a).numpy(), taps.numpy()


# ------------------------------------------------------------------------------ counter-based dropout
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(seed, i):
    """splitmix64 output for state seed + (i + 1) * golden ratio (numpy uint64, wraps mod 2^64): the hash of csrc/cft_common.h."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.asarray(i, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hash32(seed, i):
    """cft_hash32(seed, i): the upper 32 bits of splitmix64."""
    return (splitmix64(seed, i) >> np.uint64(32)).astype(np.uint32)


def drop_threshold(p):
    """The kernels' keep test hash >= (uint32)((double)(float)p * 2^32) and scale (float)1 / (1 - (float)p)."""
    pf = np.float32(p)
    return np.uint32(int(float(pf) * 4294967296.0)), np.float32(1.0) / (np.float32(1.0) - pf)


def dropout_mask(seed, n, p):
    """Keep mask of cft_dropout over n elements: element index = flat index (idx * GE + e)."""
    t, _ = drop_threshold(p)
    return hash32(seed, np.arange(n, dtype=np.uint64)) >= t


def attention_mask(seed, B, heads, p):
    """Keep mask [B, heads, 128 queries, 128 keys] of the attention kernel: index ((b * heads + h) * 128 + q) * 128 + k."""
    t, _ = drop_threshold(p)
    return (hash32(seed, np.arange(B * heads * 128 * 128, dtype=np.uint64)) >= t).reshape(B, heads, 128, 128)


def dropout_ref(x, seed, p, dtype):
    """cft_dropout's result, bit for bit: RNE_dtype(fp32(x * inv_keep)) on kept elements, 0 elsewhere (x: values of ``dtype``)."""
    x32 = _as64(x).astype(np.float32).reshape(-1)
    _, inv = drop_threshold(p)
    keep = dropout_mask(seed, x32.size, p)
    return rne(np.where(keep, x32 * inv, np.float32(0.0)).astype(np.float64), dtype)


# ------------------------------------------------------------------------------ attention
def attention_ref(q, k, v, dk, dtype, keep=None, pdrop=0.0):
    """Float64 model of the attention kernel's numerics on [B, heads, 128, dkp] operands (values of ``dtype``):
    S = Q K^T * fp32(1/sqrt(dk)); E = exp(S - rowmax) unnormalised; the normaliser sums the UNROUNDED, unmasked E; the MFMA operand
    is RNE_dtype(E * keep * fp32(1/(1-p))); O = (P V) / sum, rounded once.  -> (ref, bound) [B, heads, 128, dkp]."""
    q, k, v = (torch.as_tensor(_as64(t)) for t in (q, k, v))
    scale = float(np.float32(1.0) / np.sqrt(np.float32(dk)))
    s = (q @ k.transpose(-1, -2)) * scale
    sabs = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    if keep is not None:
        _, inv = drop_threshold(pdrop)
        em = e * torch.as_tensor(keep, dtype=torch.float64) * float(inv)
    else:
        em = e
    p16 = torch.as_tensor(rne(em.numpy(), dtype))
    ref = (p16 @ v) / den
    # bound: output rounding + fp32 accumulation of P V + the kernel's own error in each exponential (fp32 scores: accumulation
    # over dkp, x scale, minus the max; __expf) and, where that error can move E across a rounding midpoint, one ulp of E
    # (the bound itself is computed in float32: it needs no more)
    kdim = q.shape[-1]
    em32, va, den32 = em.float(), v.abs().float(), den.float()
    eps_e = (2 * GEMM_C * math.sqrt(kdim) * U24) * sabs.float() + (4 * U24) * (s - m).abs().float() + 2.0 ** -21
    if dtype != torch.float32:
        u = torch.as_tensor(ulp(em.numpy(), dtype)).float()
        r = em / u.double()
        near = ((r - torch.floor(r) - 0.5).abs().float() * u) <= eps_e * em32 + 1e-30
        slack = eps_e * em32 + torch.where(near, u, torch.zeros_like(u))
    else:
        slack = eps_e * em32
    acc = (p16.abs().float() @ va) / den32
    bound = (GEMM_C * math.sqrt(128) * U24 * acc + (slack @ va) / den32
             + (eps_e.amax(-1, keepdim=True) + 130 * U24) * ref.abs().float())
    bound = bound.double().numpy() + ulp(ref.numpy(), dtype) + (4 * U24 * np.abs(ref.numpy()) if dtype == torch.float32 else 0.0)
    return ref.numpy(), bound
