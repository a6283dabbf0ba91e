"""The CFT block on anchor grids other than 8 x 8 (reference models/common.py:549-639, GPT(..., vert_anchors, horz_anchors)): the grid
tokeniser / de-tokenisers (cft_gpt_tokenize_grid, cft_gpt_upsample_add{,2}_grid) and the flash-style attention kernel
(cft_attention_tokens) per element against float64, the GPT module against a float64 restatement, and a whole model with every GPT
swapped for a 16 x 16 and a 4 x 8 module against the oracle walker, eager vs captured graph and through a pickle round trip.

exact_ref's ``_bilinear_taps`` and ``attention_mask`` are 8 x 8 only; their general forms are restated here.  The float64 attention
model follows the numerics in the header comment of csrc/attention_tokens.hip (online softmax over 64-key tiles).
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
from helpers import to_dev_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["f32", "bf16", "f16"]
FLOOR = {torch.bfloat16: 0.995, torch.float16: 0.99, torch.float32: None}
U24 = X.U24


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _q(x, dtype):
    return x if dtype == torch.float32 else x.to(dtype).float()


def _nhwc_cpu(y):
    return y.float().cpu().contiguous()


# ------------------------------------------------------------------------------ tokeniser
TOK_GRIDS = [(1, 1), (4, 4), (5, 7), (8, 16), (16, 16), (32, 32)]
TOK_MAPS = [(40, 48), (3, 3), (7, 5), (20, 13)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("grid", TOK_GRIDS, ids=[f"{a}x{b}" for a, b in TOK_GRIDS])
def test_tokenize_grid_per_element(dev, dtype, grid):
    """tokens = AdaptiveAvgPool2d(grid) of both streams (RGB cells first) + pos_emb, per element against float64, on maps larger than
    the grid, smaller than it (overlapping windows) and rectangular."""
    from msod_amd import ops
    va, ha = grid
    B, C = 2, 64
    for (H, W) in TOK_MAPS:
        rgb = _q(_rnd(B, C, H, W, seed=H * 7 + W), dtype)
        ir = _q(_rnd(B, C, H, W, seed=H * 7 + W + 1), dtype)
        pe = _rnd(2 * va * ha, C, seed=3, scale=0.1)
        tok = ops.gpt_tokenize(to_dev_nhwc(rgb, dev, dtype), to_dev_nhwc(ir, dev, dtype), pe.to(dev), grid=grid)
        torch.cuda.synchronize()
        assert tuple(tok.shape) == (B, 2 * va * ha, C)
        pool = lambda t: F.adaptive_avg_pool2d(t.double(), (va, ha)).reshape(B, C, -1)    # noqa: E731
        ref = torch.cat([pool(rgb), pool(ir)], 2).permute(0, 2, 1) + pe.double()
        absr = torch.cat([pool(rgb.abs()), pool(ir.abs())], 2).permute(0, 2, 1) + pe.double().abs()
        win = (H // va + 2) * (W // ha + 2)              # fp32 terms summed per window (upper bound)
        bound = ((win + 4) * U24 * absr).numpy()
        X.assert_close(tok.double().cpu().numpy(), ref.numpy(), bound, torch.float32, None, f"tokenize {grid} {H}x{W} {dtype}")


# ------------------------------------------------------------------------------ de-tokeniser
def _taps(size, n):
    """PyTorch align_corners=False source taps of an n -> size bilinear resize in float64: (i0, i1, weight of i1)."""
    src = np.maximum((np.arange(size) + 0.5) * (n / size) - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, src - i0


def _upsample_ref(g, H, W):
    """g [B, C, va, ha] -> (bilinear [B, C, H, W], the same of |g|, the largest |g| among the four taps), float64."""
    g = torch.as_tensor(X._as64(g))
    y0, y1, ly = _taps(H, g.shape[2])
    x0, x1, lx = _taps(W, g.shape[3])
    ly, lx = torch.as_tensor(ly)[:, None], torch.as_tensor(lx)[None, :]

    def blend(t):
        r = t[:, :, y0] * (1 - ly) + t[:, :, y1] * ly
        return r[..., x0] * (1 - lx) + r[..., x1] * lx

    a = g.abs()
    taps = torch.maximum(torch.maximum(a[:, :, y0][..., x0], a[:, :, y0][..., x1]), torch.maximum(a[:, :, y1][..., x0], a[:, :, y1][..., x1]))
    return blend(g), blend(a), taps


def _up_bound(ref, absb, taps, dtype, n_round=1):
    """output ulp + fp32 blend and add roundings + an fp32 rounding of the source coordinate (~16 2^-24 per axis) times the taps."""
    b = X.ulp(ref.numpy(), dtype) + (8 * U24) * absb.numpy() + (64 * U24) * taps.numpy()
    if dtype == torch.float32:
        b = b + n_round * 4 * U24 * np.abs(ref.numpy())
    return b


UP_GRIDS = [(1, 1), (4, 8), (5, 7), (16, 16), (32, 32)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("grid", UP_GRIDS, ids=[f"{a}x{b}" for a, b in UP_GRIDS])
def test_upsample_grid_per_element(dev, dtype, grid):
    """One-stream form (with and without base) and the dual + sum form, per element against a float64 general-grid bilinear, on maps
    larger and smaller than the grid."""
    from msod_amd import ops
    va, ha = grid
    B, C = 2, 64
    for (H, W) in [(40, 24), (3, 5), (16, 16)]:
        tok = _rnd(B, 2 * va * ha, C, seed=va * 100 + ha)
        g = [tok[:, s * va * ha:(s + 1) * va * ha].reshape(B, va, ha, C).permute(0, 3, 1, 2) for s in (0, 1)]
        base0, base1 = _q(_rnd(B, C, H, W, seed=5), dtype), _q(_rnd(B, C, H, W, seed=6), dtype)
        td = tok.to(dev).contiguous()
        b0, b1 = to_dev_nhwc(base0, dev, dtype), to_dev_nhwc(base1, dev, dtype)
        one = ops.gpt_upsample_add(td, 1, None, H, W, dtype, grid=grid)
        withb = ops.gpt_upsample_add(td, 0, b0, H, W, dtype, grid=grid)
        o0, o1, osum = ops.gpt_upsample_add_dual(td, b0, b1, H, W, dtype, grid=grid)
        torch.cuda.synchronize()
        u0, a0, t0 = _upsample_ref(g[0], H, W)
        u1, a1, t1 = _upsample_ref(g[1], H, W)
        what = f"{grid} {H}x{W} {dtype}"
        X.assert_close(_nhwc_cpu(one).double().numpy(), u1.numpy(), _up_bound(u1, a1, t1, dtype), dtype, FLOOR[dtype], "up " + what)
        r0 = u0 + base0.double()
        bd0 = _up_bound(r0, a0 + base0.double().abs(), t0, dtype)
        X.assert_close(_nhwc_cpu(withb).double().numpy(), r0.numpy(), bd0, dtype, FLOOR[dtype], "up+base " + what)
        assert torch.equal(withb.cpu(), o0.cpu())                         # the dual form's out0 is the one-stream expression
        r1 = u1 + base1.double()
        X.assert_close(_nhwc_cpu(o1).double().numpy(), r1.numpy(), _up_bound(r1, a1 + base1.double().abs(), t1, dtype), dtype, FLOOR[dtype],
                       "dual out1 " + what)
        rs = r0 + r1
        bs = _up_bound(rs, a0 + a1 + base0.double().abs() + base1.double().abs(), torch.maximum(t0, t1) * 2, dtype, n_round=2)
        X.assert_close(_nhwc_cpu(osum).double().numpy(), rs.numpy(), bs, dtype, FLOOR[dtype], "dual sum " + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("hw,C", [((40, 40), 64), ((13, 7), 256), ((80, 64), 2048), ((5, 3), 8)])
def test_grid_entry_points_at_8x8_equal_the_8x8_kernels(dev, dtype, hw, C):
    """At (8, 8) the grid entry points are bit-identical to cft_gpt_tokenize / cft_gpt_upsample_add{,2}."""
    from msod_amd import _lib, ops
    H, W = hw
    B = 2
    lib = _lib.load()
    dt = ops._dt(dtype)
    rgb, ir = to_dev_nhwc(_q(_rnd(B, C, H, W, seed=1), dtype), dev, dtype), to_dev_nhwc(_q(_rnd(B, C, H, W, seed=2), dtype), dev, dtype)
    pe = _rnd(128, C, seed=3).to(dev)
    t_old = torch.empty(B, 128, C, device=dev)
    t_new = torch.empty(B, 128, C, device=dev)
    _lib.check(lib.cft_gpt_tokenize(rgb.data_ptr(), C, 0, ir.data_ptr(), C, 0, pe.data_ptr(), t_old.data_ptr(), B, H, W, C, dt, ops._stream()), "tok")
    _lib.check(lib.cft_gpt_tokenize_grid(rgb.data_ptr(), C, 0, ir.data_ptr(), C, 0, pe.data_ptr(), t_new.data_ptr(), B, H, W, C, 8, 8, dt,
                                         ops._stream()), "tok grid")
    torch.cuda.synchronize()
    assert torch.equal(t_old, t_new)
    tok = _rnd(B, 128, C, seed=4).to(dev)
    outs = {}
    for name in ("old", "new"):
        o = [ops.new_nhwc(B, H, W, C, dtype, dev) for _ in range(4)]
        if name == "old":
            _lib.check(lib.cft_gpt_upsample_add(tok.data_ptr(), 1, rgb.data_ptr(), C, 0, o[0].data_ptr(), C, 0, B, H, W, C, dt, ops._stream()), "up")
            _lib.check(lib.cft_gpt_upsample_add2(tok.data_ptr(), rgb.data_ptr(), C, 0, ir.data_ptr(), C, 0, o[1].data_ptr(), C, 0,
                                                 o[2].data_ptr(), C, 0, o[3].data_ptr(), C, 0, B, H, W, C, dt, ops._stream()), "up2")
        else:
            _lib.check(lib.cft_gpt_upsample_add_grid(tok.data_ptr(), 1, rgb.data_ptr(), C, 0, o[0].data_ptr(), C, 0, B, H, W, C, 8, 8, dt,
                                                     ops._stream()), "up grid")
            _lib.check(lib.cft_gpt_upsample_add2_grid(tok.data_ptr(), rgb.data_ptr(), C, 0, ir.data_ptr(), C, 0, o[1].data_ptr(), C, 0,
                                                      o[2].data_ptr(), C, 0, o[3].data_ptr(), C, 0, B, H, W, C, 8, 8, dt, ops._stream()), "up2 grid")
        torch.cuda.synchronize()
        outs[name] = [t.cpu() for t in o]
    for a, b in zip(outs["old"], outs["new"]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------ attention
def flash_ref(q, k, v, dk, dtype, keep=None, pdrop=0.0, KB=64):
    """Float64 model of cft_attention_tokens (numerics in csrc/attention_tokens.hip) on [B, heads, T, dkp] operands (values of dtype):
    running max m_j over 64-key tiles, P rounded once per key at exp(s - m_{tile(k)}), rescaled to the final max, normaliser over the
    unrounded, undropped exponentials.  -> (ref, bound) [B, heads, T, dkp]."""
    q, k, v = (torch.as_tensor(X._as64(t)) for t in (q, k, v))
    T = k.shape[-2]
    nt = -(-T // KB)
    scale = float(np.float32(1.0) / np.sqrt(np.float32(dk)))
    s = (q @ k.transpose(-1, -2)) * scale
    sabs = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    tmax = torch.stack([s[..., j * KB:(j + 1) * KB].amax(-1) for j in range(nt)], -1)
    run = torch.cummax(tmax, -1).values                                   # m_j per query
    tile = torch.as_tensor(np.arange(T) // KB)
    mk = run[..., tile]                                                   # the running max when key k was processed
    m = run[..., -1:]
    e = torch.exp(s - mk)
    den = torch.exp(s - m).sum(-1, keepdim=True)
    if keep is not None:
        _, inv = X.drop_threshold(pdrop)
        em = e * torch.as_tensor(keep, dtype=torch.float64) * float(inv)
    else:
        em = e
    p16 = torch.as_tensor(X.rne(em.numpy(), dtype))
    resc = torch.exp(mk - m)
    ref = ((p16 * resc) @ v) / den
    # bound: as exact_ref.attention_ref, plus the rescale factors (one __expf and one fp32 multiply per tile), the longer key sum
    kdim = q.shape[-1]
    em32, va, den32 = em.float(), v.abs().float(), den.float()
    eps_e = (2 * X.GEMM_C * math.sqrt(kdim) * U24) * sabs.float() + (4 * U24) * (s - mk).abs().float() + 2.0 ** -21
    eps_r = (4 * U24) * (m - mk).abs().float() + nt * 2.0 ** -21
    if dtype != torch.float32:
        u = torch.as_tensor(X.ulp(em.numpy(), dtype)).float()
        r = em / u.double()
        near = ((r - torch.floor(r) - 0.5).abs().float() * u) <= eps_e * em32 + 1e-30
        slack = eps_e * em32 + torch.where(near, u, torch.zeros_like(u))
    else:
        slack = eps_e * em32
    pr = (p16 * resc).abs().float()
    slack = slack * resc.float() + eps_r * pr
    acc = (pr @ va) / den32
    bound = (X.GEMM_C * math.sqrt(T) * U24 * acc + (slack @ va) / den32 + (nt + 2) * U24 * acc
             + (eps_e.amax(-1, keepdim=True) + eps_r.amax(-1, keepdim=True) + (T + 70) * U24) * ref.abs().float())
    bound = bound.double().numpy() + X.ulp(ref.numpy(), dtype) + (4 * U24 * np.abs(ref.numpy()) if dtype == torch.float32 else 0.0)
    return ref.numpy(), bound


def attention_mask(seed, B, heads, T, p):
    """Keep mask [B, heads, T, T] of cft_attention_tokens: index ((b * heads + h) * T + q) * T + k."""
    t, _ = X.drop_threshold(p)
    return (X.hash32(seed, np.arange(B * heads * T * T, dtype=np.uint64)) >= t).reshape(B, heads, T, T)


def _qkv(B, heads, T, dk, dkp, dtype, seed, peaked=True):
    q, k, v = (_rnd(B, heads, T, dkp, seed=seed + i) for i in range(3))
    if peaked:
        q[:, heads // 2:] *= 6.0
    for t in (q, k, v):
        t[..., dk:] = 0
    return q, k, v


def _flat(q, k, v, dtype):
    B, heads, T, dkp = q.shape
    q, k, v = (_q(t, dtype) for t in (q, k, v))
    return q, k, v, torch.cat([t.permute(0, 2, 1, 3).reshape(B * T, heads * dkp) for t in (q, k, v)], 1)


def _attn_out(out, B, heads, T, dkp):
    return out.float().cpu().view(B, T, heads, dkp).permute(0, 2, 1, 3)


def _dkp(dk, dtype):
    step = 16 if dtype == torch.float32 else 32
    return -(-dk // step) * step


ATT_T = [2, 32, 50, 128, 256, 512, 2048]


def _floor(dtype, T):
    """The correct-rounding floors of the 8x8 attention oracle up to T = 512.  Beyond, the output (a mean over T keys) shrinks like
    1/sqrt(T) against an fp32 accumulation error that does not, so the share of elements whose fp32 value sits within that error of a
    16-bit rounding midpoint grows like sqrt(T): the allowed miss rate is scaled by sqrt(T / 512) (fp16 at T = 2048 measured 0.986-0.990;
    every element stays inside its own bound, which is what catches a wrong rounding mode or a double rounding)."""
    f = FLOOR[dtype]
    return None if f is None else 1.0 - (1.0 - f) * max(1.0, math.sqrt(T / 512))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("dk", [8, 20, 64, 128, 160])
@pytest.mark.parametrize("T", ATT_T)
def test_attention_tokens_per_element(dev, dtype, dk, T):
    """cft_attention_tokens (forced at T = 128) per element against the float64 model of its documented numerics, flat and peaked rows,
    ragged token counts; correct-rounding floors as the 8x8 kernel's; the padding columns are zero."""
    from msod_amd import ops
    B, heads = (1, 2) if T >= 2048 else (2, 2) if T >= 512 else ((4, 4) if T >= 128 else (8, 4))
    dkp = _dkp(dk, dtype)
    q, k, v, flat = _flat(*_qkv(B, heads, T, dk, dkp, dtype, 300 + dk + T), dtype)
    out = ops.attention(flat.to(dev).to(dtype), B, heads, dk, dkp, T=T, general=True)
    torch.cuda.synchronize()
    got = _attn_out(out, B, heads, T, dkp)
    ref, bound = flash_ref(q, k, v, dk, dtype)
    X.assert_close(got[..., :dk].double().numpy(), ref[..., :dk], bound[..., :dk], dtype, _floor(dtype, T), f"attention T{T} dk{dk} {dtype}")
    assert float(got[..., dk:].abs().max() if dkp > dk else 0.0) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_attention_tokens_rescale_branch(dev, dtype):
    """Guide rule 26: force the online-softmax rescale.  Key 300 (tile 4 of 8 at T = 512) is aligned with query 7 of every head so that
    query's running max jumps by ~30 there; the earlier tiles' P V is then scaled by ~exp(-30).  Against the float64 model and against the
    plain (one-pass) float64 softmax."""
    from msod_amd import ops
    B, heads, T, dk = 2, 4, 512, 64
    dkp = _dkp(dk, dtype)
    q, k, v = _qkv(B, heads, T, dk, dkp, dtype, 77, peaked=False)
    k[:, :, 300, :dk] = q[:, :, 7, :dk] * (30.0 * math.sqrt(dk) / q[:, :, 7, :dk].pow(2).sum(-1, keepdim=True))
    q, k, v, flat = _flat(q, k, v, dtype)
    out = ops.attention(flat.to(dev).to(dtype), B, heads, dk, dkp, T=T)
    torch.cuda.synchronize()
    got = _attn_out(out, B, heads, T, dkp)[..., :dk].double()
    ref, bound = flash_ref(q, k, v, dk, dtype)
    X.assert_close(got.numpy(), ref[..., :dk], bound[..., :dk], dtype, FLOOR[dtype], f"attention rescale {dtype}")
    s = (q.double() @ k.double().transpose(-1, -2)) * (1.0 / math.sqrt(dk))
    assert float((s[:, :, 7, 300] - s[:, :, 7, :256].amax(-1)).min()) > 20.0          # the jump happens at tile 4
    plain = torch.softmax(s, -1) @ v.double()
    tol = {torch.float32: 1e-5, torch.bfloat16: 2e-2, torch.float16: 4e-3}[dtype]
    assert float((got - plain[..., :dk]).abs().max()) <= tol * float(plain.abs().max())
    assert float((got[:, :, 7] - v[:, :, 300, :dk].double()).abs().max()) <= tol * 4        # query 7 is all key 300


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("dk", [32, 64, 128])
def test_attention_general_vs_existing_at_128(dev, dtype, dk):
    """At T = 128 the general kernel and the single-tile kernel each agree with the float64 model of their own numerics."""
    from msod_amd import ops
    B, heads, T = 16, 8, 128
    dkp = _dkp(dk, dtype)
    q, k, v, flat = _flat(*_qkv(B, heads, T, dk, dkp, dtype, 900 + dk), dtype)
    fd = flat.to(dev).to(dtype)
    gen = _attn_out(ops.attention(fd, B, heads, dk, dkp, T=T, general=True), B, heads, T, dkp)
    old = _attn_out(ops.attention(fd, B, heads, dk, dkp), B, heads, T, dkp)
    torch.cuda.synchronize()
    ref, bound = flash_ref(q, k, v, dk, dtype)
    X.assert_close(gen[..., :dk].double().numpy(), ref[..., :dk], bound[..., :dk], dtype, FLOOR[dtype], f"general@128 dk{dk} {dtype}")
    ref1, bound1 = X.attention_ref(q, k, v, dk, dtype)
    X.assert_close(old[..., :dk].double().numpy(), ref1[..., :dk], bound1[..., :dk], dtype, FLOOR[dtype], f"single-tile@128 dk{dk} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("T,p", [(50, 0.1), (256, 0.5), (130, 0.3)])
def test_attention_tokens_dropout_mask(dev, dtype, T, p):
    """With Q = 0 every score is equal, so with V = a block of 64 columns of the identity the output's zero pattern over those columns is the
    keep mask of the keys in the block; sweeping the blocks rebuilds the whole [B, heads, T, T] mask, which must equal the host replica of
    cft_hash32 at ((b * heads + h) * T + q) * T + k exactly.  Then random operands against the host-masked float64 model."""
    from msod_amd import ops
    B, heads, dk = 2, 4, 64
    ops.manual_dropout_seed(31337)
    seed = ops.next_dropout_seed()
    keep = attention_mask(seed, B, heads, T, p)
    got = np.zeros((B, heads, T, T), dtype=bool)
    zero = torch.zeros(B, heads, T, dk)
    kk = _rnd(B, heads, T, dk, seed=5)
    for c0 in range(0, T, dk):
        eye = torch.zeros(T, dk)
        n = min(dk, T - c0)
        eye[c0:c0 + n, :n] = torch.eye(n)
        _, _, _, flat = _flat(zero, kk, eye.expand(B, heads, T, dk), dtype)
        ops.manual_dropout_seed(31337)
        out = ops.attention(flat.to(dev).to(dtype), B, heads, dk, dk, pdrop=p, T=T)
        torch.cuda.synchronize()
        got[..., c0:c0 + n] = (_attn_out(out, B, heads, T, dk)[..., :n] != 0).numpy()
    assert np.array_equal(got, keep), f"mask mismatch at {int((got != keep).sum())} of {keep.size} positions"
    q, k, v, flat = _flat(*_qkv(B, heads, T, dk, dk, dtype, 600), dtype)
    ops.manual_dropout_seed(31337)
    out = ops.attention(flat.to(dev).to(dtype), B, heads, dk, dk, pdrop=p, T=T)
    torch.cuda.synchronize()
    ref, bound = flash_ref(q, k, v, dk, dtype, keep=keep, pdrop=p)
    X.assert_close(_attn_out(out, B, heads, T, dk).double().numpy(), ref, bound, dtype, FLOOR[dtype], f"attention drop{p} T{T} {dtype}")


# ------------------------------------------------------------------------------ GPT module
def gpt_ref(sd, rgb, ir, va, ha, h=8, p=""):
    """Float64 restatement of GPT.forward on a va x ha grid (reference models/common.py:593-639)."""
    from oracle import cft_oracle as O
    b, c, H, W = rgb.shape
    r = F.adaptive_avg_pool2d(rgb, (va, ha)).reshape(b, c, -1)
    t = F.adaptive_avg_pool2d(ir, (va, ha)).reshape(b, c, -1)
    x = torch.cat([r, t], 2).permute(0, 2, 1) + sd[p + "pos_emb"]
    n = 0
    while f"{p}trans_blocks.{n}.ln_input.weight" in sd:
        n += 1
    for i in range(n):
        x = O.transformer_block(sd, f"{p}trans_blocks.{i}.", x, h)
    x = F.layer_norm(x, (c,), sd[p + "ln_f.weight"], sd[p + "ln_f.bias"], O.LN_EPS)
    x = x.view(b, 2, va, ha, c).permute(0, 1, 4, 2, 3)
    return (F.interpolate(x[:, 0].contiguous(), size=(H, W), mode="bilinear"),
            F.interpolate(x[:, 1].contiguous(), size=(H, W), mode="bilinear"))


MOD_GRIDS = [(4, 4), (4, 8), (16, 16)]


@functools.lru_cache(maxsize=None)
def _gpt_case(d, grid, dtype):
    from msod_amd.models.common import GPT
    va, ha = grid
    m = GPT(d, h=8, vert_anchors=va, horz_anchors=ha).eval()
    with torch.no_grad():
        m.pos_emb.copy_(_rnd(*m.pos_emb.shape, seed=d + va, scale=0.2))
    B, H, W = 2, 20, 24
    rgb, ir = _q(_rnd(B, d, H, W, seed=11), dtype), _q(_rnd(B, d, H, W, seed=12), dtype)
    sd = {k: v.double() for k, v in m.state_dict().items()}
    with torch.no_grad():
        want = gpt_ref(sd, rgb.double(), ir.double(), va, ha)
    return m, rgb, ir, want


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("grid", MOD_GRIDS, ids=[f"{a}x{b}" for a, b in MOD_GRIDS])
@pytest.mark.parametrize("d", [128, 256, 1024])
def test_gpt_module_on_grid(dev, dtype, grid, d):
    """GPT(d, h=8, vert_anchors, horz_anchors) (8 blocks) against the float64 restatement: fp32 1e-3, fp16 1e-2, bf16 3e-2 (the bf16
    bound of the attention block in test_gpu_ops.test_self_attention_module), as max error over max |reference|."""
    m, rgb, ir, want = _gpt_case(d, grid, dtype)
    m = m.to(dev)                                  # (the compute dtype is the input maps' dtype)
    with torch.no_grad():
        o = m([to_dev_nhwc(rgb, dev, dtype), to_dev_nhwc(ir, dev, dtype)])
        outs = [p.materialize() for p in o]
    torch.cuda.synchronize()
    m.cpu()
    lim = {torch.float32: 1e-3, torch.float16: 1e-2, torch.bfloat16: 3e-2}[dtype]
    for got, ref in zip(outs, want):
        err = float((got.float().cpu() - ref).abs().max()) / float(ref.abs().max())
        assert err < lim, f"GPT {d} {grid} {dtype}: rel err {err:.3e}"


# ------------------------------------------------------------------------------ model
def _swap_grids(model, grid):
    """Every GPT of ``model`` re-gridded in place (a new pos_emb of [1, 2 va ha, d]); returns the GPT layer indices."""
    from msod_amd.models.common import GPT
    va, ha = grid
    idx = []
    for m in model.model:
        if isinstance(m, GPT):
            m.vert_anchors, m.horz_anchors = va, ha
            m.pos_emb = torch.nn.Parameter(torch.zeros(1, 2 * va * ha, m.n_embd))
            m.avgpool = torch.nn.AdaptiveAvgPool2d((va, ha))
            idx.append(m.i)
    return idx


MODEL_GRIDS = [(16, 16), (4, 8), (4, 16)]     # (4, 16): 128 tokens like 8 x 8, on another grid


@pytest.mark.parametrize("grid", MODEL_GRIDS, ids=[f"{a}x{b}" for a, b in MODEL_GRIDS])
def test_model_with_regridded_gpts(dev, grid, monkeypatch, tmp_path):
    """yolov5s_fusion_transformerx3_vedai at 256 x 256 with every GPT on ``grid``: fp32 pred and raw maps match the oracle walker, with the
    two Add2 layers and the Add behind each GPT run as ONE grid de-tokeniser launch (Model.cft_fusion_plan); eager and captured-graph
    outputs are bit-identical; torch.save + compat.attempt_load runs and gives the same output."""
    from msod_amd import compat
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    from oracle import cft_oracle as O
    va, ha = grid
    cfg = named_config("yolov5s_fusion_transformerx3_vedai")
    model = Model(cfg)
    assert len(_swap_grids(model, grid)) == 3
    sd = seeded_state_dict(model.state_dict(), 9)
    model.load_state_dict(sd)
    ck = str(tmp_path / "regridded.pt")
    torch.save({"model": model}, ck)
    rgb, ir = seeded_inputs(2, 256, 256, 9)
    if va == ha:
        monkeypatch.setattr(O, "gpt", functools.partial(O.gpt, anchors=va))
    else:
        monkeypatch.setattr(O, "gpt", lambda sd_, p, r, i, h=8, anchors=8: gpt_ref(sd_, r, i, va, ha, h, p))
    want_pred, want_raw = O.OracleModel(cfg)(sd, rgb, ir)
    model = model.to(dev).set_compute_dtype(torch.float32)
    from msod_amd import ops
    log = []
    with torch.no_grad():
        ops.set_launch_log(log)
        try:
            e_pred, e_raw = model.forward_once(rgb.to(dev), ir.to(dev))
        finally:
            ops.set_launch_log(None)
        e_pred, e_raw = e_pred.clone(), [r.clone() for r in e_raw]
        model.capture(2, 256, 256)
        for _ in range(2):
            g_pred, g_raw = model(rgb.to(dev), ir.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(e_pred, g_pred) and all(torch.equal(a, b) for a, b in zip(e_raw, g_raw))
    model.release_graphs()
    assert sum(1 for rec in log if rec[0] == "cft_upsample_add") == 3                  # one dual launch per GPT block
    for a, b in zip(e_raw, want_raw):
        assert a.shape == b.shape
        assert (a.cpu() - b).abs().max().item() <= 1e-3
    assert torch.allclose(e_pred.cpu(), want_pred, rtol=1e-3, atol=1e-3)
    loaded = compat.attempt_load(ck, map_location="cpu")
    gpts = [m for m in loaded.model if type(m).__name__ == "GPT"]
    assert len(gpts) == 3 and all((m.vert_anchors, m.horz_anchors) == grid for m in gpts)
    loaded = loaded.to(dev).set_compute_dtype(torch.float32)
    with torch.no_grad():
        l_pred, l_raw = loaded(rgb.to(dev), ir.to(dev))
    torch.cuda.synchronize()
    for a, b in zip(l_raw, want_raw):                  # (attempt_load fuses: BatchNorm folded at load instead of at pack time)
        assert (a.cpu() - b).abs().max().item() <= 1e-3
    assert torch.allclose(l_pred.cpu(), want_pred, rtol=1e-3, atol=1e-3)
    assert torch.allclose(l_pred, e_pred, rtol=1e-4, atol=1e-3)
