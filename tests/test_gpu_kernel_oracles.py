"""Per-element checks of the root kernels against float64 (tests/exact_ref.py): every output element within its own error bound
(output ulp + fp32 accumulation + activation approximation) and, for 16-bit outputs, a correct-rounding rate of at least the floor
below.  ``helpers.rel_err`` (max error over max reference) cannot see a rounding-mode mistake or a wrong value where the tensor is
small; these checks can (tests/test_kernel_oracles_host.py shows each such mutation caught).

Correct-rounding floors (fraction of elements equal to RNE(ref64)), calibrated on the MI355X: set between the lowest rate measured
there and what the host mutations produce (round-toward-zero ~0.5, a double rounding through fp16 ~0.94 for bf16).  Lowest measured
rate per kernel, bf16 / fp16:
    conv2d (CONV_CASES, epilogue forms)  0.9997 / 0.9974      every tile configuration    0.9999 / 0.9995
    asm GEMM (96, 961-964)               0.9998 / 0.9980      wide benchmarked layers     0.9997 / 0.9980
    channel slices                       0.9999 / 0.9994      attention                   0.9996 / 0.9966
    LayerNorm / LayerNorm + reduce       0.99995 / 0.9997     BatchNorm (channels >= 1)   0.9998 / 0.9995
    gpt_upsample_add                     0.9993 / 0.9953      gpt_upsample_add2           0.9996 / 0.9980
  -> FLOOR 0.995 / 0.99.  The GELU linear at K = C: 0.9906 / 0.9776 (the A&S erfc's absolute error is a few output ulps where GELU
  is small) -> FLOOR_GELU 0.98 / 0.96.  BatchNorm channel 0 (|mean| = 1e4 sigma, 0.72 / 0.85: the fp32 affine form x * sc + sh
  cancels there) is held to its bound only.

GELU tail measured on the device (relative error of the fp32 output, max over [v - 1, v)): 5.2e-5 at -2, 4.7e-4 at -3, 1.6e-3 at
-4, 3.6e-3 at -5, 6.5e-3 at -6; fp16 output 8.3e-4 at -3, 2.0e-2 at -4 (subnormal outputs).  The documented absolute bound holds.
"""
import math

import numpy as np
import pytest
import torch

import exact_ref as X
from helpers import to_dev_nhwc
from test_gpu_ops import ASM_CASES, CONV_CASES, TILE_VARIANTS

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["f32", "bf16", "f16"]
LOWP = [torch.bfloat16, torch.float16]
FLOOR = {torch.bfloat16: 0.995, torch.float16: 0.99, torch.float32: None}
FLOOR_GELU = {torch.bfloat16: 0.98, torch.float16: 0.96, torch.float32: None}


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _q(x, dtype):
    return x if dtype == torch.float32 else x.to(dtype).float()


def _with_variant(variant, fn):
    from msod_amd import _lib
    lib = _lib.load()
    lib.cft_set_conv_variant(variant)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.cft_set_conv_variant(0)
    return out


def _conv_check(dev, dtype, B, H, W, Cin, Cout, k, s, act, use_res, variant=0, seed=1, sample=False, out_dtype=None, what=""):
    """cft_conv2d on seeded operands, every (or a sample of the) output element(s) against float64."""
    from msod_amd import ops
    out_dtype = out_dtype or dtype
    x = _q(_rnd(B, Cin, H, W, seed=seed), dtype)
    w = _q(_rnd(Cout, Cin, k, k, seed=seed + 1, scale=1.0 / math.sqrt(Cin * k * k)), dtype)
    b = _rnd(Cout, seed=seed + 2, scale=0.5)
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    pk = ops.pack_conv(w, b, dtype, s=s, device=dev)
    res = _q(_rnd(B, pk.n, Ho, Wo, seed=seed + 3), out_dtype) if use_res else None
    xd = to_dev_nhwc(x, dev, dtype)
    rd = to_dev_nhwc(res, dev, out_dtype) if use_res else None
    y = _with_variant(variant, lambda: ops.conv2d(xd, pk, act, residual=rd, out_dtype=out_dtype))
    rows = X.sample_rows(B, Ho, Wo, n_random=2000, seed=seed) if sample else None
    v, absacc, rows = X.conv_ref(x, w, b, s, rows)
    ref = X.act64(v, act)
    if use_res:
        ref = ref + X.nhwc_rows(res, rows, Cout)
    bound = X.gemm_bound(ref, absacc, k * k * Cin, out_dtype, act, v, fp32_roundings=3 if use_res else 2)
    return X.assert_close(X.nhwc_rows(y, rows, Cout), ref, bound, out_dtype, FLOOR[out_dtype], what or f"conv {dtype} v{variant}")


# ------------------------------------------------------------------------------ cft_conv2d
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CONV_CASES, ids=[f"c{i}" for i in range(len(CONV_CASES))])
def test_conv2d_per_element(dev, dtype, case):
    _conv_check(dev, dtype, *case, what=f"conv {case} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("variant", TILE_VARIANTS)
def test_conv2d_every_tile_configuration_per_element(dev, dtype, variant):
    """Ragged M (2*33*31 rows), N tail (320), border taps, SiLU + shortcut: each tile configuration."""
    _conv_check(dev, dtype, 2, 33, 31, 64, 320, 3, 1, 1, True, variant=variant, seed=31, what=f"tile v{variant} {dtype}")


ASM_RUNS = [(c, v) for c in range(len(ASM_CASES)) for v in (96, 964)] + [(0, v) for v in (961, 962, 963)] + [(2, v) for v in (961, 962, 963)]


@pytest.mark.parametrize("dtype", LOWP, ids=["bf16", "f16"])
@pytest.mark.parametrize("ci,variant", ASM_RUNS, ids=[f"a{c}-v{v}" for c, v in ASM_RUNS])
def test_asm_gemm_per_element(dev, dtype, ci, variant):
    B, H, W, Cin, Cout, k, s, use_res = ASM_CASES[ci]
    _conv_check(dev, dtype, B, H, W, Cin, Cout, k, s, 1, use_res, variant=variant, seed=91, sample=True, what=f"asm a{ci} v{variant} {dtype}")


@pytest.mark.parametrize("dtype", LOWP, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(64, 40, 256, 256, True), (64, 20, 512, 512, False)], ids=["p4_256ch", "p5_512ch"])
def test_wide_layers_at_the_benchmarked_row_count_per_element(dev, dtype, shape):
    """The benchmarked wide 3x3 layers with the automatic kernel choice; the float64 reference on a row sample (tile edges, border
    taps of the first and last images, ragged rows, random rows)."""
    B, HW, Cin, Cout, use_res = shape
    _conv_check(dev, dtype, B, HW, HW, Cin, Cout, 3, 1, 1, use_res, seed=51, sample=True, what=f"wide {shape} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "silu", "gelu"])
def test_conv2d_epilogue_forms_per_element(dev, dtype, act):
    """Each activation with and without a shortcut, and the 16-bit-in / fp32-out form (with an fp32 shortcut)."""
    _conv_check(dev, dtype, 2, 11, 13, 64, 72, 3, 1, act, False, seed=61)
    _conv_check(dev, dtype, 2, 11, 13, 64, 72, 1, 1, act, True, seed=62)
    _conv_check(dev, dtype, 2, 11, 13, 64, 72, 3, 1, act, True, seed=63, out_dtype=torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_conv2d_channel_slices_per_element(dev, dtype):
    """Input read from a channel slice, output into a slice of a wider buffer, shortcut aliasing the output."""
    from msod_amd import ops
    B, H, W, C = 2, 12, 12, 64
    wide = _q(_rnd(B, 2 * C, H, W, seed=5), dtype)
    w = _q(_rnd(C, C, 3, 3, seed=6, scale=1.0 / math.sqrt(C * 9)), dtype)
    b = _rnd(C, seed=7, scale=0.1)
    buf = to_dev_nhwc(wide, dev, dtype)
    pk = ops.pack_conv(w, b, dtype, device=dev)
    ops.conv2d(buf[:, C:], pk, 1, residual=buf[:, :C], out=buf[:, :C])
    torch.cuda.synchronize()
    v, absacc, rows = X.conv_ref(wide[:, C:], w, b, 1)
    ref = X.act64(v, 1) + X.nhwc_rows(wide[:, :C], rows, C)
    X.assert_close(X.nhwc_rows(buf[:, :C], rows, C), ref, X.gemm_bound(ref, absacc, 9 * C, dtype, 1, v, 3), dtype, FLOOR[dtype], f"slices {dtype}")
    assert torch.equal(buf[:, C:].float().cpu(), wide[:, C:])


# ------------------------------------------------------------------------------ linear, split-K, LayerNorm
def _row_sample(rows):
    return X.sample_rows(1, rows, 1, n_random=1500) if rows > 2048 else np.arange(rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows", [8192, 300])
@pytest.mark.parametrize("C", [64, 256, 320, 1024, 1280])
def test_linear_gelu_and_fp32_residual_stream(dev, dtype, rows, C):
    from msod_amd import ops
    x = _q(_rnd(rows, C, seed=C), dtype)
    w = _q(_rnd(C, C, seed=C + 1, scale=2.0 / math.sqrt(C)), dtype)
    b = _rnd(C, seed=C + 2, scale=0.3)
    r = _rnd(rows, C, seed=C + 3)
    pk = ops.pack_conv(w, b, dtype, device=dev)
    xd = x.to(dev).to(dtype)
    g = ops.linear(xd, pk, ops.ACT_GELU)
    rd = r.to(dev)
    ops.linear(xd, pk, ops.ACT_NONE, residual=rd, out=rd, out_dtype=torch.float32)
    torch.cuda.synchronize()
    sel = _row_sample(rows)
    xs = x[sel].double()
    v = (xs @ w.double().T + b.double()).numpy()
    absacc = (xs.abs() @ w.double().abs().T + b.double().abs()).numpy()
    ref = X.act64(v, 2)
    X.assert_close(g[sel][:, :C].double().cpu().numpy(), ref, X.gemm_bound(ref, absacc, C, dtype, 2, v), dtype, FLOOR_GELU[dtype], f"linear gelu {rows}x{C} {dtype}")
    ref2 = v + r[sel].double().numpy()
    X.assert_close(rd[sel][:, :C].double().cpu().numpy(), ref2, X.gemm_bound(ref2, absacc, C, torch.float32, 0, v, 3), torch.float32, None,
                   f"linear +res32 {rows}x{C} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows", [8192, 300])
@pytest.mark.parametrize("n,K,splits", [(1024, 1024, 2), (320, 1280, 4)])
def test_linear_splitk_parts_and_layernorm_reduce(dev, dtype, rows, n, K, splits):
    """Each fp32 partial sum against its float64 slice product; the reduced LayerNorm per element (see test_layernorm_per_element)."""
    from msod_amd import ops
    x = _q(_rnd(rows, K, seed=71), dtype)
    w = _q(_rnd(n, K, seed=72, scale=1.0 / math.sqrt(K)), dtype)
    b = _rnd(n, seed=73, scale=0.1)
    pk = ops.pack_conv(w, b, dtype, device=dev)
    parts = ops.linear_splitk(x.to(dev).to(dtype), pk, splits)
    res = _rnd(rows, pk.n, seed=74).to(dev)
    gamma, beta = (1.0 + 0.1 * _rnd(pk.n, seed=75)).to(dev), (0.1 * _rnd(pk.n, seed=76)).to(dev)
    xr = res.clone()
    y = ops.layernorm_reduce(xr, parts, gamma, beta, dtype)
    torch.cuda.synchronize()
    sel = _row_sample(rows)
    kc = K // splits
    for s_ in range(splits):
        xs, ws = x[sel, s_ * kc:(s_ + 1) * kc].double(), w[:, s_ * kc:(s_ + 1) * kc].double()
        bb = b.double() if s_ == 0 else torch.zeros(n, dtype=torch.float64)
        ref = (xs @ ws.T + bb).numpy()
        absacc = (xs.abs() @ ws.abs().T + bb.abs()).numpy()
        X.assert_close(parts[s_][sel][:, :n].double().cpu().numpy(), ref, X.gemm_bound(ref, absacc, kc, torch.float32), torch.float32, None,
                       f"splitk part {s_} {rows} {dtype}")
    _ln_check(xr[sel].cpu(), gamma.cpu(), beta.cpu(), y[sel].cpu(), dtype, f"layernorm_reduce {rows}x{pk.n} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("C", [4, 512, 516, 1280, 1284, 4096])
def test_layernorm_reduce_every_instantiation(dev, dtype, C):
    """cft_layernorm_reduce at 5 rows on the widths of LN_SHAPES (three partial sums): the folded stream against the float64 sum of its
    terms, the LayerNorm of it per element."""
    from msod_amd import ops
    rows, nparts = 5, 3
    x = _rnd(rows, C, seed=81) * 3 + 1
    parts = _rnd(nparts, rows, C, seed=82)
    g, b = _rnd(C, seed=83) * 0.2 + 1, _rnd(C, seed=84) * 0.1
    xr = x.to(dev)
    y = ops.layernorm_reduce(xr, parts.to(dev), g.to(dev), b.to(dev), dtype)
    torch.cuda.synchronize()
    ref = x.double() + parts.double().sum(0)
    mag = x.double().abs() + parts.double().abs().sum(0)
    assert ((xr.cpu().double() - ref).abs() <= nparts * X.U24 * mag).all(), "the folded residual stream"
    _ln_check(xr.cpu(), g, b, y.cpu(), dtype, f"layernorm_reduce {rows}x{C} {dtype}")


def _ln_check(x, g, b, y, dtype, what):
    """LayerNorm of fp32 rows x against float64: fp32 mean / variance over C and one output rounding."""
    x64, g64, b64 = x.double(), g.double(), b.double()
    C = x.shape[1]
    mu = x64.mean(1, keepdim=True)
    sd = (x64.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    xh = (x64 - mu) / sd
    ref = (xh * g64 + b64).numpy()
    bound = (X.ulp(ref, dtype) + 8 * math.sqrt(C) * X.U24 * ((xh.abs() + 1 + mu.abs() / sd) * g64.abs()).numpy()
             + 4 * X.U24 * np.abs(ref))
    return X.assert_close(y.double().numpy(), ref, bound, dtype, FLOOR[dtype], what)


# layernorm_launch picks one of three instantiations by C / 4 (<= 128, <= 320, else 16 vectors per lane): the 5-row shapes reach all three,
# the smallest and the largest C the launcher takes, and widths either side of each threshold
LN_SHAPES = [(rows, C) for rows in (8192, 300) for C in (64, 256, 320, 1024, 1280)] + [(5, C) for C in (4, 512, 516, 1280, 1284, 4096)]
LN_IDS = [f"{C}-{rows}" for rows, C in LN_SHAPES]


@pytest.mark.parametrize("rows,C", LN_SHAPES, ids=LN_IDS)
def test_layernorm_per_element(dev, rows, C):
    from msod_amd import ops
    x = _rnd(rows, C, seed=22) * 3 + 1
    g, b = _rnd(C, seed=23) * 0.2 + 1, _rnd(C, seed=24) * 0.1
    for dt in DTYPES:
        y = ops.layernorm(x.to(dev), g.to(dev), b.to(dev), dt)
        torch.cuda.synchronize()
        _ln_check(x, g, b, y.cpu(), dt, f"layernorm {rows}x{C} {dt}")


# ------------------------------------------------------------------------------ attention
def _qkv(B, heads, dk, dkp, dtype, seed, peaked):
    """[B*128, 3*heads*dkp] operands, padding columns zero; the second half of the heads gets large queries (peaked rows)."""
    q, k, v = (_rnd(B, heads, 128, dkp, seed=seed + i) for i in range(3))
    if peaked:
        q[:, heads // 2:] *= 6.0
    for t in (q, k, v):
        t[..., dk:] = 0
    q, k, v = (_q(t, dtype) for t in (q, k, v))
    flat = torch.cat([t.permute(0, 2, 1, 3).reshape(B * 128, heads * dkp) for t in (q, k, v)], 1)
    return q, k, v, flat


def _attn_out(out, B, heads, dkp):
    return out.float().cpu().view(B, 128, heads, dkp).permute(0, 2, 1, 3)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("dk", [8, 20, 32, 64, 128, 160])
def test_attention_per_element(dev, dtype, dk):
    """cft_attention on the benchmarked grid (64 images x 8 heads), flat and peaked softmax rows, against the float64 model of its
    documented numerics; the padding columns of the output are zero."""
    from msod_amd import ops
    B, heads = 64, 8
    step = 16 if dtype == torch.float32 else 32
    dkp = -(-dk // step) * step
    q, k, v, flat = _qkv(B, heads, dk, dkp, dtype, 100 + dk, True)
    out = ops.attention(flat.to(dev).to(dtype), B, heads, dk, dkp)
    torch.cuda.synchronize()
    got = _attn_out(out, B, heads, dkp)
    ref, bound = X.attention_ref(q, k, v, dk, dtype)
    X.assert_close(got[..., :dk].double().numpy(), ref[..., :dk], bound[..., :dk], dtype, FLOOR[dtype], f"attention dk{dk} {dtype}")
    assert float(got[..., dk:].abs().max() if dkp > dk else 0.0) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout_mask_and_values(dev, dtype, p):
    """Mask: with Q = 0 (every score equal) and V = identity the output's zero pattern IS the keep mask, which must equal the host
    replica of cft_hash32 at index ((b*heads + h)*128 + q)*128 + k exactly.  Values: random operands against the host-masked
    float64 model, held to the same per-element bound."""
    from msod_amd import ops
    B, heads, dk = 64, 8, 128           # the benchmarked grid: hash indices up to 64 * 8 * 128 * 128
    ops.manual_dropout_seed(4242)
    seed = ops.next_dropout_seed()
    keep = X.attention_mask(seed, B, heads, p)
    eye = torch.eye(128).expand(B, heads, 128, 128)
    zero = torch.zeros(B, heads, 128, dk)
    flat = torch.cat([t.permute(0, 2, 1, 3).reshape(B * 128, heads * dk) for t in (zero, _rnd(B, heads, 128, dk, seed=3), eye)], 1)
    ops.manual_dropout_seed(4242)
    out = ops.attention(flat.to(dev).to(dtype), B, heads, dk, dk, pdrop=p)
    torch.cuda.synchronize()
    got = _attn_out(out, B, heads, dk).numpy()
    assert np.array_equal(got != 0, keep), f"mask mismatch at {int((( got != 0) != keep).sum())} of {keep.size} positions"
    q, k, v, flat = _qkv(B, heads, 64, 64, dtype, 200, True)
    ops.manual_dropout_seed(4242)
    out = ops.attention(flat.to(dev).to(dtype), B, heads, 64, 64, pdrop=p)
    torch.cuda.synchronize()
    ref, bound = X.attention_ref(q, k, v, 64, dtype, keep=keep, pdrop=p)
    X.assert_close(_attn_out(out, B, heads, 64).double().numpy(), ref, bound, dtype, FLOOR[dtype], f"attention drop{p} {dtype}")


# ------------------------------------------------------------------------------ dropout, add
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_bit_exact(dev, dtype, p):
    """cft_dropout = x * mask * fp32(1/(1-p)) rounded once, mask from the host replica at the flat element index; n is not a
    multiple of the grid stride (4096 workgroups x 256 threads granules)."""
    from msod_amd import ops
    ge = 4 if dtype == torch.float32 else 8
    n = ge * (2 * 4096 * 256 + 1234)
    x = _q(_rnd(n, seed=9), dtype)
    xd = x.to(dev).to(dtype)
    ops.manual_dropout_seed(77)
    seed = ops.next_dropout_seed()
    ops.manual_dropout_seed(77)
    ops.dropout_(xd, p)
    torch.cuda.synchronize()
    want = X.dropout_ref(x, seed, p, dtype)
    got = xd.double().cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} elements differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_add_and_add_rows_bit_exact(dev, dtype):
    from msod_amd import ops
    a, b = _q(_rnd(2, 48, 13, 17, seed=1), dtype), _q(_rnd(2, 48, 13, 17, seed=2, scale=0.01), dtype)
    buf = to_dev_nhwc(torch.cat([a, b], 1), dev, dtype)
    s = ops.add(buf[:, :48], buf[:, 48:])
    torch.cuda.synchronize()
    # the kernel's numerics: the fp32 sum, then one rounding to the dtype
    assert np.array_equal(s.double().cpu().numpy(), X.rne((a + b).double(), dtype))
    x, y = _q(_rnd(300, 320, seed=3), dtype), _q(_rnd(300, 320, seed=4, scale=0.003), dtype)
    wide = torch.zeros(300, 640)
    wide[:, :320] = x
    xd = wide.to(dev).to(dtype)
    ops.add_rows_(xd[:, :320], y.to(dev).to(dtype))
    torch.cuda.synchronize()
    assert np.array_equal(xd[:, :320].double().cpu().numpy(), X.rne((x + y).double(), dtype))
    assert float(xd[:, 320:].abs().max()) == 0.0


# ------------------------------------------------------------------------------ CFT tokeniser, de-tokeniser, Detect decode
TOKEN_MAPS = [((80, 80), 256), ((20, 20), 1024), ((12, 20), 64), ((5, 7), 64), ((40, 40), 1280)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("hw,C", TOKEN_MAPS, ids=[f"{h}x{w}c{c}" for (h, w), c in TOKEN_MAPS])
def test_gpt_tokenize_per_element(dev, dtype, hw, C):
    """Adaptive average pool to 8 x 8 (overlapping windows, maps smaller than 8 x 8) + pos_emb, fp32 tokens: each within the
    rounding of an fp32 sum over its window (n + 2 roundings of the summed magnitudes)."""
    from msod_amd import ops
    H, W = hw
    B = 2
    rgb, ir = _q(_rnd(B, C, H, W, seed=19) + 0.5, dtype), _q(_rnd(B, C, H, W, seed=20), dtype)
    pe = _rnd(1, 128, C, seed=21, scale=0.3)
    tok = ops.gpt_tokenize(to_dev_nhwc(rgb, dev, dtype), to_dev_nhwc(ir, dev, dtype), pe.to(dev))
    torch.cuda.synchronize()
    pool = lambda t: torch.nn.functional.adaptive_avg_pool2d(t.double(), (8, 8)).reshape(B, C, 64)
    ref = (torch.cat([pool(rgb), pool(ir)], 2).permute(0, 2, 1) + pe.double()).numpy()
    mag = torch.cat([pool(rgb.abs()), pool(ir.abs())], 2).permute(0, 2, 1).numpy()
    n = (-(-H // 8) + 1) * (-(-W // 8) + 1)                  # largest window
    bound = (n + 2) * X.U24 * mag + 2 * X.U24 * (np.abs(ref) + np.abs(pe.double().numpy()))
    X.assert_close(tok.double().cpu().numpy(), ref, bound, torch.float32, None, f"tokenize {hw} C{C} {dtype}")


def _upsample_case(dtype, hw, C, seed):
    H, W = hw
    B = 2
    base0, base1 = _q(_rnd(B, C, H, W, seed=seed), dtype), _q(_rnd(B, C, H, W, seed=seed + 1, scale=0.05), dtype)
    tok = _rnd(B, 128, C, seed=seed + 2)
    grids = tok.view(B, 2, 8, 8, C).permute(0, 1, 4, 2, 3)
    ups = [X.upsample_ref(grids[:, s_], H, W) for s_ in (0, 1)]
    return B, H, W, base0, base1, tok, ups


def _upsample_bound(ref, base_mag, up_mag, taps, dtype, roundings=8):
    """fp32 blend in y then x plus the base: a few fp32 roundings of the magnitudes; the source coordinates (y + 0.5) * fp32(8 / H) - 0.5
    carry up to ~16 2^-24 per axis, which moves the blend by that times the tap difference (<= 2 x the largest tap); one output rounding."""
    return (X.ulp(ref, dtype) + roundings * X.U24 * (base_mag + up_mag) + 64 * X.U24 * taps
            + (2 * X.U24 * np.abs(ref) if dtype == torch.float32 else 0.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("hw,C", TOKEN_MAPS, ids=[f"{h}x{w}c{c}" for (h, w), c in TOKEN_MAPS])
def test_gpt_upsample_add_per_element(dev, dtype, hw, C):
    """Bilinear 8 x 8 -> H x W (align_corners=False) of one token stream + the base, one rounding; stream 1 rides on a small
    base (its outputs are low-magnitude where the tokens are), and without a base."""
    from msod_amd import ops
    B, H, W, base0, base1, tok, ups = _upsample_case(dtype, hw, C, 30)
    td = tok.to(dev)
    for s_, base in ((0, base0), (1, base1), (0, None)):
        out = ops.gpt_upsample_add(td, s_, None if base is None else to_dev_nhwc(base, dev, dtype), H, W, dtype)
        torch.cuda.synchronize()
        up, upm, taps = ups[s_]
        bm = 0.0 if base is None else np.abs(base.double().numpy())
        ref = up + (0.0 if base is None else base.double().numpy())
        X.assert_close(out.double().cpu().numpy(), ref, _upsample_bound(ref, bm, upm, taps, dtype), dtype, FLOOR[dtype],
                       f"upsample_add s{s_} base={base is not None} {hw} C{C} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("hw,C", TOKEN_MAPS, ids=[f"{h}x{w}c{c}" for (h, w), c in TOKEN_MAPS])
def test_gpt_upsample_add_dual_per_element(dev, dtype, hw, C):
    """cft_gpt_upsample_add2: both streams and their sum, each from the unrounded fp32 values with one rounding."""
    from msod_amd import ops
    B, H, W, base0, base1, tok, ups = _upsample_case(dtype, hw, C, 40)
    o0, o1, osum = ops.gpt_upsample_add_dual(tok.to(dev), to_dev_nhwc(base0, dev, dtype), to_dev_nhwc(base1, dev, dtype), H, W, dtype)
    torch.cuda.synchronize()
    b0, b1 = base0.double().numpy(), base1.double().numpy()
    r0, r1 = ups[0][0] + b0, ups[1][0] + b1
    m0, m1 = np.abs(b0) + ups[0][1], np.abs(b1) + ups[1][1]
    t0, t1 = ups[0][2], ups[1][2]
    for name, got, ref, mag, taps in (("out0", o0, r0, m0, t0), ("out1", o1, r1, m1, t1), ("sum", osum, r0 + r1, m0 + m1, t0 + t1)):
        X.assert_close(got.double().cpu().numpy(), ref, _upsample_bound(ref, mag, 0.0, taps, dtype, 9), dtype, FLOOR[dtype],
                       f"upsample_add2 {name} {hw} C{C} {dtype}")


DECODE_CASE = dict(B=2, ny=20, nx=24, na=3, no=85, stride=16.0, row0=100, tail=50)


def decode_operands():
    """Seeded operands of the Detect-decode case (shared with tests/test_gpu_memory_hygiene.py): logits [B, ldl, ny, nx] over [-12, 12]
    with one padding channel, anchors in pixels."""
    c = DECODE_CASE
    logits = _rnd(c["B"], c["na"] * c["no"] + 1, c["ny"], c["nx"], seed=27, scale=4.0).clamp(-12.0, 12.0)     # ldl = 256: one padding channel
    return logits, torch.tensor([10., 13., 16., 30., 33., 23.])


def decode_check(logits, anchors, raw, pred, before=None):
    """raw is a copy; xy = (2 s - 0.5 + grid) * stride, wh = (2 s)^2 * anchor, the rest s = sigmoid, each within __expf's error carried
    through the formula plus a few fp32 roundings; rows outside the slice keep what they held (``before``; None: zero)."""
    c = DECODE_CASE
    B, ny, nx, na, no, stride, row0 = (c[k] for k in ("B", "ny", "nx", "na", "no", "stride", "row0"))
    y = logits[:, :na * no].reshape(B, na, no, ny, nx).permute(0, 1, 3, 4, 2).double()
    assert torch.equal(raw.cpu(), y.float())
    sg = torch.sigmoid(y)
    gy, gx = torch.meshgrid(torch.arange(ny, dtype=torch.float64), torch.arange(nx, dtype=torch.float64), indexing="ij")
    ref = sg.clone()
    ref[..., 0] = (sg[..., 0] * 2 - 0.5 + gx) * stride
    ref[..., 1] = (sg[..., 1] * 2 - 0.5 + gy) * stride
    anc = anchors.double().view(1, na, 1, 1, 2)
    ref[..., 2:4] = (sg[..., 2:4] * 2) ** 2 * anc
    # sigmoid = rcp(1 + __expf(-v)): __expf relative error <= 2^-21 + |v| 2^-24 (argument rounding), scaled by s (1 - s); + rcp, add
    dsg = sg * (1 - sg) * (2.0 ** -21 + X.U24 * y.abs()) + 4 * X.U24 * sg
    slope = torch.ones_like(sg)
    slope[..., 0:2] = 2 * stride
    slope[..., 2:4] = 8 * sg[..., 2:4] * anc
    bound = (slope * dsg + 4 * X.U24 * ref.abs()).numpy()
    got = pred.cpu()
    n = na * ny * nx
    X.assert_close(got[:, row0:row0 + n].double().numpy(), ref.reshape(B, -1, no).numpy(), bound.reshape(B, -1, no),
                   torch.float32, None, "detect_decode")
    if before is None:
        assert float(got[:, :row0].abs().max()) == 0.0 and float(got[:, row0 + n:].abs().max()) == 0.0
    else:
        assert torch.equal(got[:, :row0], before[:, :row0]) and torch.equal(got[:, row0 + n:], before[:, row0 + n:])


def test_detect_decode_per_element(dev):
    """YOLO decode of fp32 logits (85 outputs per anchor, logits over [-12, 12]) into a slice of the prediction rows: raw is a
    copy; xy = (2 s - 0.5 + grid) * stride, wh = (2 s)^2 * anchor, the rest s = sigmoid, each within __expf's error carried
    through the formula plus a few fp32 roundings; rows outside the slice stay zero."""
    from msod_amd import ops
    c = DECODE_CASE
    logits, anchors = decode_operands()
    d = to_dev_nhwc(logits, dev, torch.float32)
    raw = torch.empty(c["B"], c["na"], c["ny"], c["nx"], c["no"], device=dev)
    rows = c["row0"] + c["na"] * c["ny"] * c["nx"] + c["tail"]
    pred = torch.zeros(c["B"], rows, c["no"], device=dev)
    ops.detect_decode(d, raw, pred, anchors.to(dev), c["na"], c["no"], c["stride"], c["row0"])
    torch.cuda.synchronize()
    decode_check(logits, anchors, raw, pred)


# ------------------------------------------------------------------------------ BatchNorm (training mode)
BN_CASES = [
    # M, C, act, residual dtype (None / "out" / "f32"), out dtype, momentum
    (1, 8, 1, None, torch.float32, 0.03),
    (4095, 20, 0, "out", torch.bfloat16, 0.03),
    (4097, 64, 1, "f32", torch.float16, None),
    (4097, 1024, 0, None, torch.float32, None),
    (4095, 4096, 1, "out", torch.bfloat16, 0.03),
    (64 * 80 * 80, 64, 1, "out", torch.float16, 0.03),
    (64 * 80 * 80, 20, 0, "f32", torch.float32, None),
    (64 * 80 * 80, 8, 0, None, torch.bfloat16, 0.03),
]


def bn_operands(case):
    """Seeded operands of one BN_CASES entry (shared with tests/test_gpu_memory_hygiene.py): x [M, pad8(C)] fp32 (channel 0 at |mean| =
    1e4 sigma; channel 1's row 0 1e3 sigma from its mean), gamma, beta, the running statistics before the call, the shortcut or None
    and its dtype."""
    M, C, act, rkind, odt, mom = case
    Cp = -(-C // 8) * 8
    gen = torch.Generator().manual_seed(M + C)
    mean_c = torch.randn(C, generator=gen) * 2
    sig_c = torch.rand(C, generator=gen) + 0.2
    x = torch.zeros(M, Cp)
    x[:, :C] = torch.randn(M, C, generator=gen) * sig_c + mean_c
    x[:, 0] = torch.randn(M, generator=gen) * 0.5 + 5000.0
    if C > 1 and M > 1:
        x[0, 1] = mean_c[1] + 1000.0 * sig_c[1]
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    rdt = odt if rkind == "out" else torch.float32
    res = _q(_rnd(M, C, seed=5), rdt) if rkind else None
    return dict(x=x, Cp=Cp, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, res=res, rdt=rdt)


def bn_check(case, o, got, rm, rv, m, eps=1e-5):
    """The output [M, C] per element, running mean and unbiased running variance (momentum ``m``) against float64 batch statistics."""
    M, C, act, rkind, odt, mom = case
    x, res = o["x"], o["res"]
    gamma, beta, rm0, rv0 = o["gamma"].double(), o["beta"].double(), o["rm0"].double(), o["rv0"].double()
    x64 = x[:, :C].double()
    mu = x64.mean(0)
    var = x64.var(0, unbiased=False)
    sc = gamma / (var + eps).sqrt()
    sh = beta - mu * sc
    v = (x64 * sc + sh).numpy()
    ref = X.act64(v, act) + (res.double().numpy() if rkind else 0.0)
    # the kernel's affine form x * sc + sh in fp32 (sc, sh rounded to fp32: |x sc| + |sh| carries their rounding); a relative error
    # of the statistics (and of sc) moves v - beta = (x - mean) * sc: held to 4e-6 (the parent's single-row pivot: up to 5e-3)
    bound = (X.ulp(ref, odt) + 1.1 * (4 * X.U24 * (np.abs((x64 * sc).numpy()) + np.abs(sh.numpy())) + 4e-6 * np.abs(v - beta.numpy()))
             + X.act_err(v, act) + 4 * X.U24 * np.abs(ref))
    got = got.double().cpu().numpy()
    # channel 0 (|mean| = 1e4 sigma) loses the last bits to the fp32 affine form, so the rounding-rate floor applies to the others
    X.assert_close(got[:, :1], ref[:, :1], bound[:, :1], odt, None, f"bn {case} ch0")
    X.assert_close(got[:, 1:], ref[:, 1:], bound[:, 1:], odt, FLOOR[odt] if M * C >= 4096 else None, f"bn {case}")
    unb = var * M / (M - 1) if M > 1 else var
    rm_ref, rv_ref = (1 - m) * rm0 + m * mu, (1 - m) * rv0 + m * unb
    rm, rv = rm.double().cpu(), rv.double().cpu()
    var_rel = ((rv - rv_ref).abs() / rv_ref).max().item()
    print(f"[oracle] bn {case}: running_var max rel err {var_rel:.3e}")
    assert ((rm - rm_ref).abs() <= 8 * X.U24 * (rm0.abs() + mu.abs()) + 1e-6 * var.sqrt()).all()
    assert var_rel <= 1e-5, f"running_var relative error {var_rel:.3e}"


@pytest.mark.parametrize("case", BN_CASES, ids=[f"bn{i}" for i in range(len(BN_CASES))])
def test_batchnorm_train_per_element(dev, case):
    """cft_batchnorm_train against float64 batch statistics: the output per element, running mean and unbiased running variance
    (M/(M-1); M = 1 keeps the biased 0).  Channel 0 sits at |mean| = 1e4 sigma; channel 1's row 0 lies 1e3 sigma from its mean."""
    from msod_amd import ops
    M, C, act, rkind, odt, mom = case
    o = bn_operands(case)
    x, Cp, res, rdt = o["x"], o["Cp"], o["res"], o["rdt"]
    bn = torch.nn.BatchNorm2d(C, momentum=mom).to(dev)
    with torch.no_grad():
        bn.weight.copy_(o["gamma"])
        bn.bias.copy_(o["beta"])
        bn.running_mean.copy_(o["rm0"])
        bn.running_var.copy_(o["rv0"])
        bn.num_batches_tracked.fill_(3)
    y32 = x.to(dev).view(M, 1, 1, Cp).permute(0, 3, 1, 2)
    rd = None
    if rkind:       # a channel slice of a granule-wide buffer, like the output
        rbuf = torch.zeros(M, Cp, dtype=rdt, device=dev)
        rbuf[:, :C] = res.to(dev).to(rdt)
        rd = rbuf.view(M, 1, 1, Cp).permute(0, 3, 1, 2)[:, :C]
    out = ops.batchnorm_train(y32, C, bn, act, residual=rd, out_dtype=odt)
    torch.cuda.synchronize()
    bn_check(case, o, out.permute(0, 2, 3, 1).reshape(M, C), bn.running_mean, bn.running_var, mom if mom is not None else 1.0 / 4, bn.eps)
    assert int(bn.num_batches_tracked) == 4


def test_batchnorm_train_without_running_stats(dev):
    """track_running_stats=False: batch statistics only, nothing to update."""
    from msod_amd import ops
    M, C = 4097, 24
    x = _rnd(M, C, seed=11) * 3 + 1
    bn = torch.nn.BatchNorm2d(C, track_running_stats=False).to(dev)
    out = ops.batchnorm_train(x.to(dev).view(M, 1, 1, C).permute(0, 3, 1, 2), C, bn, 0)
    torch.cuda.synchronize()
    x64 = x.double()
    ref = ((x64 - x64.mean(0)) / (x64.var(0, unbiased=False) + bn.eps).sqrt()).numpy()
    bound = 8 * X.U24 * (np.abs(ref) + np.abs(x64.numpy()) * 2) + 1e-6 * np.abs(ref)
    X.assert_close(out.permute(0, 2, 3, 1).reshape(M, C).double().cpu().numpy(), ref, bound, torch.float32, None, "bn no running stats")


# ------------------------------------------------------------------------------ GELU tail
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.bfloat16], ids=["f16", "f32", "bf16"])
def test_gelu_tail_through_an_identity_linear(dev, dtype):
    """Pre-activations swept over [-9, 9] through a linear layer with the identity as weight (one exact product per output, so no
    accumulation error): the GELU epilogue within the documented absolute bound 0.5 |v| 1.5e-7 + a few fp32 ulps (+ the output
    rounding).  Measured relative error in the negative tail is printed."""
    from msod_amd import ops
    C = 64
    v = torch.linspace(-9.0, 9.0, 64 * 1024)
    v = _q(v, dtype)
    x = v.view(-1, C)
    pk = ops.pack_conv(torch.eye(C), torch.zeros(C), dtype, device=dev)
    y = ops.linear(x.to(dev).to(dtype), pk, ops.ACT_GELU)
    torch.cuda.synchronize()
    v64 = x.double().numpy()
    ref = X.act64(v64, 2)
    got = y[:, :C].double().cpu().numpy()
    bound = X.ulp(ref, dtype) + X.act_err(v64, 2) + (2 * X.U24 * np.abs(ref) if dtype == torch.float32 else 0.0)
    X.assert_close(got, ref, bound, dtype, None, f"gelu tail {dtype}")
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print(f"[oracle] gelu tail {dtype}: max rel err " + ", ".join(
        f"v in [{t - 1}, {t}): {rel[(v64 >= t - 1) & (v64 < t)].max():.2e}" for t in (-2, -3, -4, -5, -6, -8)))
