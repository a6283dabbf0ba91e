"""Memory-hygiene sweep: no kernel reads or writes outside its tensors.

Every case builds seeded CPU operands, declares each device tensor to the harness of tests/guarded.py as an input, an output, an
in/out operand or a workspace, and calls the C ABI through ``_lib.load()`` so that every buffer is guarded.  The harness runs the
case under the three fill bytes and requires CFT_OK, intact bands, unchanged inputs and bit-identical outputs; on the 0x00 run the
result is also held to the kernel's existing reference, so nothing passes by being consistently wrong.

Output masks (``defined=``): one.  cft_anchor_kmeans' ``book`` is compared on its first info[0] rows only (include/cft_hip.h:
"book [k, 2] float64: the winning code book, its first info[0] rows").  Every other output of every swept entry point is compared in
full - also the detection slots past ``counts``, which the header documents as zeroed (cft_nms: "first counts[b] rows valid, the
others zeroed"; cft_eval_export, cft_detect_boxes: "Slots r >= counts[b] are zero").

The second half poisons the allocations a caller cannot reach (``torch.empty`` and friends inside the package) and runs whole
workloads under the three fills.  Captured-graph replays are out of scope: a fill issued during capture would become part of the
graph, so every workload here runs eagerly, with capture off.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import exact_ref as X
import guarded as G
from test_gpu_ops import TILE_VARIANTS

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
LOWP = [BF16, F16]
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}

DEV = None          # the ``dev`` fixture's device, set by test_sweep: where a check runs a reference launch of the package
CASES = []          # (id, entry points, builder): builder() -> (case(run), check(outputs of the 0x00 run) or None)


def sweep(entry_points, ident):
    def deco(fn):
        CASES.append((ident, tuple(entry_points.split()), fn))
        return fn
    return deco


def swept_entry_points():
    """Every entry point some case of the table launches (tests/test_guarded_host.py locks this against the header)."""
    return sorted({e for _, eps, _ in CASES for e in eps})


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _q(x, dtype):
    return x if dtype == F32 else x.to(dtype).float()


def _lib():
    from msod_amd import _lib as L
    return L.load()


def _dt(dtype):
    from msod_amd import ops
    return ops._dt(dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack(w, b, dtype, s=1):
    """The packed weights on the HOST: they become guarded inputs like every other operand."""
    from msod_amd import ops
    return ops.pack_conv(w, b, dtype, s=s, device="cpu")


def _p(t):
    return None if t is None else t.data_ptr()


def _base(t, off):
    """Pointer to channel 0 of the buffer a channel slice at ``off`` lives in (for the entry points' own xoff / yoff arguments)."""
    return t.data_ptr() - off * t.element_size()


def _poison(shape, dtype, fill):
    """A CPU tensor whose every byte is the fill byte: the prior content of the part of an in/out buffer that the kernel writes."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), fill, dtype=torch.uint8).view(dtype).view(shape)


def _out_size(H, W, k, s):
    p = k // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------ cft_conv2d / linear
CONV_SHAPES = [
    # B, H, W, Cin, Cout, k, s
    (2, 33, 31, 64, 320, 3, 1),     # ragged M, N tail, border taps
    (1, 9, 11, 80, 160, 3, 2),      # K = 720 inside Kpad 768; taps straddle K steps
    (2, 10, 10, 16, 32, 3, 1),      # Cin below one K step
    (1, 8, 8, 512, 24, 1, 1),       # narrow N
    (2, 9, 9, 512, 40, 3, 2),       # chunk-major, stride 2
]
ASM_VARIANTS = [96, 961, 962, 963, 964]
GENERIC_WALK = 900


def _conv_builder(dtype, shape, variant=0, act=1, use_res=True, out_dtype=None, seed=1):
    B, H, W, Cin, Cout, k, s = shape
    out_dtype = out_dtype or dtype
    x = _q(_rnd(B, Cin, H, W, seed=seed), dtype)
    w = _q(_rnd(Cout, Cin, k, k, seed=seed + 1, scale=1.0 / math.sqrt(Cin * k * k)), dtype)
    b = _rnd(Cout, seed=seed + 2, scale=0.5)
    Ho, Wo = _out_size(H, W, k, s)
    pk = _pack(w, b, dtype, s)
    res = _q(_rnd(B, pk.n, Ho, Wo, seed=seed + 3), out_dtype) if use_res else None

    def case(run):
        lib = _lib()
        xd = run.inp("x", x.to(dtype), layout="nhwc")
        wd, bd = run.inp("w", pk.w), run.inp("bias", pk.bias)
        rd = run.inp("res", res.to(out_dtype), layout="nhwc") if use_res else None
        y = run.out("y", (B, pk.n, Ho, Wo), out_dtype, layout="nhwc")
        lib.cft_set_conv_variant(variant)
        try:
            run.status(lib.cft_conv2d(_p(xd), _p(wd), _p(bd), _p(rd), _p(y), B, H, W, pk.cin, pk.cin, 0, pk.n, pk.kpad, k, s,
                                      pk.n, 0, pk.n, 0, act, _dt(dtype), _dt(out_dtype), _dt(out_dtype), _stream()), "cft_conv2d")
        finally:
            lib.cft_set_conv_variant(0)

    def check(out):
        v, absacc, rows = X.conv_ref(x, w, b, s)
        ref = X.act64(v, act)
        if use_res:
            ref = ref + X.nhwc_rows(res, rows, Cout)
        bound = X.gemm_bound(ref, absacc, k * k * Cin, out_dtype, act, v, fp32_roundings=3 if use_res else 2)
        X.assert_close(X.nhwc_rows(out["y"], rows, Cout), ref, bound, out_dtype, None, f"conv {shape} {dtype} v{variant}")
    return case, check


for _dtype in DTYPES:
    for _i, _shape in enumerate(CONV_SHAPES):
        for _v in (0, GENERIC_WALK):
            sweep("cft_conv2d", f"conv-s{_i}-{NAME[_dtype]}-v{_v}")(lambda d=_dtype, sh=_shape, v=_v: _conv_builder(d, sh, v))
    for _v in TILE_VARIANTS + (ASM_VARIANTS if _dtype != F32 else []):
        sweep("cft_conv2d", f"conv-s0-{NAME[_dtype]}-v{_v}")(lambda d=_dtype, v=_v: _conv_builder(d, CONV_SHAPES[0], v, seed=31))
for _dtype in LOWP:
    sweep("cft_conv2d", f"conv-f32out-{NAME[_dtype]}")(lambda d=_dtype: _conv_builder(d, (2, 11, 13, 64, 72, 3, 1), out_dtype=F32, seed=63))


def _conv_slices_builder(dtype, variant):
    """Input = channels [C, 2C) of a 2C buffer, output into channels [0, C) of another, the shortcut aliasing the output; the other
    half of each buffer holds the fill byte."""
    B, H, W, C = 2, 12, 12, 64
    x = _q(_rnd(B, C, H, W, seed=5), dtype)
    r = _q(_rnd(B, C, H, W, seed=8), dtype)
    w = _q(_rnd(C, C, 3, 3, seed=6, scale=1.0 / math.sqrt(C * 9)), dtype)
    b = _rnd(C, seed=7, scale=0.1)
    pk = _pack(w, b, dtype)

    def case(run):
        lib = _lib()
        xd = run.inp("x", x.to(dtype), layout="nhwc", ld=2 * C, off=C)
        wd, bd = run.inp("w", pk.w), run.inp("bias", pk.bias)
        y = run.inout("y", r.to(dtype), layout="nhwc", ld=2 * C, off=0)
        lib.cft_set_conv_variant(variant)
        try:
            run.status(lib.cft_conv2d(_base(xd, C), _p(wd), _p(bd), _p(y), _p(y), B, H, W, C, 2 * C, C, C, pk.kpad, 3, 1,
                                      2 * C, 0, 2 * C, 0, 1, _dt(dtype), _dt(dtype), _dt(dtype), _stream()), "cft_conv2d")
        finally:
            lib.cft_set_conv_variant(0)

    def check(out):
        v, absacc, rows = X.conv_ref(x, w, b, 1)
        ref = X.act64(v, 1) + X.nhwc_rows(r, rows, C)
        X.assert_close(X.nhwc_rows(out["y"], rows, C), ref, X.gemm_bound(ref, absacc, 9 * C, dtype, 1, v, 3), dtype, None, f"conv slices {dtype}")
    return case, check


def _linear_builder(dtype, variant, rows=300, K=256, N=320):
    """The linear form (B = 1, H = 1, W = rows, k = 1) with ld > K on the input and ld > N on the output, GELU."""
    x = _q(_rnd(rows, K, seed=K), dtype)
    w = _q(_rnd(N, K, seed=K + 1, scale=2.0 / math.sqrt(K)), dtype)
    b = _rnd(N, seed=K + 2, scale=0.3)
    pk = _pack(w, b, dtype)

    def case(run):
        lib = _lib()
        xd = run.inp("x", x.to(dtype), layout="rows", ld=K + 16, off=8)
        wd, bd = run.inp("w", pk.w), run.inp("bias", pk.bias)
        y = run.out("y", (rows, pk.n), dtype, layout="rows", ld=pk.n + 8, off=8)
        lib.cft_set_conv_variant(variant)
        try:
            run.status(lib.cft_conv2d(_p(xd), _p(wd), _p(bd), None, _p(y), 1, 1, rows, pk.cin, K + 16, 0, pk.n, pk.kpad, 1, 1,
                                      pk.n + 8, 0, 0, 0, 2, _dt(dtype), _dt(dtype), _dt(dtype), _stream()), "cft_conv2d")
        finally:
            lib.cft_set_conv_variant(0)

    def check(out):
        xs = x.double()
        v = (xs @ w.double().T + b.double()).numpy()
        absacc = (xs.abs() @ w.double().abs().T + b.double().abs()).numpy()
        ref = X.act64(v, 2)
        X.assert_close(out["y"][:, :N].double().numpy(), ref, X.gemm_bound(ref, absacc, K, dtype, 2, v), dtype, None, f"linear {dtype}")
    return case, check


for _dtype in DTYPES:
    for _v in (0, GENERIC_WALK) + ((96,) if _dtype != F32 else ()):
        sweep("cft_conv2d", f"conv-slices-{NAME[_dtype]}-v{_v}")(lambda d=_dtype, v=_v: _conv_slices_builder(d, v))
        sweep("cft_conv2d", f"linear300-{NAME[_dtype]}-v{_v}")(lambda d=_dtype, v=_v: _linear_builder(d, v))


# ------------------------------------------------------------------------------ cft_conv2d_chain, cft_conv2d_chain_res
def _two_convs_ref(dev, dtype, x, pk1, pk2, act2, res=None):
    """The chained kernels are bit-identical to the separate cft_conv2d launches: that is their reference."""
    from msod_amd import ops
    from helpers import to_dev_nhwc
    move = lambda pk: type(pk)(pk.w.to(dev), pk.bias.to(dev), pk.n, pk.n_valid, pk.cin, pk.kpad, pk.k, pk.s, pk.flops_per_row)
    a, b = move(pk1), move(pk2)
    y1 = ops.conv2d(to_dev_nhwc(x, dev, dtype), a, ops.ACT_SILU, residual=None if res is None else to_dev_nhwc(res, dev, dtype))
    y2 = ops.conv2d(y1, b, act2)
    torch.cuda.synchronize()
    return y1.cpu(), y2.cpu()


def _chain_builder(dtype, B, H, W, cin, k, s, n1, n2):
    x = _q(_rnd(B, cin, H, W, seed=31), dtype)
    pk1 = _pack(_rnd(n1, cin, k, k, seed=32) * (2.0 / (cin * k * k)) ** 0.5, _rnd(n1, seed=33) * 0.1, dtype, s)
    pk2 = _pack(_rnd(n2, n1, 1, 1, seed=34) * (2.0 / n1) ** 0.5, _rnd(n2, seed=35) * 0.1, dtype)
    Ho, Wo = _out_size(H, W, k, s)
    ldy = pk2.n + 16

    def case(run):
        lib = _lib()
        xd = run.inp("x", x.to(dtype), layout="nhwc")
        w1, b1, w2, b2 = run.inp("w1", pk1.w), run.inp("b1", pk1.bias), run.inp("w2", pk2.w), run.inp("b2", pk2.bias)
        y = run.out("y", (B, pk2.n, Ho, Wo), dtype, layout="nhwc", ld=ldy, off=8)
        assert lib.cft_conv2d_chain_ok(B, H, W, cin, cin, n1, pk1.kpad, k, s, pk2.n, ldy, _dt(dtype)) == 1
        run.status(lib.cft_conv2d_chain(_p(xd), _p(w1), _p(b1), _p(w2), _p(b2), _base(y, 8), B, H, W, cin, cin, 0, n1, pk1.kpad, k, s,
                                        pk2.n, ldy, 8, 1, _dt(dtype), _stream()), "cft_conv2d_chain")

    def check(out):
        _, y2 = _two_convs_ref(DEV, dtype, x, pk1, pk2, 1)
        assert torch.equal(out["y"], y2)
    return case, check


def _chain_res_builder(dtype, B, H, W, k, n2):
    cin = 256
    x = _q(_rnd(B, cin, H, W, seed=41), dtype)
    res = _q(_rnd(B, 256, H, W, seed=42), dtype)
    pk1 = _pack(_rnd(256, cin, k, k, seed=43) * (2.0 / (cin * k * k)) ** 0.5, _rnd(256, seed=44) * 0.1, dtype)
    pk2 = _pack(_rnd(n2, 256, 1, 1, seed=45) * (2.0 / 256) ** 0.5, _rnd(n2, seed=46) * 0.1, dtype)

    def case(run):
        lib = _lib()
        xd = run.inp("x", x.to(dtype), layout="nhwc")
        rd = run.inp("res", res.to(dtype), layout="nhwc")
        w1, b1, w2, b2 = run.inp("w1", pk1.w), run.inp("b1", pk1.bias), run.inp("w2", pk2.w), run.inp("b2", pk2.bias)
        y1 = run.out("y1", (B, 256, H, W), dtype, layout="nhwc", ld=272, off=8)
        y2 = run.out("y2", (B, pk2.n, H, W), dtype, layout="nhwc", ld=pk2.n + 8, off=0)
        run.status(lib.cft_conv2d_chain_res(_p(xd), _p(w1), _p(b1), _p(rd), _base(y1, 8), _p(w2), _p(b2), _p(y2), B, H, W, cin, cin, 0,
                                            256, pk1.kpad, k, 1, 256, 0, 272, 8, pk2.n, pk2.n + 8, 0, 1, _dt(dtype), _stream()),
                   "cft_conv2d_chain_res")

    def check(out):
        y1, y2 = _two_convs_ref(DEV, dtype, x, pk1, pk2, 1, res=res)
        assert torch.equal(out["y1"], y1) and torch.equal(out["y2"], y2)
    return case, check


for _dtype in LOWP:
    for _c in [(1, 51, 37, 64, 3, 2, 128, 128), (3, 40, 24, 128, 3, 1, 128, 64), (1, 45, 37, 128, 3, 2, 256, 256)]:
        sweep("cft_conv2d_chain", f"chain-{'x'.join(map(str, _c))}-{NAME[_dtype]}")(lambda d=_dtype, c=_c: _chain_builder(d, *c))
    sweep("cft_conv2d_chain_res", f"chainres-1x19x23-{NAME[_dtype]}")(lambda d=_dtype: _chain_res_builder(d, 1, 19, 23, 3, 256))


# ------------------------------------------------------------------------------ cft_bottleneck, cft_bottleneck_pack_w2
def _bottleneck_builder(dtype, C, hw, shortcut):
    H, W = hw
    B = 2
    w1 = _q(_rnd(C, C, 1, 1, seed=61, scale=1.2 / math.sqrt(C)), dtype)
    w2 = _q(_rnd(C, C, 3, 3, seed=63, scale=0.4 / math.sqrt(C)), dtype)
    pk1, pk2 = _pack(w1, _rnd(C, seed=62, scale=0.1), dtype), _pack(w2, _rnd(C, seed=64, scale=0.1), dtype)
    x = _q(_rnd(B, C, H, W, seed=65), dtype)

    def case(run):
        lib = _lib()
        xd = run.inp("x", x.to(dtype), layout="nhwc", ld=2 * C, off=C)
        w1d, b1d, w2d, b2d = run.inp("w1", pk1.w), run.inp("b1", pk1.bias), run.inp("w2", pk2.w), run.inp("b2", pk2.bias)
        stages = None
        if C == 128:
            stages = run.out("w2_stages", tuple(pk2.w.shape), dtype)
            run.status(lib.cft_bottleneck_pack_w2(_p(w2d), pk2.kpad, C, _p(stages), _dt(dtype), _stream()), "cft_bottleneck_pack_w2")
        y = run.out("y", (B, C, H, W), dtype, layout="nhwc", ld=C + 24, off=16)
        run.status(lib.cft_bottleneck(_base(xd, C), 2 * C, C, _p(w1d), pk1.kpad, _p(b1d), _p(w2d), pk2.kpad, _p(stages), _p(b2d),
                                      _base(y, 16), C + 24, 16, B, H, W, C, int(shortcut), _dt(dtype), _stream()), "cft_bottleneck")

    def check(out):
        from msod_amd import ops
        from helpers import to_dev_nhwc
        dev = DEV
        move = lambda pk: type(pk)(pk.w.to(dev), pk.bias.to(dev), pk.n, pk.n_valid, pk.cin, pk.kpad, pk.k, pk.s, pk.flops_per_row)
        xd = to_dev_nhwc(x, dev, dtype)
        two = ops.conv2d(ops.conv2d(xd, move(pk1), 1), move(pk2), 1, residual=xd if shortcut else None)
        torch.cuda.synchronize()
        assert torch.equal(out["y"], two.cpu())
    return case, check


for _dtype in LOWP:
    for _C in (64, 128):
        for _hw in ((17, 15), (8, 32)):
            for _sc in (True, False):
                sweep("cft_bottleneck" + (" cft_bottleneck_pack_w2" if _C == 128 else ""), f"bneck-c{_C}-{_hw[0]}x{_hw[1]}-sc{int(_sc)}-{NAME[_dtype]}")(
                    lambda d=_dtype, C=_C, hw=_hw, sc=_sc: _bottleneck_builder(d, C, hw, sc))


# ------------------------------------------------------------------------------ split-K linear + LayerNorm(+reduce)
def _ln_ref_check(x, g, b, y, dtype, what):
    from test_gpu_kernel_oracles import _ln_check
    _ln_check(x, g, b, y, dtype, what)


def _splitk_builder(dtype, rows, n, K, splits):
    x = _q(_rnd(rows, K, seed=71), dtype)
    w = _q(_rnd(n, K, seed=72, scale=1.0 / math.sqrt(K)), dtype)
    b = _rnd(n, seed=73, scale=0.1)
    pk = _pack(w, b, dtype)
    res = _rnd(rows, pk.n, seed=74)
    gamma, beta = 1.0 + 0.1 * _rnd(pk.n, seed=75), 0.1 * _rnd(pk.n, seed=76)

    def case(run):
        lib = _lib()
        xd = run.inp("x", x.to(dtype), layout="rows", ld=K + 8, off=0)
        wd, bd = run.inp("w", pk.w), run.inp("bias", pk.bias)
        parts = run.out("parts", (splits, rows, pk.n), F32)          # a workspace to the caller, an output of the first launch
        xr = run.inout("resid", res)
        gd, be = run.inp("gamma", gamma), run.inp("beta", beta)
        y = run.out("y", (rows, pk.n), dtype)
        run.status(lib.cft_linear_splitk(_p(xd), _p(wd), _p(bd), _p(parts), rows, pk.cin, K + 8, pk.n, pk.kpad, splits, _dt(dtype), _stream()),
                   "cft_linear_splitk")
        run.status(lib.cft_layernorm_reduce(_p(xr), _p(parts), splits, _p(gd), _p(be), _p(y), rows, pk.n, 1e-5, _dt(dtype), _stream()),
                   "cft_layernorm_reduce")

    def check(out):
        kc = K // splits
        for s_ in range(splits):
            xs, ws = x[:, s_ * kc:(s_ + 1) * kc].double(), w[:, s_ * kc:(s_ + 1) * kc].double()
            bb = b.double() if s_ == 0 else torch.zeros(n, dtype=torch.float64)
            ref = (xs @ ws.T + bb).numpy()
            absacc = (xs.abs() @ ws.abs().T + bb.abs()).numpy()
            X.assert_close(out["parts"][s_][:, :n].double().numpy(), ref, X.gemm_bound(ref, absacc, kc, F32), F32, None, f"splitk part {s_}")
        _ln_ref_check(out["resid"], gamma, beta, out["y"], dtype, f"layernorm_reduce {rows}x{pk.n} {dtype}")
    return case, check


def _layernorm_builder(out_dtype, rows, C):
    x = _rnd(rows, C, seed=22) * 3 + 1
    g, b = _rnd(C, seed=23) * 0.2 + 1, _rnd(C, seed=24) * 0.1

    def case(run):
        xd, gd, bd = run.inp("x", x), run.inp("gamma", g), run.inp("beta", b)
        y = run.out("y", (rows, C), out_dtype)
        run.status(_lib().cft_layernorm(_p(xd), _p(gd), _p(bd), _p(y), rows, C, 1e-5, _dt(out_dtype), _stream()), "cft_layernorm")
    return case, lambda out: _ln_ref_check(x, g, b, out["y"], out_dtype, f"layernorm {rows}x{C} {out_dtype}")


for _dtype in DTYPES:
    for _c in [(520, 256, 1024, 4), (256, 320, 1280, 4), (300, 320, 1280, 4)]:
        sweep("cft_linear_splitk cft_layernorm_reduce", f"splitk-{'x'.join(map(str, _c))}-{NAME[_dtype]}")(lambda d=_dtype, c=_c: _splitk_builder(d, *c))
    for _C in (64, 320, 1280):
        sweep("cft_layernorm", f"layernorm-300x{_C}-{NAME[_dtype]}")(lambda d=_dtype, C=_C: _layernorm_builder(d, 300, C))


# ------------------------------------------------------------------------------ attention
def _dkp(dk, dtype):
    step = 16 if dtype == F32 else 32
    return -(-dk // step) * step


def _attention_builder(dtype, dk, T=None, pdrop=0.0, rescale=False, seed=4242):
    """T None: cft_attention (128 tokens); otherwise cft_attention_tokens.  The pad columns [dk, dkp) of qkv are zero, as the header
    requires of the caller; the kernel must write the output's pad columns itself."""
    from test_gpu_cft_anchor_grid import _flat, _qkv, attention_mask, flash_ref
    tokens = T is not None
    T = T or 128
    B, heads = 2, 2
    dkp = _dkp(dk, dtype)
    q, k, v = _qkv(B, heads, T, dk, dkp, dtype, 300 + dk + T, peaked=not rescale)
    if rescale:         # the online-softmax rescale input of test_attention_tokens_rescale_branch
        k[:, :, 300, :dk] = q[:, :, 7, :dk] * (30.0 * math.sqrt(dk) / q[:, :, 7, :dk].pow(2).sum(-1, keepdim=True))
    q, k, v, flat = _flat(q, k, v, dtype)

    def case(run):
        lib = _lib()
        qkv = run.inp("qkv", flat.to(dtype))
        out = run.out("out", (B * T, heads * dkp), dtype)
        if tokens:
            run.status(lib.cft_attention_tokens(_p(qkv), _p(out), B, T, heads, dk, dkp, _dt(dtype), pdrop, seed, _stream()), "cft_attention_tokens")
        else:
            run.status(lib.cft_attention(_p(qkv), _p(out), B, heads, dk, dkp, _dt(dtype), pdrop, seed, _stream()), "cft_attention")

    def check(out):
        got = out["out"].float().view(B, T, heads, dkp).permute(0, 2, 1, 3)
        assert float(got[..., dk:].abs().max() if dkp > dk else 0.0) == 0.0
        keep = None
        if pdrop > 0.0:          # the host replica of the counter-based mask, as the existing dropout tests build it
            keep = attention_mask(seed, B, heads, T, pdrop) if tokens else X.attention_mask(seed, B, heads, pdrop)
        ref, bound = (flash_ref if tokens else X.attention_ref)(q, k, v, dk, dtype, keep=keep, pdrop=pdrop)
        X.assert_close(got[..., :dk].double().numpy(), ref[..., :dk], bound[..., :dk], dtype, None, f"attention T{T} dk{dk} p{pdrop} {dtype}")
    return case, check


for _dtype in DTYPES:
    for _dk in (8, 20, 160):
        sweep("cft_attention", f"attention-dk{_dk}-{NAME[_dtype]}")(lambda d=_dtype, dk=_dk: _attention_builder(d, dk))
    sweep("cft_attention", f"attention-dk20-drop-{NAME[_dtype]}")(lambda d=_dtype: _attention_builder(d, 20, pdrop=0.3))
    for _T in (1, 50, 130):
        for _pd in (0.0, 0.3):
            sweep("cft_attention_tokens", f"attention_tokens-T{_T}-p{_pd}-{NAME[_dtype]}")(lambda d=_dtype, T=_T, p=_pd: _attention_builder(d, 20, T, p))
    sweep("cft_attention_tokens", f"attention_tokens-rescale-{NAME[_dtype]}")(lambda d=_dtype: _attention_builder(d, 64, 512, rescale=True))


# ------------------------------------------------------------------------------ tokenise / upsample
def _tokenize_builder(dtype, hw, C, grid):
    H, W = hw
    B = 2
    va, ha = grid or (8, 8)
    T = 2 * va * ha
    rgb, ir = _q(_rnd(B, C, H, W, seed=19) + 0.5, dtype), _q(_rnd(B, C, H, W, seed=20), dtype)
    pe = _rnd(T, C, seed=21, scale=0.3)

    def case(run):
        lib = _lib()
        r = run.inp("rgb", rgb.to(dtype), layout="nhwc", ld=C + 16, off=8)
        i = run.inp("ir", ir.to(dtype), layout="nhwc", ld=2 * C, off=C)
        p = run.inp("pos_emb", pe)
        tok = run.out("tokens", (B, T, C), F32)
        if grid is None:
            run.status(lib.cft_gpt_tokenize(_p(r), C + 16, 0, _base(i, C), 2 * C, C, _p(p), _p(tok), B, H, W, C, _dt(dtype), _stream()), "cft_gpt_tokenize")
        else:
            run.status(lib.cft_gpt_tokenize_grid(_p(r), C + 16, 0, _base(i, C), 2 * C, C, _p(p), _p(tok), B, H, W, C, va, ha, _dt(dtype), _stream()),
                       "cft_gpt_tokenize_grid")

    def check(out):
        pool = lambda t: torch.nn.functional.adaptive_avg_pool2d(t.double(), (va, ha)).reshape(B, C, va * ha)
        ref = (torch.cat([pool(rgb), pool(ir)], 2).permute(0, 2, 1) + pe.double()).numpy()
        mag = torch.cat([pool(rgb.abs()), pool(ir.abs())], 2).permute(0, 2, 1).numpy()
        n = (-(-H // va) + 1) * (-(-W // ha) + 1)
        bound = (n + 2) * X.U24 * mag + 2 * X.U24 * (np.abs(ref) + np.abs(pe.double().numpy()))
        X.assert_close(out["tokens"].double().numpy(), ref, bound, F32, None, f"tokenize {hw} {grid} {dtype}")
    return case, check


def _upsample_builder(dtype, hw, C, grid, dual):
    """Bases and sum_out as channel slices; every output per element against the float64 bilinear under the existing bounds."""
    H, W = hw
    B = 2
    va, ha = grid or (8, 8)
    base0, base1 = _q(_rnd(B, C, H, W, seed=30), dtype), _q(_rnd(B, C, H, W, seed=31, scale=0.05), dtype)
    tok = _rnd(B, 2 * va * ha, C, seed=32)
    g = () if grid is None else (va, ha)
    sfx = "" if grid is None else "_grid"

    def case(run):
        lib = _lib()
        t = run.inp("tokens", tok)
        b0 = run.inp("base0", base0.to(dtype), layout="nhwc", ld=2 * C, off=C)
        b1 = run.inp("base1", base1.to(dtype), layout="nhwc", ld=C + 8, off=0)
        if dual:
            o0 = run.out("out0", (B, C, H, W), dtype, layout="nhwc")
            o1 = run.out("out1", (B, C, H, W), dtype, layout="nhwc", ld=C + 8, off=8)
            sm = run.out("sum", (B, C, H, W), dtype, layout="nhwc", ld=3 * C, off=C)
            run.status(getattr(lib, "cft_gpt_upsample_add2" + sfx)(_p(t), _base(b0, C), 2 * C, C, _p(b1), C + 8, 0, _p(o0), C, 0, _base(o1, 8), C + 8, 8,
                                                                   _base(sm, C), 3 * C, C, B, H, W, C, *g, _dt(dtype), _stream()), "cft_gpt_upsample_add2" + sfx)
        else:
            o0 = run.out("out0", (B, C, H, W), dtype, layout="nhwc", ld=C + 8, off=8)
            o1 = run.out("out1", (B, C, H, W), dtype, layout="nhwc")
            o2 = run.out("nobase", (B, C, H, W), dtype, layout="nhwc")
            fn = getattr(lib, "cft_gpt_upsample_add" + sfx)
            run.status(fn(_p(t), 0, _base(b0, C), 2 * C, C, _base(o0, 8), C + 8, 8, B, H, W, C, *g, _dt(dtype), _stream()), "cft_gpt_upsample_add" + sfx)
            run.status(fn(_p(t), 1, _p(b1), C + 8, 0, _p(o1), C, 0, B, H, W, C, *g, _dt(dtype), _stream()), "cft_gpt_upsample_add" + sfx)
            run.status(fn(_p(t), 0, None, 0, 0, _p(o2), C, 0, B, H, W, C, *g, _dt(dtype), _stream()), "cft_gpt_upsample_add" + sfx)

    def check(out):
        from test_gpu_cft_anchor_grid import _up_bound, _upsample_ref
        from test_gpu_kernel_oracles import FLOOR, _upsample_bound
        grids = tok.view(B, 2, va, ha, C).permute(0, 1, 4, 2, 3)
        b0, b1 = base0.double(), base1.double()
        if grid is None:          # the 8 x 8 kernels: X.upsample_ref and the bound of test_gpu_upsample_add(_dual)_per_element
            (u0, m0, t0), (u1, m1, t1) = (X.upsample_ref(grids[:, s_], H, W) for s_ in (0, 1))
            bnd = lambda ref, base_mag, up_mag, taps, r: _upsample_bound(ref, base_mag, up_mag, taps, dtype, r)        # noqa: E731
            r0, r1 = u0 + b0.numpy(), u1 + b1.numpy()
            a0, a1 = np.abs(b0.numpy()), np.abs(b1.numpy())
            if dual:
                exp = {"out0": (r0, bnd(r0, a0 + m0, 0.0, t0, 9)), "out1": (r1, bnd(r1, a1 + m1, 0.0, t1, 9)),
                       "sum": (r0 + r1, bnd(r0 + r1, a0 + m0 + a1 + m1, 0.0, t0 + t1, 9))}
            else:
                exp = {"out0": (r0, bnd(r0, a0, m0, t0, 8)), "out1": (r1, bnd(r1, a1, m1, t1, 8)), "nobase": (u0, bnd(u0, 0.0, m0, t0, 8))}
        else:                     # the grid kernels: the general-grid bilinear and the bound of test_upsample_grid_per_element
            (u0, m0, t0), (u1, m1, t1) = (_upsample_ref(grids[:, s_], H, W) for s_ in (0, 1))
            r0, r1 = u0 + b0, u1 + b1
            e0, e1 = (r0.numpy(), _up_bound(r0, m0 + b0.abs(), t0, dtype)), (r1.numpy(), _up_bound(r1, m1 + b1.abs(), t1, dtype))
            if dual:
                rs = r0 + r1
                exp = {"out0": e0, "out1": e1, "sum": (rs.numpy(), _up_bound(rs, m0 + m1 + b0.abs() + b1.abs(), torch.maximum(t0, t1) * 2, dtype, n_round=2))}
            else:
                exp = {"out0": e0, "out1": e1, "nobase": (u0.numpy(), _up_bound(u0, m0, t0, dtype))}
        for name, (ref, bound) in exp.items():
            X.assert_close(out[name].double().numpy(), ref, bound, dtype, FLOOR[dtype], f"upsample {name} {hw} {grid} {dtype}")
    return case, check


for _dtype in DTYPES:
    for _hw, _grid in (((5, 7), None), ((12, 20), None), ((12, 20), (13, 7)), ((5, 7), (13, 7))):
        _g = "8x8" if _grid is None else "13x7"
        _e = "" if _grid is None else "_grid"
        sweep("cft_gpt_tokenize" + _e, f"tokenize-{_hw[0]}x{_hw[1]}-g{_g}-{NAME[_dtype]}")(lambda d=_dtype, hw=_hw, g=_grid: _tokenize_builder(d, hw, 64, g))
        sweep("cft_gpt_upsample_add" + _e, f"upsample-{_hw[0]}x{_hw[1]}-g{_g}-{NAME[_dtype]}")(lambda d=_dtype, hw=_hw, g=_grid: _upsample_builder(d, hw, 64, g, False))
        sweep("cft_gpt_upsample_add2" + _e, f"upsample2-{_hw[0]}x{_hw[1]}-g{_g}-{NAME[_dtype]}")(lambda d=_dtype, hw=_hw, g=_grid: _upsample_builder(d, hw, 64, g, True))


# ------------------------------------------------------------------------------ Focus
def _focus_ref(img, dtype):
    """Space-to-depth of an fp32 NCHW image batch, rounded once: [B, 16, H/2, W/2], q = dy + 2 dx, channels 12.. zero."""
    B, _, H, W = img.shape
    out = torch.zeros(B, 16, H // 2, W // 2)
    for dx in (0, 1):
        for dy in (0, 1):
            qq = dy + 2 * dx
            out[:, qq * 3:qq * 3 + 3] = img[:, :, dy::2, dx::2]
    return out.to(dtype)


def _focus_s2d_builder(dtype, hw, u8):
    H, W = hw
    B = 2
    g = torch.Generator().manual_seed(12)
    if u8:
        six = torch.randint(0, 256, (B, 6, H, W), generator=g, dtype=torch.uint8)
    else:
        img = torch.rand(B, 3, H, W, generator=g)

    def case(run):
        lib = _lib()
        out = run.out("out", (B, 16, H // 2, W // 2), dtype, layout="nhwc")
        if u8:
            d = run.inp("img6", six)[:, 3:6]
            run.status(lib.cft_focus_s2d_u8(_p(d), d.stride(0), d.stride(1), d.stride(2), _p(out), B, H, W, 1.0 / 255.0, _dt(dtype), _stream()), "cft_focus_s2d_u8")
        else:
            d = run.inp("img", img)
            run.status(lib.cft_focus_s2d(_p(d), _p(out), B, H, W, _dt(dtype), _stream()), "cft_focus_s2d")

    def check(out):
        src = (six[:, 3:6].float() * np.float32(1.0 / 255.0)) if u8 else img
        assert torch.equal(out["out"], _focus_ref(src, dtype))
    return case, check


def _focus_conv_builder(dtype, hw, kind, n=48):
    H, W = hw
    B = 2
    g = torch.Generator().manual_seed(13)
    six = torch.randint(0, 256, (B, 6, H, W), generator=g, dtype=torch.uint8)
    img = torch.rand(B, 3, H, W, generator=g)
    w = _q(_rnd(n, 12, 3, 3, seed=14, scale=0.2), dtype)
    pk = _pack(w, _rnd(n, seed=15, scale=0.1), dtype)
    assert pk.cin == 16 and pk.kpad == 192

    def case(run):
        lib = _lib()
        wd, bd = run.inp("w", pk.w), run.inp("bias", pk.bias)
        y = run.out("y", (B, n, H // 2, W // 2), dtype, layout="nhwc", ld=n + 16, off=8)
        if kind == 1:
            d, scale = run.inp("img6", six)[:, 3:6], 1.0 / 255.0
        else:
            d, scale = run.inp("img", img), 1.0
        run.status(lib.cft_focus_conv(_p(d), kind, d.stride(0), d.stride(1), d.stride(2), scale, _p(wd), pk.kpad, _p(bd), _base(y, 8), n + 16, 8,
                                      B, H, W, n, 1, _dt(dtype), _stream()), "cft_focus_conv")

    def check(out):
        # the header's contract: bit-identical to cft_focus_s2d(_u8) followed by cft_conv2d
        from msod_amd import ops
        dev = DEV
        move = type(pk)(pk.w.to(dev), pk.bias.to(dev), pk.n, pk.n_valid, pk.cin, pk.kpad, pk.k, pk.s, pk.flops_per_row)
        src = six.to(dev)[:, 3:6] if kind == 1 else img.to(dev)
        two = ops.conv2d(ops.focus_s2d(src, dtype), move, 1)
        torch.cuda.synchronize()
        assert torch.equal(out["y"], two.cpu())
    return case, check


for _hw in ((32, 32), (40, 296)):
    for _dtype in DTYPES:
        sweep("cft_focus_s2d", f"focus_s2d-{_hw[0]}x{_hw[1]}-{NAME[_dtype]}")(lambda d=_dtype, hw=_hw: _focus_s2d_builder(d, hw, False))
        sweep("cft_focus_s2d_u8", f"focus_s2d_u8-{_hw[0]}x{_hw[1]}-{NAME[_dtype]}")(lambda d=_dtype, hw=_hw: _focus_s2d_builder(d, hw, True))
    for _dtype in LOWP:
        for _kind in (0, 1):
            sweep("cft_focus_conv", f"focus_conv-{_hw[0]}x{_hw[1]}-kind{_kind}-{NAME[_dtype]}")(lambda d=_dtype, hw=_hw, kd=_kind: _focus_conv_builder(d, hw, kd))


# ------------------------------------------------------------------------------ glue kernels
def _spp_builder(dtype):
    """In place in its 4C buffer: channels [0, C) are the input, the three pooled slices hold the fill byte before the launch."""
    B, C, H, W, ks = 2, 32, 7, 12, (5, 9, 13)
    x = _q(_rnd(B, C, H, W, seed=14), dtype)

    def case(run):
        buf = _poison((B, 4 * C, H, W), dtype, run.fill)
        buf[:, :C] = x.to(dtype)
        d = run.inout("buf", buf, layout="nhwc", ld=4 * C + 8, off=0)
        run.status(_lib().cft_spp_maxpool(_p(d), B, H, W, C, 4 * C + 8, *ks, _dt(dtype), _stream()), "cft_spp_maxpool")

    def check(out):
        assert torch.equal(out["buf"][:, :C].float(), x)
        for i, k in enumerate(ks):
            assert torch.equal(out["buf"][:, (i + 1) * C:(i + 2) * C].float(), torch.nn.functional.max_pool2d(x, k, 1, k // 2))
    return case, check


def _copy_builder(dtype):
    B, C, H, W = 2, 16, 6, 10
    a = _q(_rnd(B, C, H, W, seed=16), dtype)

    def case(run):
        src = run.inp("src", a.to(dtype), layout="nhwc", ld=2 * C, off=C)
        dst = run.out("dst", (B, C, 2 * H, 2 * W), dtype, layout="nhwc", ld=C + 8, off=8)
        run.status(_lib().cft_copy_channels(_base(src, C), 2 * C, C, _base(dst, 8), C + 8, 8, B, 2 * H, 2 * W, C, 1, _dt(dtype), _stream()), "cft_copy_channels")
    return case, lambda out: torch.testing.assert_close(out["dst"].float(), torch.nn.functional.interpolate(a, scale_factor=2, mode="nearest"), rtol=0, atol=0)


def _add_builder(dtype):
    B, C, H, W = 2, 48, 13, 17
    a, b = _q(_rnd(B, C, H, W, seed=1), dtype), _q(_rnd(B, C, H, W, seed=2, scale=0.01), dtype)

    def case(run):
        ad = run.inp("a", a.to(dtype), layout="nhwc", ld=2 * C, off=0)
        bd = run.inp("b", b.to(dtype), layout="nhwc", ld=2 * C, off=C)
        o = run.out("out", (B, C, H, W), dtype, layout="nhwc", ld=C + 8, off=0)
        run.status(_lib().cft_add(_p(ad), 2 * C, 0, _base(bd, C), 2 * C, C, _p(o), C + 8, 0, B * H * W, C, _dt(dtype), _stream()), "cft_add")
    return case, lambda out: np.testing.assert_array_equal(out["out"].double().numpy(), X.rne((a + b).double(), dtype))


def _to_nhwc_builder(dtype):
    """C = 3 -> 8 from a strided source: channels [1, 4) of a five-channel NCHW batch, every second column."""
    B, H, W = 2, 5, 7
    src = _rnd(B, 5, H, 2 * W, seed=3)

    def case(run):
        s = run.inp("src", src)[:, 1:4, :, ::2]
        o = run.out("out", (B, 8, H, W), dtype, layout="nhwc", ld=16, off=8)
        run.status(_lib().cft_to_nhwc(_p(s), _dt(F32), *s.stride(), _base(o, 8), 16, 8, B, 3, 8, H, W, _dt(dtype), _stream()), "cft_to_nhwc")

    def check(out):
        assert torch.equal(out["out"][:, :3], src[:, 1:4, :, ::2].to(dtype)) and float(out["out"][:, 3:].float().abs().max()) == 0.0
    return case, check


def _letterbox_builder():
    from msod_amd.utils.datasets import letterbox_geometry
    src_h, src_w, new = 30, 47, (64, 64)
    g = torch.Generator().manual_seed(4)
    src = torch.randint(0, 256, (src_h, src_w, 3), generator=g, dtype=torch.uint8)
    (rw, rh), _, _, (top, bottom, left, right) = letterbox_geometry((src_h, src_w), new, auto=False)
    assert (rh + top + bottom, rw + left + right) == new

    def case(run):
        s = run.inp("src", src)
        dst = run.out("dst", (3, new[0], new[1]), torch.uint8)
        run.status(_lib().cft_letterbox_u8(_p(s), src_h, src_w, src_w * 3, _p(dst), new[0], new[1], new[1], 1, new[0] * new[1], 1,
                                           rh, rw, top, left, 114, 114, 114, _stream()), "cft_letterbox_u8")

    def check(out):
        from test_letterbox import _oracle_letterbox
        want, _, _ = _oracle_letterbox(src.numpy(), new_shape=new, auto=False)
        assert torch.equal(out["dst"], torch.from_numpy(np.ascontiguousarray(want[:, :, ::-1].transpose(2, 0, 1))))
    return case, check


for _dtype in DTYPES:
    sweep("cft_spp_maxpool", f"spp-{NAME[_dtype]}")(lambda d=_dtype: _spp_builder(d))
    sweep("cft_copy_channels", f"copy_up2-{NAME[_dtype]}")(lambda d=_dtype: _copy_builder(d))
    sweep("cft_add", f"add-{NAME[_dtype]}")(lambda d=_dtype: _add_builder(d))
    sweep("cft_to_nhwc", f"to_nhwc-{NAME[_dtype]}")(lambda d=_dtype: _to_nhwc_builder(d))


# ------------------------------------------------------------------------------ Detect decode, NMS
def _decode_builder():
    """The case of test_detect_decode_per_element (row0 = 100 inside a wider pred), the rows around the slice holding seeded values."""
    from test_gpu_kernel_oracles import DECODE_CASE, decode_check, decode_operands
    c = DECODE_CASE
    B, ny, nx, na, no, stride, row0 = (c[k] for k in ("B", "ny", "nx", "na", "no", "stride", "row0"))
    logits, anchors = decode_operands()
    rows = row0 + na * ny * nx + c["tail"]
    before = _rnd(B, rows, no, seed=28)

    def case(run):
        lg = run.inp("logits", logits, layout="nhwc")
        an = run.inp("anchors", anchors)
        raw = run.out("raw", (B, na, ny, nx, no), F32)
        pred = run.inout("pred", before)
        run.status(_lib().cft_detect_decode(_p(lg), logits.shape[1], _p(raw), _p(pred), _p(an), B, ny, nx, na, no, stride, row0, rows, _stream()), "cft_detect_decode")
    return case, lambda out: decode_check(logits, anchors, out["raw"], out["pred"], before=before)


def _nms_builder(which):
    from oracle import nms_oracle
    from test_nms import _clustered_pred, _random_pred
    if which == "200":
        pred = torch.cat([_random_pred(200, 3, 11), _random_pred(200, 3, 12)])
    elif which == "2500":
        pred = _clustered_pred(125, 20)                              # 2500 candidates: the several-chunk path
    elif which == "ties":
        pred = _clustered_pred(250, 20, tie_scores=True)             # identical confidences overflowing a chunk
    else:
        pred = torch.zeros(2, 50, 8)                                 # no candidate at all
    B, rows, no = pred.shape
    max_det = 300
    sbytes = B * ((rows + 3) // 4 * 4) * 32

    def case(run):
        p = run.inp("pred", pred)
        scratch = run.work("scratch", (sbytes,))
        dets = run.out("dets", (B, max_det, 6), F32)
        counts = run.out("counts", (B,), torch.int32)
        run.status(_lib().cft_nms(_p(p), B, rows, no, 0.25, 0.45, 0, 0, None, max_det, 30000, _p(scratch), sbytes, _p(dets), _p(counts), _stream()), "cft_nms")

    def check(out):
        want = nms_oracle.non_max_suppression(pred, 0.25, 0.45)
        for b in range(B):
            n = int(out["counts"][b])
            assert n == want[b].shape[0] and torch.allclose(out["dets"][b, :n], want[b], rtol=0, atol=1e-4)
            assert float(out["dets"][b, n:].abs().max() if n < max_det else 0.0) == 0.0      # "the others zeroed" (include/cft_hip.h, cft_nms)
    return case, check


sweep("cft_detect_decode", "detect_decode-row0")(_decode_builder)
sweep("cft_letterbox_u8", "letterbox")(_letterbox_builder)
for _w in ("200", "2500", "ties", "empty"):
    sweep("cft_nms", f"nms-{_w}")(lambda w=_w: _nms_builder(w))


# ------------------------------------------------------------------------------ BatchNorm (training), dropout
def _bn_builder(case_):
    """Entries of BN_CASES (tests/test_gpu_kernel_oracles.py) with their operands and per-element check: the smallest (one row, eight
    channels) and the smallest with a real batch, (4095, 20): ragged rows, C below a granule multiple, a 16-bit shortcut.  The
    workspace is poisoned."""
    from test_gpu_kernel_oracles import bn_check, bn_operands
    M, C, act, rkind, odt, mom = case_
    o = bn_operands(case_)
    Cp, rdt = o["Cp"], o["rdt"]

    def case(run):
        lib = _lib()
        xd = run.inp("x", o["x"], layout="rows")
        gd, bd = run.inp("gamma", o["gamma"]), run.inp("beta", o["beta"])
        rm, rv = run.inout("running_mean", o["rm0"]), run.inout("running_var", o["rv0"])
        rd = run.inp("res", o["res"].to(rdt), layout="rows", ld=Cp, off=0) if rkind else None
        y = run.out("y", (M, C), odt, layout="rows", ld=Cp, off=0)
        nws = lib.cft_batchnorm_train_workspace(M, C)
        ws = run.work("workspace", (nws,))
        run.status(lib.cft_batchnorm_train(_p(xd), Cp, 0, M, C, _p(gd), _p(bd), _p(rm), _p(rv), mom, 1e-5, _p(rd), Cp, 0, _dt(rdt),
                                           _p(y), Cp, 0, act, _dt(odt), _p(ws), nws, _stream()), "cft_batchnorm_train")
    return case, lambda out: bn_check(case_, o, out["y"], out["running_mean"], out["running_var"], mom)


def _dropout_builder(dtype, n=None):
    ge = 4 if dtype == F32 else 8
    n = n or ge * 1234 + 3             # not a granule multiple; n = 3: less than one granule
    x = _q(_rnd(n, seed=9), dtype)
    seed, p = 0x1234567, 0.3

    def case(run):
        xd = run.inout("x", x.to(dtype))
        run.status(_lib().cft_dropout(_p(xd), n, p, seed, _dt(dtype), _stream()), "cft_dropout")
    return case, lambda out: np.testing.assert_array_equal(out["x"].double().numpy(), X.dropout_ref(x, seed, p, dtype))


def _bn_case(i):
    from test_gpu_kernel_oracles import BN_CASES
    return _bn_builder(BN_CASES[i])


sweep("cft_batchnorm_train", "batchnorm_train-1x8")(lambda: _bn_case(0))
sweep("cft_batchnorm_train", "batchnorm_train-4095x20")(lambda: _bn_case(1))
for _dtype in DTYPES:
    sweep("cft_dropout", f"dropout-{NAME[_dtype]}")(lambda d=_dtype: _dropout_builder(d))
    sweep("cft_dropout", f"dropout-n3-{NAME[_dtype]}")(lambda d=_dtype: _dropout_builder(d, 3))


# ------------------------------------------------------------------------------ evaluation: match, AP, curves, confusion, export
def _pinned(a):
    """A host tensor holding the bytes of a numpy array (what the entry points' host-side guards read)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())


def _eval_builder():
    """One small batch through the evaluator's five entry points, each feeding the next: B = 4 (one image without detections),
    max_det = 24, nc = 3.  label_hist, the confusion matrix and its flag are accumulated into: in/out operands starting at zero."""
    import confusion_ref
    import curves_ref
    import eval_ref
    from msod_amd.utils import metrics as M
    from test_gpu_eval import _random_batch
    B, max_det, nc, H, W = 4, 24, 3, 96, 128
    dets, counts, targets, shapes = _random_batch(np.random.default_rng(9), B, max_det, nc, H, W, "cpu")
    geom = M.geometry(shapes, (H, W))
    nt, niou, n = targets.shape[0], M.NIOU, B * max_det
    iouv = np.ascontiguousarray(M.IOUV.numpy(), dtype=np.float32)
    grid = np.logspace(-2.0, 0.0, 9)
    ng, npx = grid.size, len(M.PX)

    def case(run):
        lib = _lib()
        d, c, t, gm = run.inp("dets", dets), run.inp("counts", counts), run.inp("targets", targets), run.inp("geom", geom)
        nws = lib.cft_eval_match_workspace_bytes(B, nt)
        ws = run.work("match_ws", (nws,))
        correct = run.out("correct", (B, max_det, niou), torch.uint8)
        tp_bits, conf, pcls = run.out("tp_bits", (B, max_det), torch.int16), run.out("conf", (B, max_det), F32), run.out("pcls", (B, max_det), torch.int32)
        hist = run.inout("label_hist", torch.zeros(nc + 1, dtype=torch.int32))
        tcls, nl = run.out("tcls", (nt,), torch.int32), run.out("nl", (B,), torch.int32)
        run.status(lib.cft_eval_match(_p(d), _p(c), B, max_det, _p(t), nt, H, W, _p(gm), iouv.ctypes.data, niou, 0, _p(ws), nws, _p(correct),
                                      _p(tp_bits), _p(conf), _p(pcls), _p(hist), nc, _p(tcls), _p(nl), _stream()), "cft_eval_match")
        px, xg = run.inp("px", torch.from_numpy(M.PX.copy())), run.inp("xg", torch.from_numpy(M.XG.copy()))
        naws = lib.cft_eval_ap_workspace_bytes(n, nc)
        aws = run.work("ap_ws", (naws,))
        ap = run.out("ap", (nc * (4 + niou),), torch.float64)
        run.status(lib.cft_eval_ap(_p(tp_bits), _p(conf), _p(pcls), n, niou, _p(hist), nc, _p(px), _p(xg), _p(aws), naws, _p(ap), _stream()), "cft_eval_ap")
        nb = ctypes.c_long(0)
        assert lib.cft_eval_curves_workspace_bytes(n, nc, ctypes.byref(nb)) == 0
        cws = run.work("curves_ws", (nb.value,))
        gd = run.inp("fppi_grid", torch.from_numpy(grid.copy()))
        cur = [run.out(k, (nc, npx), torch.float64) for k in ("pcurve", "rcurve", "f1curve", "pycurve")]
        mr, best = run.out("mr", (nc, ng), torch.float64), run.out("best", (1,), torch.int32)
        run.status(lib.cft_eval_curves(_p(tp_bits), _p(conf), _p(pcls), n, _p(hist), nc, B, _p(px), _p(gd), grid.ctypes.data, ng, _p(cws), nb.value,
                                       *[_p(x) for x in cur], _p(mr), _p(best), _stream()), "cft_eval_curves")
        assert lib.cft_eval_confusion_workspace_bytes(B, nt, max_det, ctypes.byref(nb)) == 0
        fws = run.work("confusion_ws", (nb.value,))
        matrix = run.inout("matrix", torch.zeros((nc + 1) * (nc + 1), dtype=torch.int64))
        flag = run.inout("flag", torch.zeros(1, dtype=torch.int32))
        run.status(lib.cft_eval_confusion(_p(d), _p(c), B, max_det, _p(t), nt, H, W, _p(gm), 0.25, 0.45, 0, 0, nc, _p(fws), nb.value, _p(matrix),
                                          _p(flag), _stream()), "cft_eval_confusion")
        ex = run.out("export", (B, max_det, 16), F32)
        run.status(lib.cft_eval_export(_p(d), _p(c), B, max_det, _p(gm), 0, _p(ex), _stream()), "cft_eval_export")

    def check(out):
        t = targets.numpy()
        for b in range(B):
            nb_ = int(counts[b])
            corr, cf, pc, _ = eval_ref.match_image(dets[b, :nb_].numpy(), t[t[:, 0] == b, 1:], (H, W), shapes[b])
            assert np.array_equal(out["correct"][b, :nb_].numpy().astype(bool).reshape(corr.shape), corr)
            assert np.array_equal(out["conf"][b, :nb_].numpy(), cf) and np.array_equal(out["pcls"][b, :nb_].numpy(), pc)
            assert bool((out["pcls"][b, nb_:] == -1).all())
        assert np.array_equal(out["label_hist"][:nc].numpy(), np.bincount(t[:, 1].astype(np.int64), minlength=nc))
        # the statistics in insertion order (image-major, slot order), as test.py accumulates them
        valid = np.concatenate([np.arange(max_det) < int(counts[b]) for b in range(B)])
        tp = out["correct"].numpy().astype(bool).reshape(n, niou)[valid]
        cf, pc, tc = out["conf"].numpy().reshape(n)[valid], out["pcls"].numpy().reshape(n)[valid], t[:, 1].astype(np.float64)
        assert np.array_equal(out["tp_bits"].numpy().reshape(n)[valid].astype(np.int64) & ((1 << niou) - 1), (tp * (1 << np.arange(niou))).sum(1))
        classes = np.unique(tc).astype(np.int64)
        p, r, f1, ntp, ap = M._split(out["ap"].numpy(), nc, niou)
        rp, rr, rap, rf1, rcls = eval_ref.ap_per_class(tp, cf, pc, tc)
        assert np.array_equal(rcls, classes)
        for name, got, ref in (("p", p, rp), ("r", r, rr), ("ap", ap, rap), ("f1", f1, rf1)):          # the bound of tests/test_gpu_eval.py
            np.testing.assert_allclose(got[classes], ref, rtol=0, atol=1e-12, err_msg=name)
        cur = curves_ref.curves(tp, cf, pc, tc, B, fppi_grid=grid)
        for name, ref in (("pcurve", cur.p), ("rcurve", cur.r), ("f1curve", cur.f1), ("pycurve", cur.py)):   # the bounds of tests/test_gpu_curves.py
            np.testing.assert_allclose(out[name].numpy()[classes], ref, rtol=0, atol=1e-12, err_msg=name)
        assert np.array_equal(out["mr"].numpy()[classes], cur.mr_curve) and int(out["best"][0]) == cur.best
        for b in range(B):
            nb_ = int(counts[b])
            cls, conf_, nxywh, tl = confusion_ref.export_values(dets[b, :nb_].numpy(), (H, W), shapes[b])
            ex = out["export"][b].numpy()
            assert ex[:, 6].sum() == nb_ and not ex[nb_:].any()
            assert np.array_equal(ex[:nb_, 4], conf_) and np.array_equal(ex[:nb_, 5], cls)
            assert np.array_equal(ex[:nb_, 8:12], nxywh) and np.array_equal(ex[:nb_, 12:16], tl)
        want, skipped = confusion_ref.batch_matrix([dets[b, :int(counts[b])].numpy() for b in range(B)], t, (H, W), shapes, nc)
        assert np.array_equal(out["matrix"].numpy().reshape(nc + 1, nc + 1), want) and int(out["flag"][0]) == 0 and skipped == 0
    return case, check


sweep("cft_eval_match cft_eval_ap cft_eval_curves cft_eval_confusion cft_eval_export", "eval-chain")(_eval_builder)


# ------------------------------------------------------------------------------ detect boxes / render, plot_images' mosaic
def _atlas(gh=8, gw=6):
    return torch.randint(0, 256, (96, gh, gw), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)


def _render_table(imgs, irs):
    from msod_amd.utils.plots import RENDER_DESC
    desc = np.zeros(len(imgs), RENDER_DESC)
    for row, a, b in zip(desc, imgs, irs):
        row["img_rgb"], row["stride_rgb"], row["h0"], row["w0"] = a.data_ptr(), a.stride(0), a.shape[0], a.shape[1]
        if b is not None:
            row["img_ir"], row["stride_ir"] = b.data_ptr(), b.stride(0)
    return _pinned(desc)


def _detect_builder():
    """cft_detect_boxes on a two-image NMS output (one class outside [0, nc): the flag), then cft_detect_render into both streams."""
    import detect_ref
    B, max_det, nc = 2, 12, 3
    g = torch.Generator().manual_seed(21)
    dets = torch.zeros(B, max_det, 6)
    counts = torch.tensor([7, 3], dtype=torch.int32)
    for b in range(B):
        n = int(counts[b])
        xy = torch.rand(n, 2, generator=g) * 60
        dets[b, :n, :2], dets[b, :n, 2:4] = xy, xy + torch.rand(n, 2, generator=g) * 50 + 4
        dets[b, :n, 4] = torch.rand(n, generator=g).sort(descending=True)[0]
        dets[b, :n, 5] = torch.randint(0, nc, (n,), generator=g).float()
    dets[0, 2, 5] = 5.0
    sizes = [(50, 70), (64, 48)]
    geom = torch.tensor([[h, w, min(96 / h, 128 / w), (128 - w * min(96 / h, 128 / w)) / 2, (96 - h * min(96 / h, 128 / w)) / 2] for h, w in sizes])
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]
    names = torch.tensor([[ord(ch) for ch in nm] for nm in ("cat ", "dog ", "bird")], dtype=torch.uint8)
    name_len = torch.tensor([3, 3, 4], dtype=torch.int32)
    colors = torch.tensor([[255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=torch.uint8)
    atlas = _atlas()

    def case(run):
        lib = _lib()
        d, c, gm = run.inp("dets", dets), run.inp("counts", counts), run.inp("geom", geom)
        boxes, hist = run.out("boxes", (B, max_det, 16), torch.int32), run.out("hist", (B, nc), torch.int32)
        flag = run.inout("flag", torch.zeros(1, dtype=torch.int32))
        run.status(lib.cft_detect_boxes(_p(d), _p(c), B, max_det, _p(gm), nc, 1.02, 10.0, 0, _p(boxes), _p(hist), _p(flag), _stream()), "cft_detect_boxes")
        rgb = [run.inout(f"rgb{b}", imgs[b]) for b in range(B)]
        ir = [run.inout(f"ir{b}", imgs[b].flip(0).contiguous()) for b in range(B)]
        host = _render_table(rgb, ir)
        tdev = run.inp("desc", host)
        cd, nd, ld, ad = run.inp("colors", colors), run.inp("names", names), run.inp("name_len", name_len), run.inp("atlas", atlas)
        run.hold(host)
        run.status(lib.cft_detect_render(_p(tdev), host.data_ptr(), B, _p(boxes), max_det, _p(cd), nc, 225 | 255 << 8 | 255 << 16, 2, 3,
                                         _p(nd), _p(ld), 4, _p(ad), 8, 6, _stream()), "cft_detect_render")

    def check(out):
        ref = detect_ref.boxes_ref(dets.numpy(), counts.numpy(), geom.numpy(), nc)
        want = detect_ref.pack_slots(ref)
        assert np.array_equal(out["boxes"].numpy(), np.asarray(want).reshape(B, max_det, 16)) and int(out["flag"][0]) == 1
        assert np.array_equal(out["hist"].numpy(), ref["hist"])
        for b in range(B):           # the raster of tests/detect_ref.py, equal byte for byte as in tests/test_gpu_detect.py
            pair = [imgs[b].numpy().copy(), imgs[b].flip(0).contiguous().numpy().copy()]
            detect_ref.render_ref(pair, ref, b, colors.tolist(), (225, 255, 255), 2, True, True, ("cat", "dog", "bird"), atlas.numpy())
            assert np.array_equal(out[f"rgb{b}"].numpy(), pair[0]) and np.array_equal(out[f"ir{b}"].numpy(), pair[1]), b
        assert any(not torch.equal(out[f"rgb{b}"], imgs[b]) for b in range(B))          # something was drawn
    return case, check


def _mosaic_builder():
    """plot_images' four entry points on a [3, 6, 40, 56] fp32 batch, max_size 32: compose (resize, RGB and IR streams), slots from label
    rows, the cells drawn by cft_detect_render, finish (names + borders) and the INTER_AREA reduction."""
    from msod_amd.utils.plots import RENDER_DESC, mosaic_geometry, mosaic_render_flags
    B, H, W, nc, cap = 3, 40, 56, 3, 4
    gen = torch.Generator().manual_seed(17)
    images = torch.rand(B, 6, H, W, generator=gen)
    g = mosaic_geometry(B, H, W, 32, 16)
    rows = torch.tensor([[0, 1, 0.5, 0.5, 0.3, 0.4], [0, 2, 0.2, 0.3, 0.2, 0.2], [1, 0, 0.6, 0.4, 0.5, 0.5], [2, 1, 0.1, 0.1, 0.3, 0.3], [2, 7, 0.5, 0.5, 0.2, 0.2],
                         [1, 2, 0.3, 0.7, 0.2, 0.1], [1, 1, 0.8, 0.8, 0.3, 0.3], [1, 0, 0.5, 0.5, 0.9, 0.9], [1, 0, 0.4, 0.4, 0.1, 0.1]])
    codes = torch.zeros(g.bs, 40, dtype=torch.uint8)
    for i, nm in enumerate(("a.jpg", "image_two.png", "x")):          # = paths
        codes[i, :len(nm)] = torch.tensor([ord(ch) for ch in nm], dtype=torch.uint8)
    name_len = torch.tensor([5, 13, 1], dtype=torch.int32)
    cnames, clen = torch.tensor([[48], [49], [50]], dtype=torch.uint8), torch.ones(3, dtype=torch.int32)
    import mosaic_ref
    colors = torch.tensor(mosaic_ref.PALETTE[:nc], dtype=torch.uint8)
    atlas = _atlas()
    paths = ("a.jpg", "image_two.png", "x")
    mh, mw = g.ns * g.h, g.ns * g.w
    dh, dw = (mh + 1) // 2, (mw + 2) // 3

    def case(run):
        lib = _lib()
        img = run.inp("images", images)
        mos = [run.out(f"mosaic{s}", (mh, mw, 3), torch.uint8) for s in (0, 1)]
        maxkey = run.work("maxkey", (1,), torch.int32)
        for s in (0, 1):
            run.status(lib.cft_mosaic_compose(_p(img), 2, B, 6, H, W, *img.stride(), 3 * s, g.bs, g.ns, g.h, g.w, int(g.resize), _p(mos[s]), mw * 3,
                                              _p(maxkey), _stream()), "cft_mosaic_compose")
        rd = run.inp("rows", rows)
        slots = run.out("slots", (g.bs, cap, 16), torch.int32)
        flag = run.inout("flag", torch.zeros(1, dtype=torch.int32))
        sf = ctypes.c_double(g.sf)
        run.status(lib.cft_mosaic_slots(_p(rd), rows.shape[0], 6, 0, None, None, 0, 0, g.bs, cap, nc, g.h, g.w, ctypes.byref(sf), _p(slots), _p(flag),
                                        _stream()), "cft_mosaic_slots")
        desc = np.zeros(g.bs, RENDER_DESC)
        for i, row in enumerate(desc):
            off = g.h * (i % g.ns) * mw * 3 + g.w * (i // g.ns) * 3
            row["img_rgb"], row["img_ir"], row["stride_rgb"], row["stride_ir"] = mos[0].data_ptr() + off, mos[1].data_ptr() + off, mw * 3, mw * 3
            row["h0"], row["w0"] = g.h, g.w
        host = _pinned(desc)
        run.hold(host)
        tdev = run.inp("desc", host)
        cd, nd, ld, ad = run.inp("colors", colors), run.inp("cnames", cnames), run.inp("clen", clen), run.inp("atlas", atlas)
        run.status(lib.cft_detect_render(_p(tdev), host.data_ptr(), g.bs, _p(slots), cap, _p(cd), nc, 225 | 255 << 8 | 255 << 16, 3,
                                         mosaic_render_flags(False), _p(nd), _p(ld), 1, _p(ad), 8, 6, _stream()), "cft_detect_render")
        co, nl = run.inp("codes", codes), run.inp("name_len", name_len)
        run.status(lib.cft_mosaic_finish(_p(mos[0]), _p(mos[1]), mw * 3, mw * 3, g.bs, g.ns, g.h, g.w, _p(co), _p(nl), _p(ad), 8, 6, _stream()), "cft_mosaic_finish")
        small = run.out("reduced", (dh, dw * 3), torch.uint8, layout="rows", ld=dw * 3 + 5)
        run.status(lib.cft_mosaic_area(_p(mos[0]), mw * 3, mh, mw, _p(small), dw * 3 + 5, dh, dw, _stream()), "cft_mosaic_area")

    def check(out):
        assert int(out["flag"][0]) == 3                       # a class outside [0, nc) and a cell with more targets than cap
        slots, flag = mosaic_ref.slots_ref(rows.numpy(), g.bs, cap, nc, g.h, g.w, g.sf)
        assert np.array_equal(out["slots"].numpy(), slots) and flag == 3
        # compose, the drawn cells and finish: the whole restatement before the reduction, byte for byte (tests/test_gpu_mosaic.py)
        full, _, _ = mosaic_ref.plot_images_ref(images.numpy(), rows.numpy(), list(paths), ("0", "1", "2"), 32, 16, atlas.numpy(), reduce=False, cap=cap)
        assert np.array_equal(out["mosaic0"].numpy(), full[0]) and np.array_equal(out["mosaic1"].numpy(), full[1])
        want, mark = mosaic_ref.area_ref(out["mosaic0"].numpy(), dh, dw)
        mosaic_ref.assert_area_equal(out["reduced"].numpy().reshape(dh, dw, 3), want, mark)
    return case, check


sweep("cft_detect_boxes cft_detect_render", "detect-boxes-render")(_detect_builder)
sweep("cft_mosaic_compose cft_mosaic_slots cft_detect_render cft_mosaic_finish cft_mosaic_area", "mosaic-chain")(_mosaic_builder)


# ------------------------------------------------------------------------------ ComputeLoss forward / backward
def _loss_builder():
    """B = 2, three levels of 8 / 4 / 2 cells, about 50 targets, one of them with an image index outside the batch."""
    import loss_ref
    B, na, nc, cells = 2, 3, 3, (8, 4, 2)
    p = [_rnd(B, na, c, c, nc + 5, seed=50 + i) for i, c in enumerate(cells)]
    g = torch.Generator().manual_seed(53)
    nt = 50
    targets = torch.cat([torch.randint(0, B, (nt, 1), generator=g).float(), torch.randint(0, nc, (nt, 1), generator=g).float(),
                         torch.rand(nt, 2, generator=g) * 0.9 + 0.05, torch.rand(nt, 2, generator=g) * 0.4 + 0.05], 1)
    targets[17, 0] = 5.0
    anchors = torch.tensor([[[1.25, 1.625], [2.0, 3.75], [4.125, 2.875]], [[1.875, 3.8125], [3.875, 2.8125], [3.6875, 7.4375]],
                            [[3.625, 2.8125], [4.875, 6.1875], [11.65625, 10.1875]]])
    hyp = dict(box=0.05, obj=1.0, cls=0.5, cls_pw=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
    hv = (ctypes.c_double * 10)(hyp["box"], hyp["obj"], hyp["cls"], hyp["cls_pw"], hyp["obj_pw"], hyp["anchor_t"], hyp["fl_gamma"], 1.0, 0.0, 1.0)
    ny = (ctypes.c_int * 3)(*cells)

    def case(run):
        lib = _lib()
        pd = [run.inp(f"p{i}", t) for i, t in enumerate(p)]
        td, ad = run.inp("targets", targets), run.inp("anchors", anchors)
        bal = run.inout("balance", torch.tensor([4.0, 1.0, 0.4], dtype=torch.float64))
        nws = lib.cft_loss_workspace_bytes(3, B, na, ny, ny, nc, nt)
        ws = run.work("workspace", (nws,))
        loss, items = run.out("loss", (1,), F32), run.out("items", (4,), F32)
        err = run.inout("err", torch.zeros(1, dtype=torch.int32))
        ptrs = (ctypes.c_void_p * 3)(*[_p(t) for t in pd])
        run.status(lib.cft_loss_forward(3, ptrs, B, na, ny, ny, nc, _p(td), nt, _p(ad), hv, _p(bal), 0, 0, _p(ws), nws, _p(loss), _p(items), _p(err),
                                        _stream()), "cft_loss_forward")
        gl = run.inp("grad_loss", torch.ones(1))
        grads = [run.out(f"grad{i}", tuple(t.shape), F32) for i, t in enumerate(p)]
        gptrs = (ctypes.c_void_p * 3)(*[_p(t) for t in grads])
        run.status(lib.cft_loss_backward(3, ptrs, B, na, ny, ny, nc, nt, _p(ad), hv, _p(gl), gptrs, _p(ws), nws, _stream()), "cft_loss_backward")

    def check(out):
        from test_gpu_loss import _grad_ok
        ref = loss_ref.compute(p, targets, anchors, hyp, 1.0, [4.0, 1.0, 0.4])
        for i, gr in enumerate(ref["grads"]):
            ok, worst = _grad_ok(out[f"grad{i}"].numpy(), gr)
            assert ok, f"level {i}: gradient vs restatement, worst {worst:.3g} x tolerance"
        np.testing.assert_allclose(out["items"].double().numpy(), ref["items"], rtol=1e-6, atol=1e-8)          # the bounds of tests/test_gpu_loss.py
        np.testing.assert_allclose(out["loss"].item(), ref["loss"], rtol=1e-6)
        assert int(out["err"][0]) == ref["err"]
    return case, check


sweep("cft_loss_forward cft_loss_backward", "loss-8-4-2")(_loss_builder)


# ------------------------------------------------------------------------------ autoanchor
def _anchor_builder():
    import anchor_ref
    rng = np.random.default_rng(4)
    n, na, thr, gen, iters = 301, 9, 0.25, 5, 4
    wh = np.exp(rng.normal(3.5, 0.8, (n, 2))).astype(np.float32)
    k0 = np.exp(rng.normal(3.5, 0.8, (na, 2)))
    obs = wh.astype(np.float64) / wh.astype(np.float64).std(0)
    idx = np.stack([rng.choice(n, na, replace=False) for _ in range(iters)]).astype(np.int32)
    v = np.clip(rng.normal(1.0, 0.1, (gen, na, 2)), 0.3, 3.0)

    def case(run):
        lib = _lib()
        whd = run.inp("wh", torch.from_numpy(wh))
        kd = run.inp("k32", torch.from_numpy(k0.astype(np.float32)))
        met = run.out("metric", (8,), torch.int64)
        run.status(lib.cft_anchor_metric(_p(whd), n, _p(kd), na, thr, _p(met), _stream()), "cft_anchor_metric")
        nb = ctypes.c_long(0)
        assert lib.cft_anchor_kmeans_workspace_bytes(n, ctypes.byref(nb)) == 0
        kws = run.work("kmeans_ws", (nb.value,))
        od, ixd = run.inp("obs", torch.from_numpy(obs)), run.inp("idx", torch.from_numpy(idx))
        # include/cft_hip.h, cft_anchor_kmeans: "book [k, 2] float64: the winning code book, its first info[0] rows" - rows past the surviving codes are unspecified
        book = run.out("book", (na, 2), torch.float64, defined=lambda o: (torch.arange(na) < int(o["info"][0])).view(na, 1))
        dist, info = run.out("dist", (1,), torch.float64), run.out("info", (4,), torch.int32)
        run.status(lib.cft_anchor_kmeans(_p(od), n, na, _p(ixd), iters, _p(kws), nb.value, _p(book), _p(dist), _p(info), _stream()), "cft_anchor_kmeans")
        assert lib.cft_anchor_evolve_workspace_bytes(gen, ctypes.byref(nb)) == 0
        ews = run.work("evolve_ws", (nb.value,))
        vd = run.inp("v", torch.from_numpy(v))
        kk = run.inout("k", torch.from_numpy(k0.copy()))
        f, flags, fg = run.out("f", (1,), F32), run.out("flags", (gen,), torch.int32), run.out("fg", (gen,), F32)
        run.status(lib.cft_anchor_evolve(_p(whd), n, na, thr, _p(vd), gen, _p(kk), _p(f), _p(flags), _p(fg), _p(ews), nb.value, _stream()), "cft_anchor_evolve")

    def check(out):
        from msod_amd.utils.autoanchor import AnchorMetric
        got, want = AnchorMetric(out["metric"].tolist(), n, na), anchor_ref.metric(wh, k0.astype(np.float32), thr)
        assert (got.n_best_above, got.n_x_above) == (want["n_best_above"], want["n_x_above"])
        assert got.sum_x == want["sum_x"] and got.sum_best == want["sum_best"]
        assert got.sum_x_above == want["sum_x_above"] and got.sum_best_above == want["sum_best_above"]
        rbook, rdist, _ = anchor_ref.kmeans(obs, na, idx)
        book = out["book"].numpy()[:int(out["info"][0])]
        by_area = lambda b: b[np.lexsort((b[:, 0], b.prod(1)))]      # noqa: E731      (the comparison of test_kmeans_equals_scipys)
        assert len(book) == len(rbook)
        np.testing.assert_allclose(by_area(book), by_area(rbook), rtol=1e-9, atol=0)
        np.testing.assert_allclose(float(out["dist"][0]), rdist, rtol=1e-9, atol=0)
        k, f, flags, fg = anchor_ref.evolve(wh, k0, thr, v)
        assert out["k"].numpy().tobytes() == k.tobytes() and np.array_equal(out["flags"].numpy().astype(bool), flags)
        assert out["fg"].numpy().tobytes() == fg.tobytes() and out["f"].numpy().tobytes() == np.float32(f).tobytes()
    return case, check


sweep("cft_anchor_metric cft_anchor_kmeans cft_anchor_evolve", "autoanchor")(_anchor_builder)


# ------------------------------------------------------------------------------ optimiser steps
def _optim_builder(which):
    """Three segments of ragged length (5000 from an odd storage offset: the dword path; 4096: one full 16-byte chunk; 33) and a frozen
    tensor next to them that no table row names."""
    import adam_ref
    import optim_ref
    from msod_amd.utils.optim import work_rows
    lens = (5000, 4096, 33)
    ps = [_rnd(n + 1, seed=80 + i) for i, n in enumerate(lens)]
    gs = [_rnd(n + 1, seed=90 + i, scale=0.1) for i, n in enumerate(lens)]
    bs = [_rnd(n + 1, seed=100 + i, scale=0.05) for i, n in enumerate(lens)]
    vs = [_rnd(n + 1, seed=110 + i, scale=0.05).abs() for i, n in enumerate(lens)]
    frozen = _rnd(77, seed=120)
    first = (1, 0, 0)                      # segment 0 starts one element into its storage
    groups = (0, 1, 0)
    chunk = 4096

    def table(cols):
        rows = np.array(cols, dtype=np.int64)
        work = work_rows(np.array(lens, dtype=np.int64), chunk)
        return torch.from_numpy(np.concatenate([rows.reshape(-1), work.reshape(-1)])), work.shape[0]

    def case(run):
        lib = _lib()
        run.inp("frozen", frozen)
        at = lambda t, i: t.data_ptr() + 4 * first[i]
        P = [run.inout(f"p{i}", t) for i, t in enumerate(ps)]
        if which == "ema":
            Mo = [run.inp(f"m{i}", t) for i, t in enumerate(gs)]
            host, nwork = table([(at(P[i], i), at(Mo[i], i), lens[i]) for i in range(3)])
            run.hold(host)
            dev = run.inp("table", host)
            run.status(lib.cft_ema_update(_p(dev), host.data_ptr(), 3, nwork, chunk, 0, 0.9990000128746033, 0.0010000000474974513, _stream()), "cft_ema_update")
            return
        Gr = [run.inp(f"g{i}", t) for i, t in enumerate(gs)]
        Bu = [run.inout(f"b{i}", t) for i, t in enumerate(bs)]
        if which == "sgd":
            host, nwork = table([(at(P[i], i), at(Gr[i], i), at(Bu[i], i), lens[i], groups[i]) for i in range(3)])
            run.hold(host)
            dev = run.inp("table", host)
            hyper = (ctypes.c_float * 8)(0.01, 0.937, 0.0, 1.0, 0.02, 0.9, 0.0005, 0.0)
            run.status(lib.cft_sgd_step(_p(dev), host.data_ptr(), 3, nwork, chunk, 0, hyper, 2, None, None, _stream()), "cft_sgd_step")
        else:
            Va = [run.inout(f"v{i}", t) for i, t in enumerate(vs)]
            steps = run.inout("steps", torch.tensor([3.0, 3.0, 0.0]))
            coef = run.work("coef", (3, 2), F32)
            host, nwork = table([(at(P[i], i), at(Gr[i], i), at(Bu[i], i), at(Va[i], i), steps.data_ptr() + 4 * i, lens[i], groups[i]) for i in range(3)])
            run.hold(host)
            dev = run.inp("table", host)
            hyper = (ctypes.c_double * 12)(0.001, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.002, 0.937, 0.999, 1e-8, 0.01, 1.0)
            run.status(lib.cft_adam_step(_p(dev), host.data_ptr(), 3, nwork, chunk, 0, hyper, 2, _p(coef), None, None, _stream()), "cft_adam_step")

    def check(out):
        for i, n in enumerate(lens):
            sl = slice(first[i], first[i] + n)
            rest = np.ones(n + 1, bool)
            rest[sl] = False
            assert np.array_equal(out[f"p{i}"].numpy()[rest], ps[i].numpy()[rest])            # elements outside the segment are not touched
            if which == "sgd":
                hy = ((0.01, 0.937, 0.0, True), (0.02, 0.9, 0.0005, False))[groups[i]]
                p1, b1, bound_p, bound_b = optim_ref.sgd_step(ps[i][sl], gs[i][sl], bs[i][sl], *hy)           # the bounds of tests/test_gpu_optim.py
                assert optim_ref.worst(out[f"p{i}"][sl], p1, bound_p) <= 1.0 and optim_ref.worst(out[f"b{i}"][sl], b1, bound_b) <= 1.0
            elif which == "ema":
                e1, bound = optim_ref.ema_update(ps[i][sl], gs[i][sl], 0.999)
                assert optim_ref.worst(out[f"p{i}"][sl], e1, bound) <= 1.0
            elif which == "adam":
                hy = ((0.001, 0.9, 0.999, 1e-8, 0.0, False), (0.002, 0.937, 0.999, 1e-8, 0.01, True))[groups[i]]
                p1, m1, v1, bp, bm, bv = adam_ref.adam_step(ps[i][sl], gs[i][sl], bs[i][sl], vs[i][sl], (4, 4, 1)[i], *hy)      # the bounds of tests/test_gpu_adam.py
                for name, got, ref, bound in (("p", out[f"p{i}"], p1, bp), ("m", out[f"b{i}"], m1, bm), ("v", out[f"v{i}"], v1, bv)):
                    assert optim_ref.worst(got[sl], ref, bound) <= 1.0, (name, i)
        if which == "adam":
            assert out["steps"].tolist() == [4.0, 4.0, 1.0]
    return case, check


for _w in ("sgd", "ema", "adam"):
    sweep({"sgd": "cft_sgd_step", "ema": "cft_ema_update", "adam": "cft_adam_step"}[_w], f"optim-{_w}")(lambda w=_w: _optim_builder(w))


# ------------------------------------------------------------------------------ test-time augmentation
def _tta_builder():
    import tta_ref
    from msod_amd import ops
    B, H, W, gs = 2, 40, 56, 32
    g = torch.Generator().manual_seed(6)
    six = torch.randint(0, 256, (B, 6, H, W), generator=g, dtype=torch.uint8)
    ratio = 0.83
    _, (Ho, Wo) = ops.tta_view_size(H, W, ratio, gs)
    no, ns = 8, (21, 13, 9)
    ys = [_rnd(B, n, no, seed=60 + i).abs() * 20 for i, n in enumerate(ns)]

    def case(run):
        lib = _lib()
        img = run.inp("img6", six)[:, 3:6]
        view = run.out("view", (B, 3, Ho, Wo), F32)
        r = ctypes.c_double(ratio)
        run.status(lib.cft_tta_view(_p(img), 0, B, H, W, *img.stride(), ctypes.byref(r), gs, 1, _p(view), Ho, Wo, _stream()), "cft_tta_view")
        yd = [run.inp(f"y{i}", t) for i, t in enumerate(ys)]
        merged = run.out("merged", (B, sum(ns), no), F32)
        run.status(lib.cft_tta_merge(_p(yd[0]), _p(yd[1]), _p(yd[2]), B, *ns, no, 1.0, 0.83, 0.67, 2, float(W), _p(merged), sum(ns), _stream()), "cft_tta_merge")

    def check(out):
        assert np.array_equal(out["view"].numpy(), np.asarray(tta_ref.view(six[:, 3:6].numpy(), ratio, gs, flip=True), np.float32))
        assert np.array_equal(out["merged"].numpy(), np.asarray(tta_ref.merge([t.numpy() for t in ys], (1.0, 0.83, 0.67), (False, True, False), float(W)), np.float32))
    return case, check


sweep("cft_tta_view cft_tta_merge", "tta")(_tta_builder)


# ------------------------------------------------------------------------------ data loaders: pair batch, augmented batch, JPEG
def _pair_builder():
    """Three pairs in one launch: a copy, an INTER_LINEAR enlargement and an INTER_AREA reduction, into a 64 x 64 letterbox."""
    from msod_amd.utils.datasets import PAIR_DESC
    g = torch.Generator().manual_seed(8)
    geo = [(40, 64, 40, 64, 0), (20, 30, 43, 64, 1), (100, 150, 43, 64, 2)]          # h0, w0, h, w, mode
    src = [(torch.randint(0, 256, (h0, w0, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (h0, w0, 3), generator=g, dtype=torch.uint8))
           for h0, w0, _, _, _ in geo]
    B, D = len(geo), 64

    def case(run):
        desc = np.zeros(B, PAIR_DESC)
        for i, (row, (h0, w0, h, w, mode)) in enumerate(zip(desc, geo)):
            a, b = run.inp(f"rgb{i}", src[i][0]), run.inp(f"ir{i}", src[i][1])
            row["src_rgb"], row["src_ir"], row["stride_rgb"], row["stride_ir"] = a.data_ptr(), b.data_ptr(), 3 * w0, 3 * w0
            row["h0"], row["w0"], row["h"], row["w"], row["top"], row["left"], row["mode"], row["flip"] = h0, w0, h, w, (D - h) // 2, (D - w) // 2, mode, 0
        host = _pinned(desc)
        run.hold(host)
        dev = run.inp("desc", host)
        dst = run.out("batch", (B, 6, D, D), torch.uint8)
        run.status(_lib().cft_pair_batch_u8(_p(dev), host.data_ptr(), B, _p(dst), D, D, 114, _stream()), "cft_pair_batch_u8")

    def check(out):
        from test_gpu_dataset import assert_block, expected_block          # the CPU restatements and the bound of test_recorded_batches
        for i, (h0, w0, h, w, mode) in enumerate(geo):
            want, mark = expected_block(src[i][0].numpy(), src[i][1].numpy(), h, w, (D - h) // 2, (D - w) // 2, mode, D, D)
            assert_block(out["batch"][i].numpy(), want, mark, f"pair {i} mode {mode}")
    return case, check


def _augment_builder():
    """Two output images in one launch: a letterboxed pair (plain read, both flips) and a four-tile mosaic through the affine warp."""
    from msod_amd.utils.datasets import AUG_DESC
    g = torch.Generator().manual_seed(10)
    D = 32
    mk = lambda h, w: torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    src = [(mk(20, 24), mk(20, 24))] + [(mk(40, 40), mk(40, 40)) for _ in range(4)]
    luts = torch.randint(0, 256, (2, 2, 3, 256), generator=g, dtype=torch.uint8)
    luts[:, :, 0] %= 180
    INV = (1.5, 0.1, 5.0, -0.1, 1.6, 3.0)
    geo = [(20, 24, 20, 24, 4, 6, 28, 26, 4, 6)] + [(40, 40, 32, 32, x1, y1, x1 + D, y1 + D, x1, y1) for x1, y1 in ((0, 0), (D, 0), (0, D), (D, D))]
    TILES = [dict(zip(("h0", "w0", "h", "w", "x1", "y1", "x2", "y2", "padw", "padh"), t), rgb=src[i][0].numpy(), ir=src[i][1].numpy())
             for i, t in enumerate(geo)]

    def case(run):
        desc = np.zeros(2, AUG_DESC)
        S = [(run.inp(f"rgb{i}", a), run.inp(f"ir{i}", b)) for i, (a, b) in enumerate(src)]

        def tile(t, s, h0, w0, h, w, x1, y1, x2, y2, padw, padh):
            assert (h0, w0, h, w, x1, y1, x2, y2, padw, padh) == tuple(TILES[s][k] for k in ("h0", "w0", "h", "w", "x1", "y1", "x2", "y2", "padw", "padh"))
            t["src_rgb"], t["src_ir"], t["stride_rgb"], t["stride_ir"] = S[s][0].data_ptr(), S[s][1].data_ptr(), 3 * w0, 3 * w0
            t["h0"], t["w0"], t["h"], t["w"] = h0, w0, h, w
            t["x1"], t["y1"], t["x2"], t["y2"], t["padw"], t["padh"] = x1, y1, x2, y2, padw, padh
        desc[0]["ntiles"], desc[0]["warp"], desc[0]["canvas_h"], desc[0]["canvas_w"], desc[0]["flip"] = 1, 0, D, D, 3
        tile(desc[0]["tile"][0], 0, 20, 24, 20, 24, 4, 6, 28, 26, 4, 6)
        desc[1]["ntiles"], desc[1]["warp"], desc[1]["canvas_h"], desc[1]["canvas_w"], desc[1]["flip"] = 4, 1, 2 * D, 2 * D, 1
        desc[1]["inv"] = INV
        for q, (x1, y1) in enumerate(((0, 0), (D, 0), (0, D), (D, D))):
            tile(desc[1]["tile"][q], 1 + q, 40, 40, 32, 32, x1, y1, x1 + D, y1 + D, x1, y1)
        host = _pinned(desc)
        run.hold(host)
        dev, ld = run.inp("desc", host), run.inp("luts", luts)
        dst = run.out("batch", (2, 6, D, D), torch.uint8)
        run.status(_lib().cft_augment_batch_u8(_p(dev), host.data_ptr(), _p(ld), 2, _p(dst), D, D, _stream()), "cft_augment_batch_u8")

    def check(out):
        import augment_ref          # the numpy raster of tests/augment_ref.py, byte for byte as in tests/test_gpu_augment.py
        rows = [dict(ntiles=1, warp=0, canvas_h=D, canvas_w=D, flip=3, inv=(0,) * 6, tiles=TILES[:1]),
                dict(ntiles=4, warp=1, canvas_h=2 * D, canvas_w=2 * D, flip=1, inv=INV, tiles=TILES[1:])]
        want = np.stack([augment_ref.render_row(r, l, D, D) for r, l in zip(rows, luts.numpy())])
        assert np.array_equal(out["batch"].numpy(), want), f"{int((out['batch'].numpy() != want).sum())} bytes differ"
    return case, check


def _jpeg_builder():
    """One decode and one encode of a ragged 37 x 29 4:2:0 image: PIL's decode is the decoder's yardstick byte for byte, the
    coefficients of PIL's file the encoder's (real blocks; the dummy blocks are zero)."""
    import jpeg_enc_ref
    import jpeg_ref
    from msod_amd.utils import jpeg as J
    h, w, q = 29, 37, 75
    arr = jpeg_enc_ref.content(jpeg_enc_ref.CONTENTS[0], h, w, 5)
    blob = jpeg_ref.encode(arr, "420", q)
    want = jpeg_ref.pil_decode(blob)
    info, coef, qtab = jpeg_ref.entropy(blob)
    nblk = int(sum(int(info["bw"][c]) * int(info["bh"][c]) for c in range(3)))
    qt = jpeg_enc_ref.quality_tables(q)

    def case(run):
        lib = _lib()
        cd, qd = run.inp("coef", torch.from_numpy(coef.copy())), run.inp("qtab", torch.from_numpy(qtab.astype(np.uint16).view(np.int16).copy()))
        dst = run.out("rgb", (h, 3 * w), torch.uint8, layout="rows", ld=3 * w + 9)
        ws = run.work("planes", (64 * nblk,))
        desc = np.zeros(1, J.JPEG_DESC)
        r = desc[0]
        r["coef"], r["qtab"], r["dst"], r["dst_stride"], r["plane_off"] = cd.data_ptr(), qd.data_ptr(), dst.data_ptr(), 3 * w + 9, 0
        for k in ("width", "height", "ncomp", "hmax", "vmax", "bw", "bh"):
            r[k] = info[k]
        host = _pinned(desc)
        dev = run.inp("dec_table", host)
        run.status(lib.cft_jpeg_decode_u8(_p(dev), host.data_ptr(), 1, _p(ws), 64 * nblk, _stream()), "cft_jpeg_decode_u8")
        sd = run.inp("src", torch.from_numpy(arr.copy()).reshape(h, 3 * w), layout="rows", ld=3 * w + 7)
        qh = torch.from_numpy(qt.view(np.int16).copy())
        eq = run.inp("enc_qtab", qh)
        out = run.out("enc_coef", (64 * nblk,), torch.int16)
        ed = np.zeros(1, J.JPEG_ENC_DESC)
        e = ed[0]
        e["src"], e["qtab"], e["qtab_host"], e["coef"], e["src_stride"] = sd.data_ptr(), eq.data_ptr(), qh.data_ptr(), out.data_ptr(), 3 * w + 7
        for k in ("width", "height", "ncomp", "hmax", "vmax", "bw", "bh"):
            e[k] = info[k]
        ehost = _pinned(ed)
        run.hold(host, ehost, qh)
        edev = run.inp("enc_table", ehost)
        run.status(lib.cft_jpeg_encode_coef(_p(edev), ehost.data_ptr(), 1, _stream()), "cft_jpeg_encode_coef")

    def check(out):
        assert np.array_equal(out["rgb"].numpy().reshape(h, w, 3), want)
        mask = np.repeat(jpeg_enc_ref.real_block_mask(info), 64)
        got = out["enc_coef"].numpy()
        assert np.array_equal(got[mask], coef[mask]) and not got[~mask].any()
    return case, check


sweep("cft_pair_batch_u8", "pair-batch")(_pair_builder)
sweep("cft_augment_batch_u8", "augment-batch")(_augment_builder)
sweep("cft_jpeg_decode_u8 cft_jpeg_encode_coef", "jpeg")(_jpeg_builder)


# ------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("ident", [c[0] for c in CASES])
def test_sweep(dev, ident):
    global DEV
    DEV = dev
    _, declared, builder = next(c for c in CASES if c[0] == ident)
    case, check = builder()
    launched = set()
    out = G.check_case(case, dev, launched=launched)
    assert launched == set(declared), f"the table declares {sorted(declared)}, the case launched {sorted(launched)}"
    if check is not None:
        check(out)


# ------------------------------------------------------------------------------ the allocations a caller cannot reach
# Many scratch tensors are allocated inside the package (torch.empty / new_nhwc / new_empty): a guarded buffer cannot replace them.
# The fixture below makes every such allocation come back filled with the run's byte - NaN or the large finite value for float
# types, -1 or 0x7B7B... for integer types - which is deterministic and does not depend on how the caching allocator recycles blocks.
# Each workload is rebuilt from scratch under each fill (so that cached plans and buffers are allocated under that fill too) and
# runs eagerly; its results must be bit-identical across the three fills.  Captured-graph replays are out of scope: a fill issued
# during capture would become part of the graph.
def _fill_value(t, fill):
    """Fill a fresh tensor so that every byte of every element is ``fill`` (any strides)."""
    if t.numel() == 0:
        return t
    if t.dtype == torch.bool:
        return t.fill_(bool(fill))
    if t.is_complex():
        return t
    es = t.element_size()
    return t.copy_(torch.full((es,), fill, dtype=torch.uint8).view(t.dtype)[0].to(t.device))      # a same-dtype copy keeps the bit pattern


@pytest.fixture
def poisoned_allocations(monkeypatch):
    state = {"fill": 0x00, "count": 0}

    def wrap(orig):
        def alloc(*a, **k):
            t = orig(*a, **k)
            state["count"] += 1
            with torch.no_grad():
                return _fill_value(t, state["fill"])
        return alloc
    for name in ("empty", "empty_like", "empty_strided"):
        monkeypatch.setattr(torch, name, wrap(getattr(torch, name)))
    monkeypatch.setattr(torch.Tensor, "new_empty", wrap(torch.Tensor.new_empty))
    return state


def _bits(obj):
    """Every tensor / array / scalar of a nested result as bytes, in a fixed order."""
    import dataclasses
    if isinstance(obj, torch.Tensor):
        return [obj.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if obj.numel() else b""]
    if isinstance(obj, np.ndarray):
        return [np.ascontiguousarray(obj).tobytes()]
    if isinstance(obj, (list, tuple)):
        return [b for o in obj for b in _bits(o)]
    if isinstance(obj, dict):
        return [b for k in sorted(obj, key=str) for b in _bits(obj[k])]
    if dataclasses.is_dataclass(obj) and not isinstance(obj, type):
        return _bits(dataclasses.asdict(obj))
    return [repr(obj).encode()]


def _wl_forward(dev):
    """The two-stream forward at the (5, 32, 32) shape of test_small_odd_shapes_match_oracle and at (1, 64, 96), three precisions."""
    from msod_amd.utils.seeded import seeded_inputs
    from test_gpu_model import _seeded
    _, model, _ = _seeded("yolov5s_fusion_transformerx3_vedai", 21)
    model = model.to(dev)
    out = []
    for b, h, w in ((5, 32, 32), (1, 64, 96)):
        rgb, ir = seeded_inputs(b, h, w, 21)
        for dtype in DTYPES:
            model.set_compute_dtype(dtype)
            with torch.no_grad():
                pred, raw = model(rgb.to(dev), ir.to(dev))
            torch.cuda.synchronize()
            out.append((pred.cpu(), [r.cpu() for r in raw]))
    return out


def _wl_single(dev):
    """The single-stream tiny model, plain and with augment=True."""
    import test_gpu_single as S
    model, x = S.build(S.golden("tta_64x64")["case"], dev)
    x = x.to(dev)
    out = []
    for dtype in (F32, BF16):
        pred, raw = S.run(model, x, dtype)
        out.append((pred.cpu(), [r.cpu() for r in raw], S.run(model, x, dtype, augment=True)[0].cpu()))
    return out


def _wl_gpt(dev):
    """models.common.GPT at d = 128 on the 8 x 8 grid and on a regridded one, in eval mode and in train mode with a fixed dropout seed."""
    from helpers import to_dev_nhwc
    from msod_amd import ops
    from msod_amd.models.common import GPT
    out = []
    for va, ha in ((8, 8), (5, 3)):
        torch.manual_seed(7)
        m = GPT(128, h=8, vert_anchors=va, horz_anchors=ha)
        with torch.no_grad():
            m.pos_emb.copy_(_rnd(*m.pos_emb.shape, seed=va, scale=0.2))
        m = m.to(dev)
        rgb, ir = _rnd(2, 128, 20, 24, seed=11), _rnd(2, 128, 20, 24, seed=12)
        for train in (False, True):
            m.train(train)
            ops.manual_dropout_seed(99)
            for dtype in (F32, BF16):
                with torch.no_grad():
                    o = m([to_dev_nhwc(rgb, dev, dtype), to_dev_nhwc(ir, dev, dtype)])
                    out.append([p.materialize().cpu() if hasattr(p, "materialize") else p.cpu() for p in o])
        torch.cuda.synchronize()
    return out


def _wl_train_forward(dev):
    """The two-stream model in train mode (the recorded 96-pixel training case): every Conv runs cft_batchnorm_train on scratch that
    ops.batchnorm_train allocates, the GPT blocks run their dropouts under a fixed seed; raw outputs and every running statistic."""
    import test_train as TT
    from msod_amd import ops
    _, _, model, _, rgb, ir = TT._case()
    out = []
    for dtype in (F32, BF16):
        model = model.to(dev).set_compute_dtype(dtype).train()
        ops.manual_dropout_seed(1234)
        with torch.no_grad():
            raws = model(rgb.to(dev), ir.to(dev))
        torch.cuda.synchronize()
        out.append([r.cpu() for r in raws])
    out.append([b.cpu() for b in model.buffers()])
    return out


def _wl_eval(dev):
    """NMS -> evaluate over the smallest recorded evaluation case: stats, AP, curves, confusion matrix, export rows."""
    import test_gpu_eval as E
    from msod_amd.utils import metrics as M
    from msod_amd.utils.general import batched_nms
    cases = [c for c in torch.load(E.GOLDEN, weights_only=False)["cases"] if c["stats"] is not None]
    case = min(cases, key=lambda c: sum(b["rows"].numel() for b in c["batches"]))
    nc = 1 if case["single_cls"] else case["nc"]
    ev = M.DetectionEvaluator(nc, single_cls=case["single_cls"], confusion=True)
    out = []
    for b in case["batches"]:
        dets, counts = batched_nms(b["rows"].to(dev), case["conf_thres"], case["iou_thres"], multi_label=True, agnostic=case["single_cls"])
        ev.update(dets, counts, b["targets"].to(dev), b["img_hw"], b["shapes"])
        out.append((dets.cpu(), counts.cpu(), M.export_batch(dets, counts, b["img_hw"], b["shapes"], case["single_cls"]).cpu()))
    res, cur = ev.compute(), ev.curves()
    return out, res.as_test_tuple(), res.p, res.r, res.ap, res.f1, res.confusion_matrix, cur


def _wl_loss(dev):
    """ComputeLoss forward and backward on the smallest recorded loss case."""
    import test_gpu_loss as TL
    from msod_amd.utils import loss as L
    c = min(torch.load(TL.GOLDEN, weights_only=False)["cases"], key=lambda c: sum(t.numel() for t in c["calls"][0]["p"]))
    cl = L.ComputeLoss(TL._stub(c["nc"], c["hyp"], c["gr"], dev), autobalance=c["autobalance"])
    out = []
    for call in c["calls"]:
        loss, items, grads = TL._run(cl, [t.float().to(dev) for t in call["p"]], c["targets"])
        out.append((loss.cpu(), items.cpu(), [g.cpu() for g in grads], cl.balance))
    return out


def _wl_train_step(dev):
    """One SGD step with EMA, and one Adam step, on the tiny two-stream model; then a forward on the stepped weights."""
    import test_gpu_optim as TO
    from msod_amd.utils import optim, torch_utils
    hyp = torch.load(TO.GOLDEN, weights_only=False)["sgd"]["hyp"]
    out = []
    for adam in (False, True):
        cfg, model, x, x2 = TO._small_model(dev)
        ema = torch_utils.ModelEMA(model)
        opt = optim.build_adam_optimizer(model, hyp) if adam else optim.build_optimizer(model, hyp)
        TO._seeded_model_grads(model)
        opt.step()
        ema.update(model)
        with torch.no_grad():
            pred = model(x, x2)[0]
        torch.cuda.synchronize()
        out.append((pred.cpu(), [p.detach().cpu() for p in model.parameters()], [v.cpu() for v in ema.ema.state_dict().values()]))
    return out


def _wl_anchors(dev):
    """check_anchors on the smallest autoanchor case."""
    import test_gpu_autoanchor as TA
    from msod_amd.utils import autoanchor as aa
    c = {c["name"]: c for c in torch.load(TA.GOLDEN, weights_only=False)["cases"]}["small_170_n9"]
    model = TA.small_model(dev, c["check_anchor_list"])
    np.random.seed(c["seed"])
    _, text = TA.quiet(getattr(aa, c["check"]), TA.dataset(c), model, thr=4.0, imgsz=640)
    m = model.model[-1]
    return m.anchors.cpu(), m.anchor_grid.cpu(), text


def _wl_jpeg(dev):
    """One decode and one encode of the smallest JPEG fixture pair."""
    import jpeg_enc_ref
    import jpeg_ref
    from msod_amd.utils import jpeg as J
    arr = jpeg_enc_ref.content("mixed", 29, 37, 5)
    blob = jpeg_ref.encode(arr, "420", 75)
    got = J.decode_jpeg_batch([blob], dev)
    files = J.encode_jpeg_batch([torch.from_numpy(arr).to(dev)], 75, "4:2:0")
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), jpeg_ref.pil_decode(blob))
    return got[0].cpu(), files


def _wl_loaders(dev):
    """One batch each from the validation and from the training loader on the fixture images."""
    import random
    from types import SimpleNamespace
    import test_gpu_augment as TA
    import test_gpu_dataset as TD
    from msod_amd.utils import datasets as D
    c = TD.VAL
    loader, _ = TD.quiet(D.create_dataloader_rgb_ir, TD.RGB_DIR, TD.IR_DIR, c["img_size"], c["batch_size"], c["stride"], SimpleNamespace(single_cls=False),
                         pad=c["pad"], rect=c["rect"])
    val = next(iter(loader))
    random.seed(3)
    np.random.seed(3)
    tl, _ = TA._loader(TA.B64)
    tr = next(iter(tl))
    torch.cuda.synchronize()
    return list(val), list(tr)


def _wl_plot_images(dev):
    """plot_images on one six-channel batch with label rows and file names (the mosaic of both streams, reduced)."""
    from msod_amd.utils import plots as P
    images = torch.rand(3, 6, 40, 56, generator=torch.Generator().manual_seed(17))
    rows = torch.tensor([[0, 1, 0.5, 0.5, 0.3, 0.4], [0, 2, 0.2, 0.3, 0.2, 0.2], [1, 0, 0.6, 0.4, 0.5, 0.5], [2, 1, 0.1, 0.1, 0.3, 0.3]])
    mosaics, flag, _ = P.plot_images_device(images.to(dev), rows, ["a.jpg", "b.jpg", "c.jpg"], ("cat", "dog", "bird"), max_size=32)
    torch.cuda.synchronize()
    return [m.cpu() for m in mosaics], flag.cpu()


WORKLOADS = {"forward": _wl_forward, "single": _wl_single, "gpt": _wl_gpt, "train_forward": _wl_train_forward, "eval": _wl_eval, "loss": _wl_loss, "train_step": _wl_train_step,
             "check_anchors": _wl_anchors, "jpeg": _wl_jpeg, "loaders": _wl_loaders, "plot_images": _wl_plot_images}


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_results_do_not_depend_on_what_fresh_allocations_hold(dev, poisoned_allocations, name):
    first = None
    for fill in G.FILLS:
        poisoned_allocations["fill"] = fill
        before = poisoned_allocations["count"]
        bits = _bits(WORKLOADS[name](dev))
        assert poisoned_allocations["count"] > before, "the workload allocated nothing through the patched functions"
        if first is None:
            first = bits
            continue
        assert len(bits) == len(first)
        differ = [i for i, (a, b) in enumerate(zip(bits, first)) if a != b]
        assert not differ, f"{name}: results {differ} of {len(bits)} differ between fill 0x00 and fill 0x{fill:02X}"
