"""The contract of the tensor-level wrappers of ``msod_amd.ops``, as one table: which views of a tensor a wrapper accepts (and must
compute exactly as on dense operands) and which it refuses (and with which exception) before anything reaches the library.

One ``Entry`` per wrapper and shape: a builder of dense seeded operands, the tensor arguments with their kind / role (from which the
accepted view families and the generic refused cases follow) and the refused cases that are the wrapper's own.  Shared by
tests/test_ops_contract_host.py (CPU tensors, a stub library: what is handed over) and tests/test_gpu_ops_contract.py (the real
library on accepted views, the stub on refused ones).

Granule ``ge``: 8 elements for bf16 / f16, 4 for f32.  cft_conv2d and its relatives (``linear``, the chained kernels) store outputs and
read residuals in units of 8 elements whatever the dtype (include/cft_hip.h: n, ldy, ldr multiples of 8), so the row stride of their
2-D fp32 operands is padded by 8 where the other wrappers' is padded by ``ge``: ``Arg.ge8``.
"""
import math
from dataclasses import dataclass, field
from typing import Callable

import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
LOWP = (torch.bfloat16, torch.float16)
DTYPE_IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
OTHER = {torch.bfloat16: torch.float16, torch.float16: torch.bfloat16, torch.float32: torch.bfloat16}      # "a wrong dtype" of each

SLICES = ("slice@0", "slice@ge", "slice@C+ge")       # channel slices of a buffer with ld = 2C + 2ge
CONVERTED = ("nchw", "channels_last", "unaligned")   # what as_nhwc converts (inputs only)


def granule(dtype):
    return 4 if dtype == torch.float32 else 8


def rnd(shape, seed, dtype=torch.float32, dev="cpu", scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def pattern(shape, dtype, dev, seed=999):
    """The fill of everything a kernel must leave alone: seeded, finite, unlike any result."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 64 + 1000).to(dtype).to(dev)


def nhwc(t):
    """The same logical [B,C,H,W] values in a fresh NHWC buffer."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def on_meta(t):
    """The same shape / strides / dtype on another device (one that needs no hardware)."""
    return torch.empty_strided(tuple(t.shape), tuple(t.stride()), dtype=t.dtype, device="meta")


@dataclass
class Arg:
    kind: str                   # "nhwc": logical [B,C,H,W] in NHWC memory; "rows": [rows, C]; "dense": contiguous, aligned; "aux": raw-pointer parameter;
                                # "any": any strides (images)
    role: str = "in"            # "in": converted where as_nhwc can; "nocopy": read in place (residuals); "out"; "inout"
    ld: tuple = ()              # names of the library call's parameters that follow this argument's strides
    ge8: bool = False           # the 8-element unit of cft_conv2d's outputs / residuals
    dtype_free: bool = False    # any compute dtype is legal here (no wrong-dtype case)
    families: tuple = None      # accepted view families; None: the defaults of kind and role

    def accepted(self):
        if self.families is not None:
            return self.families
        if self.kind == "nhwc":
            return SLICES + ("batch",) + (CONVERTED if self.role == "in" else ())
        if self.kind == "rows":
            return ("rowstride",)
        return ()


def embed(t, family, ge, seed=999):
    """``(view, buffer, mask)``: a view of ``family`` holding the values of ``t``; the enclosing buffer (pattern filled) and the mask of
    the view's elements in it, or None where the family has no surroundings."""
    def carve(fn, shape):
        buf = pattern(shape, t.dtype, t.device, seed)
        mask = torch.zeros(shape, dtype=torch.bool, device=t.device)
        v = fn(buf)
        v.copy_(t)
        fn(mask).fill_(True)
        return v, buf, mask

    if family == "dense":
        return (nhwc(t) if t.dim() == 4 else t.contiguous().clone()), None, None
    if t.dim() == 2:
        rows, C = t.shape
        if family == "rowstride":          # row stride C + ge, column offset ge
            return carve(lambda b: b[:, ge:], (rows, C + ge))
        if family == "col+1":              # REFUSED: a column slice whose base is 1 element off
            return carve(lambda b: b[:, 1:1 + C], (rows, C + ge))
        if family == "colstride":          # REFUSED: column stride != 1
            return t.t().contiguous().t(), None, None
        raise KeyError(family)
    B, C, H, W = t.shape
    Cp = -(-C // ge) * ge
    ld = 2 * Cp + 2 * ge
    offs = {"slice@0": 0, "slice@ge": ge, "slice@C+ge": Cp + ge, "unaligned": 1, "off+1": 1, "off+ge/2": ge // 2}
    if family in offs:                     # ("unaligned" is legal for inputs: conversion path; "off+1" / "off+ge/2" name the REFUSED output views)
        o = offs[family]
        return carve(lambda b: b.permute(0, 3, 1, 2)[:, o:o + C], (B, H, W, ld))
    if family == "batch":                  # images [1:3] of a four-image buffer
        assert B == 2
        return carve(lambda b: b.permute(0, 3, 1, 2)[1:3], (4, H, W, C))
    if family == "nchw":
        return t.contiguous().clone(), None, None
    if family == "channels_last":
        return t.contiguous().clone().contiguous(memory_format=torch.channels_last), None, None
    raise KeyError(family)


@dataclass
class Entry:
    name: str
    wrapper: str                      # the public function of ops this entry calls
    dtypes: tuple
    build: Callable                   # (ops, dtype, dev) -> dict of dense operands
    call: Callable                    # (ops, o) -> the wrapper's return value
    args: dict                        # tensor argument -> Arg
    entry_point: str                  # the library function an accepted call ends in
    packed: tuple = ()                # operands that are PackedConv weights (a pack in another dtype is refused)
    overlap: tuple = ()               # (input, output): an output sharing elements with the input is refused, a disjoint slice of one buffer legal
    extra_refused: Callable = None    # (ops, dtype, o) -> [(id, {operand: value}, exception)]
    extra_accepted: Callable = None   # (ops, dtype, o) -> [(id, {operand: value}, [(buffer, mask)])]
    aliases: dict = field(default_factory=dict)      # operand -> the operand it IS in the dense call (linear's in-place stream)


def arg_ge(a, t):
    return 8 if a.ge8 and a.kind == "rows" else granule(t.dtype)


def accepted_cases(e, ops, dtype, o):
    """[(id, operand overrides, [(buffer, mask)])] of every accepted view of every argument."""
    cases = []
    for name, a in e.args.items():
        if name in e.aliases:
            continue
        for fam in a.accepted():
            v, buf, mask = embed(o[name], fam, arg_ge(a, o[name]))
            over = {name: v}
            over.update({k: v for k, tgt in e.aliases.items() if tgt == name})
            cases.append((f"{name}:{fam}", over, [(buf, mask)] if buf is not None else []))
    if e.overlap:
        xi, yo = e.overlap
        x, y = o[xi], o[yo]
        if x.dtype == y.dtype:            # input and output as DISJOINT slices of one buffer
            ge = 8
            if x.dim() == 4 and x.shape[0] == y.shape[0] and x.shape[2:] == y.shape[2:]:
                B, C, H, W = x.shape
                N = y.shape[1]
                buf = pattern((B, H, W, C + N + ge), dtype, x.device)
                full = buf.permute(0, 3, 1, 2)
                vx, vy = full[:, :C], full[:, C + ge:]
            elif x.dim() == 2:
                rows, C = x.shape
                N = y.shape[1]
                buf = pattern((rows, C + N + ge), dtype, x.device)
                vx, vy = buf[:, :C], buf[:, C + ge:]
            else:
                vx = None
            if vx is not None:
                vx.copy_(x)
                mask = torch.zeros(buf.shape, dtype=torch.bool, device=x.device)
                (mask.permute(0, 3, 1, 2) if x.dim() == 4 else mask)[:, :C] = True       # the input is checked with the inputs
                (mask.permute(0, 3, 1, 2) if x.dim() == 4 else mask)[:, C + ge:] = True
                over = {xi: vx, yo: vy}
                over.update({k: vy for k, tgt in e.aliases.items() if tgt == yo})
                cases.append((f"{xi}+{yo}:one-buffer-disjoint", over, [(buf, mask)]))
    if e.extra_accepted:
        cases += e.extra_accepted(ops, dtype, o)
    return cases


def refused_cases(e, ops, dtype, o):
    """[(id, operand overrides, exception type)]: the generic cases of every argument's kind and role, then the entry's own."""
    cases = []
    primary = next(iter(e.args))
    for name, a in e.args.items():
        if name in e.aliases:
            continue
        t = o[name]
        ge = arg_ge(a, t)

        def case(what, value, exc, name=name):
            over = {name: value}
            over.update({k: value for k, tgt in e.aliases.items() if tgt == name})
            cases.append((f"{name}:{what}", over, exc))

        if name != primary:
            case("device", on_meta(t), RuntimeError)
        if a.kind == "nhwc" and a.role != "in":
            case("off+1", embed(t, "off+1", ge)[0], ValueError)
            case("off+ge/2", embed(t, "off+ge/2", ge)[0], ValueError)
            case("nchw-layout", t.contiguous().clone(), ValueError)
            case("half-the-channels", nhwc(t[:, :t.shape[1] // 2]), ValueError)
            if not a.dtype_free:
                case("dtype", t.to(OTHER[t.dtype]), TypeError)
        elif a.kind == "rows":
            case("col+1", embed(t, "col+1", ge)[0], ValueError)
            case("colstride", embed(t, "colstride", ge)[0], ValueError)
            if name != primary:
                case("fewer-rows", t[:-1].clone(), ValueError)
                case("half-the-columns", t[:, :t.shape[1] // 2].clone(), ValueError)
                if not a.dtype_free:
                    case("dtype", t.to(OTHER[t.dtype]), TypeError)
        elif a.kind == "dense":
            wide = pattern(tuple(t.shape[:-1]) + (2 * t.shape[-1],), t.dtype, t.device)
            case("noncontiguous", wide[..., :t.shape[-1]], ValueError)
            case("off+1", pattern((t.numel() + 8,), t.dtype, t.device)[1:1 + t.numel()].view(t.shape), ValueError)
            if not a.dtype_free:
                case("dtype", t.to(OTHER[t.dtype]), TypeError)
        elif a.kind == "aux":
            case("dtype", t.to(torch.float16), TypeError)
            case("length", torch.cat([t.reshape(-1), t.reshape(-1)[:4]]), ValueError)
            case("noncontiguous", torch.stack([t, t], -1)[..., 0], ValueError)
    for p in e.packed:
        cases.append((f"{p}:dtype", {p: repack(ops, o[p], OTHER[dtype])}, TypeError))
    if e.overlap:
        xi, yo = e.overlap
        x, y = o[xi], o[yo]
        if x.dtype == y.dtype:            # intersecting channel intervals of one buffer
            if x.dim() == 4:
                B, C, H, W = x.shape
                N = y.shape[1]
                full = pattern((B, H, W, C + N + 8), dtype, x.device).permute(0, 3, 1, 2)
                if full.shape[2:] == y.shape[2:]:
                    cases.append((f"{yo}:overlaps-{xi}", {xi: full[:, :C], yo: full[:, 8:8 + N]}, ValueError))
            else:
                rows, C = x.shape
                N = y.shape[1]
                buf = pattern((rows, C + N + 8), dtype, x.device)
                over = {xi: buf[:, :C], yo: buf[:, 8:8 + N]}
                over.update({k: over[yo] for k, tgt in e.aliases.items() if tgt == yo})
                cases.append((f"{yo}:overlaps-{xi}", over, ValueError))
            if x.shape == y.shape:
                cases.append((f"{yo}:is-{xi}", {yo: x}, ValueError))
    if e.extra_refused:
        cases += e.extra_refused(ops, dtype, o)
    return cases


def repack(ops, pk, dtype):
    """The same PackedConv with its weights in another dtype."""
    import dataclasses
    return dataclasses.replace(pk, w=pk.w.to(dtype))


# ------------------------------------------------------------------------------ the stub library
class Reached(Exception):
    """Raised by the stub library in place of a launch."""


class StubLib:
    """Stands in for libcft_hip.so: records the entry point and its arguments, then raises ``Reached``.  Nothing is ever launched: the
    conversion / packing helpers in front of a wrapper's own call return success without doing anything, the two host-side queries
    answer with a constant."""
    HELPERS = {"cft_to_nhwc": 0, "cft_bottleneck_pack_w2": 0}
    QUERIES = {"cft_conv2d_chain_ok": 1, "cft_batchnorm_train_workspace": 256}

    def __init__(self, names):
        self._names = names
        self.calls = []          # (entry point, args) of everything that would have launched

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._names:
            raise AttributeError(name)

        def fn(*args):
            if name in self.QUERIES:
                return self.QUERIES[name]
            self.calls.append((name, args))
            if name in self.HELPERS:
                return self.HELPERS[name]
            raise Reached(name)
        return fn


def install_stub(monkeypatch, host):
    """Put a StubLib in place of the library for the wrappers; ``host``: also let CPU tensors through the device checks."""
    import msod_amd  # noqa: F401
    from msod_amd import _lib, ops
    stub = StubLib(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "load", lambda: stub)
    if host:
        monkeypatch.setattr(ops, "_require_cuda", lambda t, what: None)
        monkeypatch.setattr(ops, "_is_cuda", lambda t: True, raising=False)
        monkeypatch.setattr(ops, "_stream", lambda: 0)
    return stub


def tensors_of(o):
    return {k: v for k, v in o.items() if isinstance(v, torch.Tensor)}


# ------------------------------------------------------------------------------ the table
def _conv_entry(name, B, H, W, k):
    def build(ops, dtype, dev):
        C = 64
        w = rnd((C, C, k, k), 2, scale=1.0 / math.sqrt(C * k * k))
        pk = ops.pack_conv(w, rnd((C,), 3, scale=0.5), dtype, s=1, device=dev)
        return dict(x=nhwc(rnd((B, C, H, W), 1, dtype, dev)), pk=pk, residual=nhwc(rnd((B, C, H, W), 4, dtype, dev)),
                    out=nhwc(pattern((B, C, H, W), dtype, dev, 5)))

    full = B == 2 and H > 1 and W > 1

    def free_strides(ops, dtype, o):
        x = o["x"]
        free = torch.empty_strided(tuple(x.shape), tuple(s * 3 if n == 1 else s for n, s in zip(x.shape, x.stride())), dtype=x.dtype, device=x.device)
        free.copy_(x)
        return [("x:free-strides-on-size-1-dims", {"x": free}, [])]

    return Entry(name, "conv2d", DTYPES, build, lambda ops, o: ops.conv2d(o["x"], o["pk"], 1, residual=o["residual"], out=o["out"]),
                 dict(x=Arg("nhwc", "in", ("ldx",), families=None if full else CONVERTED[:2]),
                      residual=Arg("nhwc", "nocopy", ("ldr",), ge8=True, families=None if full else ()),
                      out=Arg("nhwc", "out", ("ldy",), ge8=True, families=None if full else ())),
                 "cft_conv2d", packed=("pk",), overlap=("x", "out") if full else (), extra_accepted=None if full else free_strides)


def _conv_f32out_build(ops, dtype, dev):
    C = 64
    pk = ops.pack_conv(rnd((C, C, 1, 1), 2, scale=0.125), rnd((C,), 3, scale=0.5), dtype, device=dev)
    return dict(x=nhwc(rnd((2, C, 5, 7), 1, dtype, dev)), pk=pk, out=nhwc(pattern((2, C, 5, 7), torch.float32, dev, 5)))


def _chain_build(ops, dtype, dev):
    pk1 = ops.pack_conv(rnd((128, 64, 3, 3), 2, scale=1 / 24.0), rnd((128,), 3, scale=0.5), dtype, s=2, device=dev)
    pk2 = ops.pack_conv(rnd((72, 128, 1, 1), 4, scale=1 / 11.0), rnd((72,), 5, scale=0.5), dtype, device=dev)
    return dict(x=nhwc(rnd((2, 64, 13, 13), 1, dtype, dev)), pk1=pk1, pk2=pk2, out=nhwc(pattern((2, 72, 7, 7), dtype, dev, 6)))


def _chain_res_build(ops, dtype, dev):
    pk1 = ops.pack_conv(rnd((256, 256, 3, 3), 2, scale=1 / 48.0), rnd((256,), 3, scale=0.5), dtype, device=dev)
    pk2 = ops.pack_conv(rnd((256, 256, 1, 1), 4, scale=1 / 16.0), rnd((256,), 5, scale=0.5), dtype, device=dev)
    return dict(x=nhwc(rnd((2, 256, 9, 9), 1, dtype, dev)), pk1=pk1, pk2=pk2, res=nhwc(rnd((2, 256, 9, 9), 6, dtype, dev)),
                out1=nhwc(pattern((2, 256, 9, 9), dtype, dev, 7)), out2=nhwc(pattern((2, 256, 9, 9), dtype, dev, 8)))


def _bottleneck_build(ops, dtype, dev):
    C = 64
    pk1 = ops.pack_conv(rnd((C, C, 1, 1), 2, scale=0.125), rnd((C,), 3, scale=0.5), dtype, device=dev)
    pk2 = ops.pack_conv(rnd((C, C, 3, 3), 4, scale=1 / 24.0), rnd((C,), 5, scale=0.5), dtype, device=dev)
    return dict(x=nhwc(rnd((2, C, 17, 15), 1, dtype, dev)), pk1=pk1, pk2=pk2, out=nhwc(pattern((2, C, 17, 15), dtype, dev, 6)))


ROWS, K_LIN, N_LIN = 37, 64, 72


def _linear_build(ops, dtype, dev):
    pk = ops.pack_conv(rnd((N_LIN, K_LIN), 2, scale=0.125), rnd((N_LIN,), 3, scale=0.1), dtype, device=dev)
    return dict(x=rnd((ROWS, K_LIN), 1, dtype, dev), pk=pk, residual=rnd((ROWS, N_LIN), 4, dtype, dev), out=pattern((ROWS, N_LIN), dtype, dev, 5))


def _linear_stream_build(ops, dtype, dev):
    o = _linear_build(ops, dtype, dev)
    o["residual"] = o["out"] = rnd((ROWS, N_LIN), 4, torch.float32, dev)
    return o


def _linear_refused(ops, dtype, o):
    """A dense [rows, n / 2] ``out``: written with n columns per row it is an out-of-bounds write."""
    return [("out:half-the-columns-dense", {"out": pattern((ROWS, N_LIN // 2), o["out"].dtype, o["x"].device)}, ValueError)]


def _splitk_build(ops, dtype, dev):
    pk = ops.pack_conv(rnd((N_LIN, 128), 2, scale=0.09), rnd((N_LIN,), 3, scale=0.1), dtype, device=dev)
    return dict(x=rnd((ROWS, 128), 1, dtype, dev), pk=pk)


def _ln_build(out_dtype):
    def build(ops, dtype, dev):
        return dict(x=rnd((ROWS, 64), 1, torch.float32, dev) * 3 + 1, gamma=rnd((64,), 2, dev=dev) * 0.2 + 1, beta=rnd((64,), 3, dev=dev) * 0.1,
                    out_dtype=dtype)
    return build


def _ln_refused(ops, dtype, o):
    x = o["x"]
    wide = pattern((ROWS, 2 * 64 + 8), torch.float32, x.device)
    return [("x:column-slice-of-a-wider-buffer", {"x": wide[:, :64]}, ValueError),
            ("x:bf16-read-as-fp32", {"x": x.to(torch.bfloat16)}, TypeError),
            ("x:three-dims", {"x": x.view(1, ROWS, 64)}, ValueError)]


def _lnr_build(ops, dtype, dev):
    o = _ln_build(None)(ops, dtype, dev)
    o["parts"] = rnd((2, ROWS, 64), 4, torch.float32, dev)
    return o


def _lnr_refused(ops, dtype, o):
    return [("parts:fewer-rows", {"parts": o["parts"][:, :-1].contiguous()}, ValueError)]


def _attention_entry(T):
    B, heads, dk = 2, 2, 32

    def build(ops, dtype, dev):
        return dict(qkv=rnd((B * T, 3 * heads * dk), 1, dtype, dev), T=T)

    def refused(ops, dtype, o):
        q = o["qkv"]
        return [("qkv:fewer-than-B*T-rows", {"qkv": q[:B * T - 8].clone()}, ValueError),
                ("qkv:one-image-only", {"qkv": q[:T].clone()}, ValueError),
                ("qkv:narrower", {"qkv": q[:, :2 * heads * dk].contiguous()}, ValueError)]

    return Entry(f"attention_T{T}", "attention", DTYPES, build, lambda ops, o: ops.attention(o["qkv"], B, heads, dk, dk, T=o["T"]),
                 dict(qkv=Arg("dense", "in", dtype_free=True)), "cft_attention" if T == 128 else "cft_attention_tokens", extra_refused=refused)


def _add_build(ops, dtype, dev):
    return dict(a=nhwc(rnd((2, 64, 5, 7), 1, dtype, dev)), b=nhwc(rnd((2, 64, 5, 7), 2, dtype, dev)), out=nhwc(pattern((2, 64, 5, 7), dtype, dev, 3)))


def _add_accepted(ops, dtype, o):
    a = nhwc(o["a"])
    va, buf, mask = embed(o["a"], "slice@ge", granule(dtype))
    return [("out:is-a", {"a": a, "out": a}, []), ("out:is-a-slice", {"a": va, "out": va}, [(buf, mask)])]


def _add_refused(ops, dtype, o):
    return [("b:dtype", {"b": o["b"].to(OTHER[dtype])}, TypeError), ("b:shape", {"b": nhwc(o["b"][:, :32])}, ValueError)]


def _add_rows_build(ops, dtype, dev):
    return dict(x=rnd((ROWS, 64), 1, dtype, dev), y=rnd((ROWS, 64), 2, dtype, dev))


def _copy_build(ops, dtype, dev):
    return dict(src=nhwc(rnd((2, 64, 5, 7), 1, dtype, dev)), dst=nhwc(pattern((2, 64, 10, 14), dtype, dev, 2)))


def _copy_refused(ops, dtype, o):
    return [("src:dtype", {"src": o["src"].to(OTHER[dtype])}, TypeError), ("src:shape", {"src": nhwc(o["src"][:, :, :4])}, ValueError)]


SPP_C = 32


def _spp_build(ops, dtype, dev):
    buf = nhwc(pattern((2, 4 * SPP_C, 7, 12), dtype, dev, 2))
    buf[:, :SPP_C] = rnd((2, SPP_C, 7, 12), 1, dtype, dev)
    return dict(buf=buf)


def _spp_refused(ops, dtype, o):
    """A view of fewer than 4C channels inside a wider buffer: the kernel would write the neighbouring channels."""
    wide = nhwc(pattern((2, 8 * SPP_C, 7, 12), dtype, o["buf"].device))
    return [("buf:2C-channels-of-a-wider-buffer", {"buf": wide[:, :2 * SPP_C]}, ValueError),
            ("buf:C-channels-of-a-wider-buffer", {"buf": wide[:, :SPP_C]}, ValueError)]


def _token_entries():
    out = []
    for H, W in ((5, 7), (12, 20)):
        C, B, T = 64, 2, 128

        def tok_build(ops, dtype, dev, H=H, W=W):
            return dict(rgb=nhwc(rnd((B, C, H, W), 1, dtype, dev)), ir=nhwc(rnd((B, C, H, W), 2, dtype, dev)), pos_emb=rnd((1, T, C), 3, dev=dev))

        def tok_refused(ops, dtype, o):
            return [("ir:another-shape", {"ir": nhwc(o["ir"][:, :, :-1])}, ValueError), ("ir:dtype", {"ir": o["ir"].to(OTHER[dtype])}, TypeError),
                    ("pos_emb:one-stream-only", {"pos_emb": o["pos_emb"][:, :T // 2].contiguous()}, ValueError)]

        out.append(Entry(f"gpt_tokenize_{H}x{W}", "gpt_tokenize", DTYPES, tok_build, lambda ops, o: ops.gpt_tokenize(o["rgb"], o["ir"], o["pos_emb"]),
                         dict(rgb=Arg("nhwc", "in", ("ld_rgb",)), ir=Arg("nhwc", "in", ("ld_ir",)), pos_emb=Arg("aux")), "cft_gpt_tokenize",
                         extra_refused=tok_refused))

        def up_build(ops, dtype, dev, H=H, W=W):
            return dict(tokens=rnd((B, T, C), 1, dev=dev), base=nhwc(rnd((B, C, H, W), 2, dtype, dev)), base1=nhwc(rnd((B, C, H, W), 3, dtype, dev)),
                        sum_out=nhwc(pattern((B, C, H, W), dtype, dev, 4)), H=H, W=W, dtype=dtype)

        def up_refused(ops, dtype, o):
            """On the 8 x 8 grid too: bf16 tokens, tokens of another grid's length, a base of another dtype / shape."""
            t = o["tokens"]
            return [("tokens:bf16", {"tokens": t.to(torch.bfloat16)}, TypeError), ("tokens:64-of-128", {"tokens": t[:, :64].contiguous()}, ValueError),
                    ("base:dtype", {"base": o["base"].to(OTHER[dtype])}, TypeError), ("base:shape", {"base": nhwc(o["base"][:, :, :-1])}, ValueError)]

        out.append(Entry(f"gpt_upsample_add_{H}x{W}", "gpt_upsample_add", DTYPES, up_build,
                         lambda ops, o: ops.gpt_upsample_add(o["tokens"], 1, o["base"], o["H"], o["W"], o["dtype"]),
                         dict(tokens=Arg("dense"), base=Arg("nhwc", "in", ("ldb",), dtype_free=True)), "cft_gpt_upsample_add", extra_refused=up_refused))
        out.append(Entry(f"gpt_upsample_add_dual_{H}x{W}", "gpt_upsample_add_dual", DTYPES, up_build,
                         lambda ops, o: ops.gpt_upsample_add_dual(o["tokens"], o["base"], o["base1"], o["H"], o["W"], o["dtype"], sum_out=o["sum_out"]),
                         dict(tokens=Arg("dense"), base=Arg("nhwc", "in", ("ldb0",), dtype_free=True), base1=Arg("nhwc", "in", ("ldb1",), dtype_free=True),
                              sum_out=Arg("nhwc", "out", ("lds",))), "cft_gpt_upsample_add2", extra_refused=up_refused))
    return out


def _decode_build(ops, dtype, dev):
    from test_gpu_kernel_oracles import DECODE_CASE as c, decode_operands
    logits, anchors = decode_operands()
    n = c["na"] * c["ny"] * c["nx"]
    return dict(logits=nhwc(logits.to(dev)), raw=pattern((c["B"], c["na"], c["ny"], c["nx"], c["no"]), torch.float32, dev, 2),
                pred=pattern((c["B"], c["row0"] + n + c["tail"], c["no"]), torch.float32, dev, 3), anchors_px=anchors.to(dev), case=c)


def _decode_call(ops, o):
    c = o["case"]
    return ops.detect_decode(o["logits"], o["raw"], o["pred"], o["anchors_px"], c["na"], c["no"], c["stride"], c["row0"])


def _decode_refused(ops, dtype, o):
    c, raw, pred = o["case"], o["raw"], o["pred"]
    n = c["na"] * c["ny"] * c["nx"]
    return [("pred:too-few-rows", {"pred": pred[:, :c["row0"] + n - 1].contiguous()}, ValueError),
            ("pred:one-image", {"pred": pred[:1].contiguous()}, ValueError),
            ("pred:narrower", {"pred": pred[:, :, :-1].contiguous()}, ValueError),
            ("raw:shape", {"raw": raw[:, :, :-1].contiguous()}, ValueError),
            ("raw:flat", {"raw": raw.reshape(c["B"], -1)}, ValueError),
            ("logits:channel-slice", {"logits": embed(o["logits"], "slice@0", 4)[0]}, ValueError),
            ("logits:nchw", {"logits": o["logits"].contiguous()}, ValueError)]


BN_M, BN_C = 70, 20


def _bn_build(ops, dtype, dev):
    B, H, W, Cp = 2, 5, 7, 24
    y32 = torch.zeros(B, Cp, H, W)
    y32[:, :BN_C] = rnd((B, BN_C, H, W), 1) * 2 + 0.5
    bn = torch.nn.BatchNorm2d(BN_C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * rnd((BN_C,), 2))
        bn.bias.copy_(0.2 * rnd((BN_C,), 3))
        bn.running_mean.copy_(rnd((BN_C,), 4))
        bn.running_var.copy_(rnd((BN_C,), 5).abs() + 0.5)
    wide = nhwc(pattern((B, Cp, H, W), dtype, dev, 6))
    rwide = nhwc(pattern((B, Cp, H, W), dtype, dev, 7))
    rwide[:, :BN_C] = rnd((B, BN_C, H, W), 8, dtype, dev)
    return dict(y32=nhwc(y32.to(dev)), bn=bn, residual=rwide[:, :BN_C], out=wide[:, :BN_C], out_full=wide, residual_full=rwide, dtype=dtype,
                weight=bn.weight, bias=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var)


def _bn_accepted(ops, dtype, o):
    """The kernel stores (and reads the shortcut in) whole granules: a C-channel output owns the channels up to pad8(C) behind it, as the
    conv output it normalises does.  So the views are slices of pad8(C) channels, the operand their first C."""
    cases = []
    for name in ("out", "residual"):
        for fam in SLICES + ("batch",):
            v, buf, mask = embed(o[name + "_full"], fam, granule(dtype))
            cases.append((f"{name}:{fam}", {name: v[:, :BN_C]}, [(buf, mask)]))
    return cases


def _bn_refused(ops, dtype, o):
    """The last C channels of a pixel: the padding channels up to pad8(C) would land in the next pixel (a granule-aligned offset with
    that property exists for fp32 only: C = 20 at offset 28 of 48)."""
    if dtype != torch.float32:
        return []
    wide = nhwc(pattern((2, 48, 5, 7), dtype, o["out"].device))
    return [("out:padding-channels-past-the-pixel", {"out": wide[:, 28:]}, ValueError),
            ("residual:padding-channels-past-the-pixel", {"residual": wide[:, 28:]}, ValueError)]


def _bn_call(ops, o):
    import copy
    bn = copy.copy(o["bn"])          # a shallow copy that takes the (possibly replaced) parameters; the statistics update goes to the tensors
    bn._parameters = dict(bn._parameters, weight=o["weight"], bias=o["bias"])
    bn._buffers = dict(bn._buffers, running_mean=o["running_mean"], running_var=o["running_var"])
    return ops.batchnorm_train(o["y32"], BN_C, bn, 1, residual=o["residual"], out=o["out"], out_dtype=o["dtype"])


def _dropout_build(ops, dtype, dev):
    return dict(x=rnd((ROWS, 70), 1, dtype, dev))


def _dropout_call(ops, o):
    ops.manual_dropout_seed(1234)
    return ops.dropout_(o["x"], 0.5)


def _to_nhwc_build(ops, dtype, dev):
    return dict(x=nhwc(rnd((2, 20, 5, 7), 1, dtype, dev)), dtype=dtype)


def _to_nhwc_accepted(ops, dtype, o):
    row = o["x"][:, :, :, :1].contiguous()
    dense = row.expand(-1, -1, -1, 7)
    return [("x:expand-stride-0", {"x": dense, "__dense__": {"x": dense.contiguous()}}, [])]


def _to_nhwc_refused(ops, dtype, o):
    x = o["x"]
    return [("x:float64", {"x": x.double()}, TypeError), ("x:three-dims", {"x": x[0]}, ValueError)]


def _size1_entries():
    """Tensors with size-1 dims, whose strides PyTorch leaves free: B = 1, H = 1, W = 1 (inputs; whatever as_nhwc makes of them)."""
    out = []
    for tag, (B, H, W) in (("b1", (1, 5, 7)), ("h1", (2, 1, 7)), ("w1", (2, 5, 1))):
        out.append(_conv_entry(f"conv2d_k3_{tag}", B, H, W, 3))

        def build(ops, dtype, dev, B=B, H=H, W=W):
            return dict(x=nhwc(rnd((B, 24, H, W), 1, dtype, dev)), dtype=dtype)

        def accepted(ops, dtype, o):
            x = o["x"]
            free = torch.empty_strided(tuple(x.shape), tuple(s * 3 if n == 1 else s for n, s in zip(x.shape, x.stride())), dtype=x.dtype, device=x.device)
            free.copy_(x)
            return [("x:free-strides-on-size-1-dims", {"x": free}, [])]

        out.append(Entry(f"to_nhwc_{tag}", "to_nhwc", DTYPES, build, lambda ops, o: ops.to_nhwc(o["x"], o["dtype"]),
                         dict(x=Arg("nhwc", "in", ("stride_b", "stride_c", "stride_h", "stride_w"), families=CONVERTED[:2])), "cft_to_nhwc",
                         extra_accepted=accepted))

        def add_build(ops, dtype, dev, B=B, H=H, W=W):
            return dict(a=nhwc(rnd((B, 64, H, W), 1, dtype, dev)), b=nhwc(rnd((B, 64, H, W), 2, dtype, dev)), out=nhwc(pattern((B, 64, H, W), dtype, dev, 3)))

        out.append(Entry(f"add_{tag}", "add", DTYPES, add_build, lambda ops, o: ops.add(o["a"], o["b"], out=o["out"]),
                         dict(a=Arg("nhwc", "in", ("lda",), families=CONVERTED[:2]), b=Arg("nhwc", "in", ("ldb",), families=CONVERTED[:2]),
                              out=Arg("nhwc", "out", ("ldo",), families=())), "cft_add"))
    return out


def _focus_build(kind):
    def build(ops, dtype, dev):
        six = (rnd((2, 6, 8, 12), 1).abs().clamp(0, 1) * (255 if kind == "u8" else 1)).to(torch.uint8 if kind == "u8" else torch.float32).to(dev)
        pk = ops.pack_conv(rnd((32, 12, 3, 3), 2, scale=0.1), rnd((32,), 3, scale=0.5), dtype, cin_pad=16, device=dev)
        return dict(img=six[:, 3:].contiguous(), six=six, pk=pk, dtype=dtype)
    return build


def _focus_accepted(ops, dtype, o):
    return [("img:channels-3..5-of-six", {"img": o["six"][:, 3:]}, [])]


def _focus_refused(ops, dtype, o):
    img = o["img"]
    return [("img:four-channels", {"img": o["six"][:, :4]}, ValueError), ("img:odd-height", {"img": img[:, :, :-1]}, ValueError),
            ("img:float64", {"img": img.double()}, TypeError)]


TABLE = [
    _conv_entry("conv2d_k3", 2, 5, 7, 3),
    _conv_entry("conv2d_k1", 2, 5, 7, 1),
    Entry("conv2d_fp32_out", "conv2d", LOWP, _conv_f32out_build, lambda ops, o: ops.conv2d(o["x"], o["pk"], 0, out=o["out"]),
          dict(x=Arg("nhwc", "in", ("ldx",), families=SLICES[:1]), out=Arg("nhwc", "out", ("ldy",), ge8=True, dtype_free=True)), "cft_conv2d"),
    Entry("conv2d_chain", "conv2d_chain", LOWP, _chain_build, lambda ops, o: ops.conv2d_chain(o["x"], o["pk1"], o["pk2"], 1, out=o["out"]),
          dict(x=Arg("nhwc", "in", ("ldx",)), out=Arg("nhwc", "out", ("ldy",), ge8=True)), "cft_conv2d_chain", packed=("pk1", "pk2"),
          overlap=("x", "out")),
    Entry("conv2d_chain_res", "conv2d_chain_res", LOWP, _chain_res_build,
          lambda ops, o: ops.conv2d_chain_res(o["x"], o["pk1"], o["res"], o["pk2"], 1, out1=o["out1"], out2=o["out2"]),
          dict(x=Arg("nhwc", "in", ("ldx",)), res=Arg("nhwc", "nocopy", ("ldr",), ge8=True), out1=Arg("nhwc", "out", ("ldy1",), ge8=True),
               out2=Arg("nhwc", "out", ("ldy2",), ge8=True)), "cft_conv2d_chain_res", packed=("pk1", "pk2"), overlap=("x", "out1")),
    Entry("bottleneck", "bottleneck", LOWP, _bottleneck_build, lambda ops, o: ops.bottleneck(o["x"], o["pk1"], o["pk2"], True, out=o["out"]),
          dict(x=Arg("nhwc", "in", ("ldx",)), out=Arg("nhwc", "out", ("ldy",))), "cft_bottleneck", packed=("pk1", "pk2")),
    Entry("linear", "linear", DTYPES, _linear_build, lambda ops, o: ops.linear(o["x"], o["pk"], 2, residual=o["residual"], out=o["out"]),
          dict(x=Arg("rows", "in", ("ldx",)), residual=Arg("rows", "nocopy", ("ldr",), ge8=True), out=Arg("rows", "out", ("ldy",), ge8=True)),
          "cft_conv2d", packed=("pk",), overlap=("x", "out"), extra_refused=_linear_refused),
    Entry("linear_stream", "linear", DTYPES, _linear_stream_build,
          lambda ops, o: ops.linear(o["x"], o["pk"], 0, residual=o["residual"], out=o["out"], out_dtype=torch.float32),
          dict(x=Arg("rows", "in", ("ldx",)), out=Arg("rows", "inout", ("ldy", "ldr"), ge8=True), residual=Arg("rows", "nocopy", ge8=True)),
          "cft_conv2d", aliases={"residual": "out"}),
    Entry("linear_splitk", "linear_splitk", DTYPES, _splitk_build, lambda ops, o: ops.linear_splitk(o["x"], o["pk"], 2),
          dict(x=Arg("rows", "in", ("ldx",))), "cft_linear_splitk", packed=("pk",)),
    Entry("layernorm", "layernorm", DTYPES, _ln_build(None), lambda ops, o: ops.layernorm(o["x"], o["gamma"], o["beta"], o["out_dtype"]),
          dict(x=Arg("dense"), gamma=Arg("aux"), beta=Arg("aux")), "cft_layernorm", extra_refused=_ln_refused),
    Entry("layernorm_reduce", "layernorm_reduce", DTYPES, _lnr_build,
          lambda ops, o: ops.layernorm_reduce(o["x"], o["parts"], o["gamma"], o["beta"], o["out_dtype"]),
          dict(x=Arg("dense", "inout"), parts=Arg("dense"), gamma=Arg("aux"), beta=Arg("aux")), "cft_layernorm_reduce", extra_refused=_lnr_refused),
    _attention_entry(128),
    _attention_entry(64),
    Entry("add", "add", DTYPES, _add_build, lambda ops, o: ops.add(o["a"], o["b"], out=o["out"]),
          dict(a=Arg("nhwc", "in", ("lda",)), b=Arg("nhwc", "in", ("ldb",)), out=Arg("nhwc", "out", ("ldo",))), "cft_add",
          extra_accepted=_add_accepted, extra_refused=_add_refused),
    Entry("add_rows_", "add_rows_", DTYPES, _add_rows_build, lambda ops, o: ops.add_rows_(o["x"], o["y"]),
          dict(x=Arg("rows", "inout", ("lda", "ldo")), y=Arg("rows", "in", ("ldb",))), "cft_add"),
    Entry("copy_channels", "copy_channels", DTYPES, _copy_build, lambda ops, o: ops.copy_channels(o["src"], o["dst"], 1),
          dict(src=Arg("nhwc", "in", ("ldi",)), dst=Arg("nhwc", "out", ("ldo",))), "cft_copy_channels", extra_refused=_copy_refused),
    Entry("spp_maxpool", "spp_maxpool", DTYPES, _spp_build, lambda ops, o: ops.spp_maxpool(o["buf"], SPP_C, (5, 9, 13)),
          dict(buf=Arg("nhwc", "inout", ("ld",), dtype_free=True)), "cft_spp_maxpool", extra_refused=_spp_refused),
    *_token_entries(),
    Entry("detect_decode", "detect_decode", (torch.float32,), _decode_build, _decode_call,
          dict(logits=Arg("dense", families=()), raw=Arg("dense", "out"), pred=Arg("dense", "inout"), anchors_px=Arg("aux")), "cft_detect_decode",
          extra_refused=_decode_refused),
    Entry("batchnorm_train", "batchnorm_train", DTYPES, _bn_build, _bn_call,
          dict(y32=Arg("nhwc", "nocopy", ("ldx",)), residual=Arg("nhwc", "nocopy", ("ldr",), families=()), out=Arg("nhwc", "out", ("ldy",), families=()),
               weight=Arg("aux"), bias=Arg("aux"), running_mean=Arg("aux", "inout"), running_var=Arg("aux", "inout")), "cft_batchnorm_train",
          extra_accepted=_bn_accepted, extra_refused=_bn_refused),
    Entry("dropout_", "dropout_", DTYPES, _dropout_build, _dropout_call, dict(x=Arg("dense", "inout", dtype_free=True)), "cft_dropout"),
    Entry("to_nhwc", "to_nhwc", DTYPES, _to_nhwc_build, lambda ops, o: ops.to_nhwc(o["x"], o["dtype"]),
          dict(x=Arg("nhwc", "in", ("stride_b", "stride_c", "stride_h", "stride_w"))), "cft_to_nhwc",
          extra_accepted=_to_nhwc_accepted, extra_refused=_to_nhwc_refused),
    *_size1_entries(),
    Entry("focus_s2d", "focus_s2d", DTYPES, _focus_build("f32"), lambda ops, o: ops.focus_s2d(o["img"], o["dtype"]),
          dict(img=Arg("any", ld=("stride_b", "stride_c", "stride_h"))), "cft_focus_s2d", extra_accepted=_focus_accepted, extra_refused=_focus_refused),
    Entry("focus_s2d_u8", "focus_s2d", DTYPES, _focus_build("u8"), lambda ops, o: ops.focus_s2d(o["img"], o["dtype"]),
          dict(img=Arg("any", ld=("stride_b", "stride_c", "stride_h"))), "cft_focus_s2d_u8", extra_accepted=_focus_accepted, extra_refused=lambda ops, dtype, o: _focus_refused(ops, dtype, o)[:2]),
    Entry("focus_conv", "focus_conv", LOWP, _focus_build("f32"), lambda ops, o: ops.focus_conv(o["img"], o["pk"], 1, o["dtype"]),
          dict(img=Arg("any", ld=("stride_b", "stride_c", "stride_h"))), "cft_focus_conv", packed=("pk",), extra_accepted=_focus_accepted, extra_refused=_focus_refused),
    Entry("focus_conv_u8", "focus_conv", LOWP, _focus_build("u8"), lambda ops, o: ops.focus_conv(o["img"], o["pk"], 1, o["dtype"]),
          dict(img=Arg("any", ld=("stride_b", "stride_c", "stride_h"))), "cft_focus_conv", packed=("pk",), extra_accepted=_focus_accepted),
]

# Pointers the library takes at any element alignment (include/cft_hip.h): the converter's strided input, the image of the Focus kernels.
ANY_ALIGNMENT = {"cft_to_nhwc": ("in",), "cft_focus_s2d_u8": ("in",), "cft_focus_conv": ("in",)}

WRAPPERS = ("conv2d", "conv2d_chain", "conv2d_chain_res", "bottleneck", "linear", "linear_splitk", "layernorm", "layernorm_reduce", "attention",
            "add", "add_rows_", "copy_channels", "spp_maxpool", "gpt_tokenize", "gpt_upsample_add", "gpt_upsample_add_dual", "detect_decode",
            "batchnorm_train", "dropout_", "to_nhwc", "focus_s2d", "focus_conv")

CASES = [(e, dt) for e in TABLE for dt in e.dtypes]
CASE_IDS = [f"{e.name}-{DTYPE_IDS[dt]}" for e, dt in CASES]
