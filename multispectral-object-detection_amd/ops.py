"""Thin tensor-level wrappers over the C ABI of libcft_hip.so.

PyTorch is used here only for device memory (``torch.empty``), the current HIP stream and
one-time weight packing; every arithmetic op of the forward is a HIP kernel.  Activations are
torch tensors of logical shape [B,C,H,W] whose memory is NHWC ("channels-last"), possibly a
channel slice of a wider buffer (stride(3) = channels per pixel of the parent).

No CPU path exists: CPU tensors raise.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_SILU, CFT_BF16, CFT_F16, CFT_F32  # noqa: F401


COMPUTE_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _dt(dtype):
    if dtype == torch.bfloat16:
        return CFT_BF16
    if dtype == torch.float16:
        return CFT_F16
    if dtype == torch.float32:
        return CFT_F32
    raise TypeError(f"compute dtype must be torch.bfloat16, torch.float16 or torch.float32, got {dtype}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _is_cuda(t):
    return t.is_cuda


def _require_cuda(t, what):
    if not _is_cuda(t):
        raise RuntimeError(f"{what}: tensor is on {t.device}; this package runs on MI355X only "
                           "(no CPU fallback - use oracle/ for a CPU reference)")


def granule(dtype):
    return 4 if dtype == torch.float32 else 8


def new_nhwc(B, H, W, C, dtype, device):
    """Logical [B,C,H,W] tensor backed by a fresh NHWC buffer."""
    return torch.empty((B, H, W, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


def to_nhwc(x, dtype=None, cpad=None):
    """Any strided [B,C,H,W] fp32/bf16/half tensor -> fresh NHWC buffer in ``dtype`` with the channel count
    padded to ``cpad`` (default: next granule multiple; padding channels zero) - the cft_to_nhwc kernel."""
    _require_cuda(x, "to_nhwc")
    if x.dim() != 4:
        raise ValueError(f"to_nhwc: expected a [B,C,H,W] tensor, got {tuple(x.shape)}")
    B, C, H, W = x.shape
    dtype = dtype or x.dtype
    _dt(x.dtype), _dt(dtype)
    ge = granule(dtype)
    cp = cpad or ((C + ge - 1) // ge) * ge
    if cp < C or cp % ge:
        raise ValueError(f"to_nhwc: cpad {cp} must be a multiple of the {ge}-element granule >= {C} channels")
    y = new_nhwc(B, H, W, cp, dtype, x.device)
    st = _lib.load().cft_to_nhwc(x.data_ptr(), _dt(x.dtype), x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                                 y.data_ptr(), cp, 0, B, C, cp, H, W, _dt(dtype), _stream())
    _lib.check(st, "cft_to_nhwc")
    return y


def as_nhwc(x):
    """Return (x', ld): x' has NHWC memory, ld = channels/pixel.  A tensor in another layout (e.g. a plain NCHW
    tensor handed to a module from outside the network) is converted by the cft_to_nhwc kernel; its channel
    count must already be a granule multiple (the consumer's packed weights fix the channel count)."""
    B, C, H, W = x.shape
    ld = x.stride(3)
    ok = x.stride(1) == 1 and ld >= C and x.stride(2) == W * ld and x.stride(0) == H * W * ld
    ge = granule(x.dtype)
    ok = ok and ld % ge == 0 and x.storage_offset() % ge == 0 and x.data_ptr() % 16 == 0
    if not ok:
        if C % ge:
            raise ValueError(f"as_nhwc: {C} channels is not a multiple of the {ge}-element granule")
        return to_nhwc(x), C
    return x, ld


def _view_ld(x, what):
    """ld of an NHWC view that must NOT be copied (outputs / residuals)."""
    B, C, H, W = x.shape
    ld = x.stride(3)
    if not (x.stride(1) == 1 and ld >= C and x.stride(2) == W * ld and x.stride(0) == H * W * ld):
        raise ValueError(f"{what}: tensor is not an NHWC buffer or a channel slice of one")
    return ld


# ------------------------------------------------------------------------------ argument guards
# Metadata only (shape, stride, dtype, device, data_ptr() % 16): nothing here synchronises, allocates or reads device memory.
# RuntimeError: wrong device; TypeError: wrong dtype; ValueError: shape, stride, alignment or overlap.
def _on(t, ref, what):
    if t.device != ref.device:
        raise RuntimeError(f"{what}: tensor is on {t.device}, expected {ref.device}")


def _is(t, dtype, what):
    if t.dtype != dtype:
        raise TypeError(f"{what}: dtype {t.dtype}, expected {dtype}")


def _packed_for(pk, x, what, dtype=None):
    """The packed weights are in the dtype the kernel computes in (the dtype of ``x``) and on the device of ``x``."""
    _on(pk.w, x, f"{what} packed weight")
    _is(pk.w, dtype or x.dtype, f"{what} packed weight")


def _out_view(t, ref, what, shape=None, ge=None):
    """ld of an NHWC view the kernel writes, adds or updates in place (never copied): on the device of ``ref``, a compute dtype, the
    shape asked for, ld a multiple of the granule (``ge``: 8 for what cft_conv2d and its relatives store, whatever the dtype) and the
    base pointer 16-byte aligned (the kernels store whole granules)."""
    _on(t, ref, what)
    _dt(t.dtype)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    ld = _view_ld(t, what)
    ge = ge or granule(t.dtype)
    if ld % ge or t.data_ptr() % 16:
        raise ValueError(f"{what}: channels per pixel ({ld}) must be a multiple of {ge} and the base pointer 16-byte aligned (a channel "
                         f"slice starts at a granule multiple)")
    return ld


def _rows_ld(t, ref, what, shape=None, ge=None):
    """Row stride of a [rows, C] operand (``linear`` x / out / residual, ``add_rows_``): unit column stride, a row stride that is a granule
    multiple >= C, a 16-byte aligned base."""
    _on(t, ref, what)
    _dt(t.dtype)
    if t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape) if shape is not None else '[rows, C]'}")
    ld = t.stride(0)
    ge = ge or granule(t.dtype)
    if t.stride(1) != 1 or ld < t.shape[1] or ld % ge or t.data_ptr() % 16:
        raise ValueError(f"{what}: needs unit column stride, a row stride (a multiple of {ge}) >= {t.shape[1]} and a 16-byte aligned base, "
                         f"got strides {tuple(t.stride())}")
    return ld


def _vec(t, ref, shape, what, dtype=torch.float32):
    """An auxiliary tensor the kernel reads through a raw pointer (gamma, beta, pos_emb, anchors, BN parameters): dense, ``dtype``, as
    many elements as ``shape`` says, on the device of ``ref``."""
    _on(t, ref, what)
    _is(t, dtype, what)
    n = 1
    for d in shape:
        n *= d
    if t.numel() != n or tuple(t.shape[-len(shape):]) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: must be a contiguous {tuple(shape)} tensor, got {tuple(t.shape)} with strides {tuple(t.stride())}")


def _span(t):
    """[lo, hi) in bytes of the elements a strided view touches."""
    lo = t.data_ptr()
    return lo, lo + (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _disjoint(x, ld_x, cx, out, ld_out, co, what):
    """``out`` (``co`` channels of ``ld_out`` per pixel / row) shares no element with the input ``x`` the kernel reads while other
    workgroups already store: other byte ranges, or two channel intervals of ONE buffer (same ld, same element size) that do not
    intersect.  Anything else cannot be proven disjoint and is refused."""
    (xl, xh), (ol, oh) = _span(x), _span(out)
    if xh <= ol or oh <= xl:
        return
    es = x.element_size()
    d = ol - xl
    if es == out.element_size() and ld_x == ld_out and d % es == 0:
        c = (d // es) % ld_x
        if c >= cx and c + co <= ld_x:
            return
    raise ValueError(f"{what}: out shares elements with the input (only a disjoint channel slice of the same buffer may be written)")


# ------------------------------------------------------------------------------ weight packing
@dataclass
class PackedConv:
    """Weights in the layout cft_conv2d consumes: w[n][kpad] with (kh,kw,ci) flattened, ci
    fastest, zero padded; bias fp32."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    n: int        # rows of w (output channels incl. zero padding to a multiple of 8)
    n_valid: int  # real output channels
    cin: int      # input channels the kernel expects (incl. zero padding)
    kpad: int
    k: int
    s: int
    flops_per_row: float = 0.0   # algorithmic 2*N*K of the unpadded layer (roofline accounting)
    w_stages: Optional[torch.Tensor] = None   # stage-major image of w for cft_bottleneck (128-channel 3x3), built on first use


def fold_bn(weight, bn_weight, bn_bias, running_mean, running_var, eps):
    """Conv+BN(eval) folding, W' = diag(g/sqrt(v+eps)) W, b' = beta - g*mu/sqrt(v+eps)
    (reference utils/torch_utils.py:181-201)."""
    scale = bn_weight.float() / torch.sqrt(running_var.float() + eps)
    return weight.float() * scale.view(-1, 1, 1, 1), bn_bias.float() - running_mean.float() * scale


def pack_conv(weight, bias, dtype, k=None, s=1, cin_pad=None, device=None, n_true=None):
    """weight [N,Cin,kh,kw] (or [N,K] for a Linear) fp32 -> PackedConv in ``dtype``.
    ``n_true``: number of non-padding rows when the caller already padded N (padded heads)."""
    if weight.dim() == 2:
        weight = weight.view(weight.shape[0], weight.shape[1], 1, 1)
    N, Cin, kh, kw = weight.shape
    assert kh == kw, "square kernels only"
    device = device or weight.device
    ge = granule(dtype)
    cin_p = cin_pad or ((Cin + ge - 1) // ge) * ge
    n_p = ((N + 7) // 8) * 8
    bk = 8 * ge
    K = kh * kw * cin_p
    kpad = ((K + bk - 1) // bk) * bk
    w = torch.zeros((n_p, kh, kw, cin_p), dtype=torch.float32, device=device)
    w[:N, :, :, :Cin] = weight.detach().to(device=device, dtype=torch.float32).permute(0, 2, 3, 1)
    wp = torch.zeros((n_p, kpad), dtype=dtype, device=device)
    wp[:, :K] = w.view(n_p, K).to(dtype)
    b = None
    if bias is not None:
        b = torch.zeros((n_p,), dtype=torch.float32, device=device)
        b[:N] = bias.detach().to(device=device, dtype=torch.float32)
    return PackedConv(wp.contiguous(), b, n_p, N, cin_p, kpad, kh, s, 2.0 * (n_true or N) * kh * kw * Cin)


# ------------------------------------------------------------------------------ launch timing
# When a list is installed here every GEMM launch is bracketed by HIP events recorded on the launch
# stream (bench.py uses it to time the dominant kernel family live): entries are
# (tile_family, algorithmic_flops, start_event, end_event, algorithmic_bytes).  The callers build the label and the byte count whether
# or not a log is installed (a few integer products and one f-string per launch; graph replay never comes here).
_launch_log = None


def set_launch_log(log):
    global _launch_log
    _launch_log = log


def _timed(name, flops, abytes, fn):
    """Run ``fn()`` (one kernel launch); when a launch log is installed bracket it with HIP events."""
    if _launch_log is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    st = fn()
    e1.record()
    _launch_log.append((name, flops, e0, e1, abytes))
    return st


def conv_out_size(H, W, k, s):
    """(Ho, Wo) of a k x k convolution with stride s and padding k // 2 on an H x W input."""
    p = k // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _bias_ptr(pk):
    return None if pk.bias is None else pk.bias.data_ptr()


# ------------------------------------------------------------------------------ ops
def conv2d(x, pk, act, residual=None, out=None, out_dtype=None):
    """act(conv(x) + bias) (+ residual) as one implicit-GEMM kernel; see cft_conv2d."""
    _require_cuda(x, "conv2d")
    _dt(x.dtype)
    _packed_for(pk, x, "conv2d")
    x, ldx = as_nhwc(x)
    B, C, H, W = x.shape
    if C != pk.cin:
        raise ValueError(f"conv2d: input has {C} channels, packed weight expects {pk.cin}")
    Ho, Wo = conv_out_size(H, W, pk.k, pk.s)
    if out is None:
        out = new_nhwc(B, Ho, Wo, pk.n, out_dtype or x.dtype, x.device)
        ldy = pk.n
    else:
        if out.dtype != (out_dtype or out.dtype) or out.dtype not in (x.dtype, torch.float32):
            raise TypeError(f"conv2d: out is {out.dtype}, expected {out_dtype or x.dtype} (the compute dtype or float32)")
        ldy = _out_view(out, x, "conv2d out", (B, pk.n, Ho, Wo), 8)
        _disjoint(x, ldx, C, out, ldy, pk.n, "conv2d")
    rp, ldr, rdt = None, 0, CFT_BF16
    if residual is not None:
        if residual.dtype not in (x.dtype, torch.float32):
            raise TypeError(f"conv2d: residual is {residual.dtype}, expected the compute dtype {x.dtype} or float32")
        ldr = _out_view(residual, x, "conv2d residual", out.shape, 8)
        rp, rdt = residual.data_ptr(), _dt(residual.dtype)
    lib = _lib.load()
    es_in, es_out = x.element_size(), out.element_size()
    abytes = (B * H * W * pk.cin * es_in + B * Ho * Wo * pk.n_valid * es_out + pk.w.numel() * es_in
              + (0 if residual is None else residual.numel() * residual.element_size()))
    st = _timed(f"conv_k{pk.k}s{pk.s}_n{pk.n}_K{pk.kpad}", B * Ho * Wo * pk.flops_per_row, abytes,
                lambda: lib.cft_conv2d(x.data_ptr(), pk.w.data_ptr(), _bias_ptr(pk), rp, out.data_ptr(), B, H, W, pk.cin, ldx, 0,
                                       pk.n, pk.kpad, pk.k, pk.s, ldy, 0, ldr, 0, act, _dt(x.dtype), _dt(out.dtype), rdt, _stream()))
    _lib.check(st, "cft_conv2d")
    return out


def conv2d_chain_ok_geometry(B, H, W, dtype, pk1, pk2, ldx=None, ldy=None):
    """``conv2d_chain_ok`` from the input geometry alone ([B, pk1.cin, H, W] of ``dtype`` on the GPU).  ``ldx`` / ``ldy``: channels per
    pixel of the buffers the input / output are slices of (default: dense) - the launcher's 2^31-element limits are on THOSE extents, so
    'ok' here means the launcher accepts."""
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    if pk2.k != 1 or pk2.s != 1 or pk2.cin != pk1.n or pk2.kpad != pk1.n or pk1.n_valid != pk1.n:
        return False
    return bool(_lib.load().cft_conv2d_chain_ok(B, H, W, pk1.cin, ldx or pk1.cin, pk1.n, pk1.kpad, pk1.k, pk1.s, pk2.n, ldy or pk2.n, _dt(dtype)))


def _chain_geometry(x, pk1):
    """(B, H, W, dtype, ldx) of ``x`` for the ``_geometry`` predicates, or None when ``x`` is not a 4-D GPU tensor of ``pk1.cin`` channels."""
    if not (isinstance(x, torch.Tensor) and _is_cuda(x) and x.dim() == 4 and x.shape[1] == pk1.cin):
        return None
    ldx = x.stride(3) if (x.stride(1) == 1 and x.stride(3) >= x.shape[1]) else None      # (another layout is converted to dense NHWC first)
    return x.shape[0], x.shape[2], x.shape[3], x.dtype, ldx


def conv2d_chain_ok(x, pk1, pk2):
    """True when ``conv2d_chain`` takes this pair: conv ``pk1`` (SiLU) then the pointwise conv ``pk2`` on its output (cft_conv2d_chain_ok)."""
    g = _chain_geometry(x, pk1)
    return g is not None and conv2d_chain_ok_geometry(*g[:4], pk1, pk2, ldx=g[4])


def conv2d_chain(x, pk1, pk2, act2, out=None):
    """act2(conv1x1(SiLU(conv(x)))) as ONE kernel (cft_conv2d_chain): the first conv's output tile becomes the second GEMM's A operand
    in LDS.  Bit-identical to ``conv2d(conv2d(x, pk1, ACT_SILU), pk2, act2)``."""
    _require_cuda(x, "conv2d_chain")
    for pk in (pk1, pk2):
        _packed_for(pk, x, "conv2d_chain")
    if not conv2d_chain_ok(x, pk1, pk2):
        raise ValueError("conv2d_chain: layer pair not eligible (conv2d_chain_ok)")
    x, ldx = as_nhwc(x)
    B, C, H, W = x.shape
    Ho, Wo = conv_out_size(H, W, pk1.k, pk1.s)
    if out is None:
        out = new_nhwc(B, Ho, Wo, pk2.n, x.dtype, x.device)
        ldy = pk2.n
    else:
        _is(out, x.dtype, "conv2d_chain out")
        ldy = _out_view(out, x, "conv2d_chain out", (B, pk2.n, Ho, Wo), 8)
        _disjoint(x, ldx, C, out, ldy, pk2.n, "conv2d_chain")
    lib = _lib.load()
    es = x.element_size()
    M = B * Ho * Wo
    abytes = B * H * W * pk1.cin * es + M * pk2.n_valid * es + (pk1.w.numel() + pk2.w.numel()) * es
    args = (x.data_ptr(), pk1.w.data_ptr(), _bias_ptr(pk1), pk2.w.data_ptr(), _bias_ptr(pk2), out.data_ptr(),
            B, H, W, pk1.cin, ldx, 0, pk1.n, pk1.kpad, pk1.k, pk1.s, pk2.n, ldy, 0, act2, _dt(x.dtype), _stream())
    # counted with the GEMM family: both layers' FLOPs, one launch
    st = _timed(f"conv_chain_k{pk1.k}s{pk1.s}_n{pk1.n}_K{pk1.kpad}+{pk2.kpad}", M * (pk1.flops_per_row + pk2.flops_per_row), abytes,
                lambda: lib.cft_conv2d_chain(*args))
    _lib.check(st, "cft_conv2d_chain")
    return out


CHAIN_RES_MIN_ROWS = 192 * 256      # output pixels from which the chained kernel's 256-row tiles fill >= 3/4 of the 256 CUs


def conv2d_chain_res_ok_geometry(B, H, W, dtype, pk1, pk2, any_size=False, ldx=None):
    """True when ``conv2d_chain_res`` takes the pair on a [B, pk1.cin, H, W] input of ``dtype``: ``conv2d_chain_ok_geometry``, a 256-channel
    first layer (the four-image form of the kernel) and - unless ``any_size`` - enough output pixels: the chained kernel exists in the
    256 x 256 tile only, and below ~49 000 pixels (cfg3: < 32 pairs at 640 x 640) the separate launches run on smaller tiles with 4 - 8 x
    the workgroups (measured at 8 pairs: 71 against ~33 us per pair of launches, profiles/r05_splitk_ab.md).  ``ldx`` as in
    ``conv2d_chain_ok_geometry``; by default input and outputs are DENSE (what ``C3.forward`` passes: the hidden tensor and y1 are dense;
    the shortcut's own row stride is checked at launch)."""
    if not (pk1.n == 256 and conv2d_chain_ok_geometry(B, H, W, dtype, pk1, pk2, ldx=ldx)):
        return False
    Ho, Wo = conv_out_size(H, W, pk1.k, pk1.s)
    return any_size or B * Ho * Wo >= CHAIN_RES_MIN_ROWS


def conv2d_chain_res_ok(x, pk1, pk2, any_size=False):
    """``conv2d_chain_res_ok_geometry`` of the GPU tensor ``x`` (False for anything else)."""
    g = _chain_geometry(x, pk1)
    return g is not None and conv2d_chain_res_ok_geometry(*g[:4], pk1, pk2, any_size=any_size, ldx=g[4])


def conv2d_chain_res(x, pk1, res, pk2, act2, out1=None, out2=None):
    """(y1, y2) = (SiLU(conv(x)) + res, act2(conv1x1(y1))) as ONE kernel (cft_conv2d_chain_res): Bottleneck j's 3x3 conv with its shortcut
    and Bottleneck j+1's 1x1 conv inside a C3 with shortcuts.  Bit-identical to ``conv2d(x, pk1, SILU, residual=res)`` followed by
    ``conv2d(y1, pk2, act2)``; y1 is stored but never re-read, and the 1x1 launch disappears."""
    _require_cuda(x, "conv2d_chain_res")
    for pk in (pk1, pk2):
        _packed_for(pk, x, "conv2d_chain_res")
    if not conv2d_chain_res_ok(x, pk1, pk2, any_size=True):
        raise ValueError("conv2d_chain_res: layer pair not eligible (conv2d_chain_res_ok)")
    x, ldx = as_nhwc(x)
    B, C, H, W = x.shape
    Ho, Wo = conv_out_size(H, W, pk1.k, pk1.s)
    _is(res, x.dtype, "conv2d_chain_res residual")
    ldr = _out_view(res, x, "conv2d_chain_res residual", (B, pk1.n, Ho, Wo))
    if out1 is None:
        out1 = new_nhwc(B, Ho, Wo, pk1.n, x.dtype, x.device)
    if out2 is None:
        out2 = new_nhwc(B, Ho, Wo, pk2.n, x.dtype, x.device)
    for o in (out1, out2):
        _is(o, x.dtype, "conv2d_chain_res out")
    ldy1 = _out_view(out1, x, "conv2d_chain_res out1", (B, pk1.n, Ho, Wo))
    ldy2 = _out_view(out2, x, "conv2d_chain_res out2", (B, pk2.n, Ho, Wo))
    _disjoint(x, ldx, C, out1, ldy1, pk1.n, "conv2d_chain_res out1")
    _disjoint(x, ldx, C, out2, ldy2, pk2.n, "conv2d_chain_res out2")
    lib = _lib.load()
    es = x.element_size()
    M = B * Ho * Wo
    abytes = (B * H * W * pk1.cin + 2 * M * pk1.n_valid + M * pk2.n_valid + pk1.w.numel() + pk2.w.numel()) * es
    args = (x.data_ptr(), pk1.w.data_ptr(), _bias_ptr(pk1), res.data_ptr(), out1.data_ptr(), pk2.w.data_ptr(), _bias_ptr(pk2), out2.data_ptr(),
            B, H, W, pk1.cin, ldx, 0, pk1.n, pk1.kpad, pk1.k, pk1.s, ldr, 0, ldy1, 0, pk2.n, ldy2, 0, act2, _dt(x.dtype), _stream())
    st = _timed(f"conv_chainres_k{pk1.k}s{pk1.s}_n{pk1.n}_K{pk1.kpad}+{pk2.kpad}", M * (pk1.flops_per_row + pk2.flops_per_row), abytes,
                lambda: lib.cft_conv2d_chain_res(*args))
    _lib.check(st, "cft_conv2d_chain_res")
    return out1, out2


# cft_bottleneck covers 64 and 128 channels (activation patch resident in LDS, weights streamed through a 4-slot LDS ring, two
# workgroups per CU: 147-173 vs 220-234 us for the two launches it replaces at 128 channels - profiles/r02_bottleneck128.md).
FUSED_BOTTLENECK_WIDTHS = (64, 128)


def bottleneck_fusable(x, pk1, pk2, act1, act2):
    """True when ``bottleneck`` below can run as the single cft_bottleneck kernel."""
    return bottleneck_kernel_covers(x, pk1, pk2, act1, act2) and x.shape[1] in FUSED_BOTTLENECK_WIDTHS


def bottleneck_kernel_covers(x, pk1, pk2, act1, act2):
    """True when cft_bottleneck implements this Bottleneck at all (64 or 128 channels, 16-bit, SiLU)."""
    return (x.dtype in (torch.bfloat16, torch.float16) and act1 == ACT_SILU and act2 == ACT_SILU
            and pk1.k == 1 and pk1.s == 1 and pk2.k == 3 and pk2.s == 1
            and pk1.cin == pk1.n == pk2.cin == pk2.n == x.shape[1] and x.shape[1] in (64, 128))


def bottleneck(x, pk1, pk2, shortcut, out=None):
    """x (+) SiLU(conv3x3(SiLU(conv1x1(x)))) for 64 / 128 channels in one kernel (cft_bottleneck); ``out`` must not
    overlap ``x`` (a disjoint channel slice of the same buffer is fine)."""
    _require_cuda(x, "bottleneck")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"bottleneck: the fused kernel computes in bfloat16 or float16, got {x.dtype}")
    for pk in (pk1, pk2):
        _packed_for(pk, x, "bottleneck")
    x, ldx = as_nhwc(x)
    B, C, H, W = x.shape
    if out is None:
        out = new_nhwc(B, H, W, C, x.dtype, x.device)
    _is(out, x.dtype, "bottleneck out")
    ldy = _out_view(out, x, "bottleneck out", (B, C, H, W))
    lib = _lib.load()
    if C == 128 and pk2.w_stages is None:   # one-time: the 3x3 weights as 36 contiguous 8-KiB stage images (cft_bottleneck_pack_w2)
        pk2.w_stages = torch.empty_like(pk2.w)
        _lib.check(lib.cft_bottleneck_pack_w2(pk2.w.data_ptr(), pk2.kpad, C, pk2.w_stages.data_ptr(), _dt(x.dtype), _stream()),
                   "cft_bottleneck_pack_w2")
    args = (x.data_ptr(), ldx, 0, pk1.w.data_ptr(), pk1.kpad, _bias_ptr(pk1),
            pk2.w.data_ptr(), pk2.kpad, None if pk2.w_stages is None else pk2.w_stages.data_ptr(), _bias_ptr(pk2),
            out.data_ptr(), ldy, 0, B, H, W, C, 1 if shortcut else 0, _dt(x.dtype), _stream())
    rows = B * H * W
    abytes = rows * C * 2 * (3 if shortcut else 2) + (pk1.w.numel() + pk2.w.numel()) * 2
    # counted with the GEMM family: both convolutions' FLOPs, one launch
    st = _timed(f"conv_bneck_c{C}_K{pk1.kpad}+{pk2.kpad}", rows * (pk1.flops_per_row + pk2.flops_per_row), abytes,
                lambda: lib.cft_bottleneck(*args))
    _lib.check(st, "cft_bottleneck")
    return out


def linear(x, pk, act=ACT_NONE, residual=None, out=None, out_dtype=None):
    """x [rows, K] (row stride >= K) -> [rows, pk.n]; nn.Linear(+bias)(+act)(+residual)."""
    _require_cuda(x, "linear")
    _dt(x.dtype)
    _packed_for(pk, x, "linear")
    ldx = _rows_ld(x, x, "linear input")
    rows, K = x.shape
    if K != pk.cin:
        raise ValueError(f"linear: input [{rows},{K}] does not match packed weight (cin {pk.cin})")
    if out is None:
        out = torch.empty((rows, pk.n), dtype=out_dtype or x.dtype, device=x.device)
        ldy = pk.n
    else:
        if out.dtype != (out_dtype or out.dtype) or out.dtype not in (x.dtype, torch.float32):
            raise TypeError(f"linear: out is {out.dtype}, expected {out_dtype or x.dtype} (the compute dtype or float32)")
        ldy = _rows_ld(out, x, "linear out", (rows, pk.n), 8)
        _disjoint(x, ldx, K, out, ldy, pk.n, "linear")
    rp, ldr, rdt = None, 0, CFT_BF16
    if residual is not None:
        if residual.dtype not in (x.dtype, torch.float32):
            raise TypeError(f"linear: residual is {residual.dtype}, expected the compute dtype {x.dtype} or float32")
        ldr = _rows_ld(residual, x, "linear residual", (rows, pk.n), 8)
        rp, rdt = residual.data_ptr(), _dt(residual.dtype)
    lib = _lib.load()
    abytes = (rows * K * x.element_size() + rows * pk.n_valid * out.element_size() + pk.w.numel() * x.element_size()
              + (0 if residual is None else rows * pk.n_valid * residual.element_size()))
    st = _timed(f"linear_k{pk.k}s{pk.s}_n{pk.n}_K{pk.kpad}", rows * pk.flops_per_row, abytes,
                lambda: lib.cft_conv2d(x.data_ptr(), pk.w.data_ptr(), _bias_ptr(pk), rp, out.data_ptr(), 1, 1, rows, pk.cin, x.stride(0), 0,
                                       pk.n, pk.kpad, 1, 1, out.stride(0), 0, ldr, 0, act, _dt(x.dtype), _dt(out.dtype), rdt, _stream()))
    _lib.check(st, "cft_conv2d(linear)")
    return out


SPLITK_MAX_ROWS = 1024      # token rows (B * 128) up to which split-K pays with two forwards in flight: <= 8 pairs per GPU.  At 2 048 rows it still buys
                            # +4.8 % with ONE forward in flight (latency) but costs 0.6 - 2.6 % of the throughput with two (profiles/r05_splitk_ab.md): a
                            # latency-bound deployment raises this constant


def splitk_choice(rows, pk, dtype):
    """Number of K splits for ``linear_splitk`` (1 = run ``linear``): GEMMs whose 256 x 256 tiles would leave most of the 256 CUs idle and
    whose K loop is long enough to cut (the CFT block's out_proj / fc2 at B * 128 rows) - the smallest of 2 / 4 / 8 that yields >= 128
    workgroups, each split keeping >= 4 K steps."""
    bk = 32 if dtype == torch.float32 else 64
    if pk.k != 1 or pk.kpad != pk.cin or pk.cin % bk or 2 * pk.kpad * (4 if dtype == torch.float32 else 2) + 128 > 65536:
        return 1
    steps = pk.kpad // bk
    t256 = -(-rows // 256) * -(-pk.n // 256)
    # Measured (profiles/r05_splitk_ab.md): at 8192 rows (64 pairs) the split GEMMs gain 0.31 ms per forward and the LayerNorms that fold
    # 2-4 x [rows, d] fp32 partial sums lose 0.50 ms (HBM bytes); at 1024 rows (8 pairs) everything is latency-bound and the CFT block drops
    # from 2.37 to 1.84 ms.  So: only where the un-split GEMM leaves >= 3/4 of the chip idle, and only for small row counts (SPLITK_MAX_ROWS).
    if t256 >= 64 or rows > SPLITK_MAX_ROWS:
        return 1
    best = 1
    for s in (2, 4, 8):
        if steps % s or steps // s < 4 or s * rows * pk.n >= 2 ** 31:
            break
        best = s
        if t256 * s >= 128:      # half the CUs busy is enough: every further split doubles the partial sums the LayerNorm has to fold
            break
    return best


def linear_splitk(x, pk, splits):
    """fp32 partial sums [splits, rows, pk.n] of ``x @ w.T (+ bias)`` over ``splits`` slices of K (cft_linear_splitk); summed in order they equal
    ``linear(x, pk, out_dtype=float32)`` up to fp32 rounding.  ``layernorm_reduce`` folds them into the residual stream."""
    _require_cuda(x, "linear_splitk")
    _dt(x.dtype)
    _packed_for(pk, x, "linear_splitk")
    _rows_ld(x, x, "linear_splitk input")
    rows, K = x.shape
    if K != pk.cin:
        raise ValueError(f"linear_splitk: input [{rows},{K}] does not match packed weight (cin {pk.cin})")
    if not 2 <= int(splits) <= 8:
        raise ValueError(f"linear_splitk: splits must be 2 .. 8, got {splits}")
    parts = torch.empty((splits, rows, pk.n), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    abytes = rows * K * x.element_size() + splits * rows * pk.n_valid * 4 + pk.w.numel() * x.element_size()
    st = _timed(f"linear_k{pk.k}s{pk.s}_n{pk.n}_K{pk.kpad}", rows * pk.flops_per_row, abytes,
                lambda: lib.cft_linear_splitk(x.data_ptr(), pk.w.data_ptr(), _bias_ptr(pk), parts.data_ptr(),
                                              rows, pk.cin, x.stride(0), pk.n, pk.kpad, splits, _dt(x.dtype), _stream()))
    _lib.check(st, "cft_linear_splitk")
    return parts


def layernorm_reduce(x, parts, gamma, beta, out_dtype, eps=1e-5):
    """x (float32 [rows, C], IN PLACE) += parts[0] + parts[1] + ... (float32 [n, rows, C]); returns LayerNorm(x) in ``out_dtype``."""
    _require_cuda(x, "layernorm_reduce")
    _on(parts, x, "layernorm_reduce parts")
    _is(x, torch.float32, "layernorm_reduce x")
    _is(parts, torch.float32, "layernorm_reduce parts")
    _dt(out_dtype)
    if x.dim() != 2 or parts.dim() != 3 or x.data_ptr() % 16 or parts.data_ptr() % 16:
        raise ValueError(f"layernorm_reduce: x {tuple(x.shape)} / parts {tuple(parts.shape)} must be 16-byte aligned [rows, C] / [n, rows, C] tensors")
    rows, C = x.shape
    _vec(gamma, x, (C,), "layernorm_reduce gamma")
    _vec(beta, x, (C,), "layernorm_reduce beta")
    if parts.dtype != torch.float32 or tuple(parts.shape[1:]) != (rows, C) or not parts.is_contiguous() or not x.is_contiguous() or x.dtype != torch.float32:
        raise ValueError(f"layernorm_reduce: x {tuple(x.shape)} {x.dtype} / parts {tuple(parts.shape)} {parts.dtype} must be contiguous fp32 with matching rows")
    out = torch.empty((rows, C), dtype=out_dtype, device=x.device)
    lib = _lib.load()
    st = _timed("cft_layernorm", 0.0, rows * C * (8.0 + 4.0 * parts.shape[0] + out.element_size()),
                lambda: lib.cft_layernorm_reduce(x.data_ptr(), parts.data_ptr(), parts.shape[0], gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                                 rows, C, eps, _dt(out_dtype), _stream()))
    _lib.check(st, "cft_layernorm_reduce")
    return out


def focus_s2d(img, dtype):
    """[B,3,H,W] float image batch (NCHW) -> [B,16,H/2,W/2] NHWC in ``dtype`` (12 real channels)."""
    _require_cuda(img, "focus_s2d")
    _dt(dtype)
    if img.dim() != 4:
        raise ValueError(f"focus_s2d: expected a [B,3,H,W] image batch, got {tuple(img.shape)}")
    if img.dtype == torch.uint8:
        # raw camera bytes, e.g. ``img6[:, :3]`` / ``img6[:, 3:]`` of the reference's [B,6,H,W] uint8 batch:
        # normalisation (/255), channel split (strides) and cast are fused into the gather
        B, C, H, W = img.shape
        if C != 3 or img.stride(3) != 1 or H % 2 or W % 2:
            raise ValueError("focus_s2d: uint8 input must be [B,3,H,W] with contiguous rows and even H and W")
        out = new_nhwc(B, H // 2, W // 2, 16, dtype, img.device)
        st = _lib.load().cft_focus_s2d_u8(img.data_ptr(), img.stride(0), img.stride(1), img.stride(2), out.data_ptr(),
                                          B, H, W, 1.0 / 255.0, _dt(dtype), _stream())
        _lib.check(st, "cft_focus_s2d_u8")
        return out
    B, C, H, W = img.shape
    if C != 3 or H % 2 or W % 2:
        raise ValueError(f"focus_s2d: expected 3 input channels and even H and W, got {tuple(img.shape)}")
    if img.dtype != torch.float32 or not img.is_contiguous():
        # half / bf16 / strided images -> contiguous fp32 NCHW with the conversion kernel: seen as an "NHWC" problem
        # with (batch*channel, row, 1 pixel, W "channels") the output is exactly the contiguous NCHW image
        if img.dtype not in COMPUTE_DTYPES:
            raise TypeError(f"focus_s2d: unsupported image dtype {img.dtype}")
        if W % 4:
            raise ValueError("focus_s2d: image width must be a multiple of 4")
        flat = torch.empty((B, 3, H, W), dtype=torch.float32, device=img.device)
        lib, es = _lib.load(), img.element_size()
        sb, sc, sh, sw = img.stride()
        if sb == 3 * sc:          # (batch, channel) collapse into one uniform axis of 3B planes
            calls = [(img.data_ptr(), flat.data_ptr(), (sc, sw, sh, 0), B * 3, H)]
        elif sc == H * sh:        # the three planes of an image are stacked rows, e.g. f[:, :3] / f[:, 3:] of the callers'
            calls = [(img.data_ptr(), flat.data_ptr(), (sb, sw, sh, 0), B, 3 * H)]      # [B,6,H,W] batch (test.py:112-113)
        else:                     # arbitrary strides: one launch per image
            calls = [(img.data_ptr() + b * sb * es, flat.data_ptr() + b * 3 * H * W * 4, (sc, sw, sh, 0), 3, H) for b in range(B)]
        for src, dst, (s0, s1, s2, s3), nb, nh in calls:
            _lib.check(lib.cft_to_nhwc(src, _dt(img.dtype), s0, s1, s2, s3, dst, W, 0, nb, W, W, nh, 1, CFT_F32, _stream()),
                       "cft_to_nhwc(image)")
        img = flat
    out = new_nhwc(B, H // 2, W // 2, 16, dtype, img.device)
    st = _lib.load().cft_focus_s2d(img.data_ptr(), out.data_ptr(), B, H, W, _dt(dtype), _stream())
    _lib.check(st, "cft_focus_s2d")
    return out


def focus_conv(img, pk, act, dtype):
    """Focus = space-to-depth + 3x3 Conv of the image batch ``img`` ([B,3,H,W] float or uint8, NCHW).
    bf16 with 32/48/64/80 output channels runs as ONE kernel (cft_focus_conv: no intermediate tensor, bit-identical);
    anything else as cft_focus_s2d + cft_conv2d."""
    _require_cuda(img, "focus_conv")
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"focus_conv: expected a [B,3,H,W] image batch, got {tuple(img.shape)}")
    _dt(dtype)
    _packed_for(pk, img, "focus_conv", dtype)
    fusable = (dtype in (torch.bfloat16, torch.float16) and pk.k == 3 and pk.s == 1 and pk.cin == 16 and pk.kpad == 192
               and pk.n in (32, 48, 64, 80) and act in (ACT_NONE, ACT_SILU)
               and (img.dtype in (torch.uint8, torch.float32) or (img.dtype == torch.float16 and dtype == torch.float16)))
    if not fusable:
        return conv2d(focus_s2d(img, dtype), pk, act)
    es = img.element_size()
    if img.stride(3) != 1 or any(img.stride(i) % 2 for i in range(3)) or img.data_ptr() % (2 * es):
        img = img.contiguous()
    B, _, H, W = img.shape
    if H % 2 or W % 2:
        raise ValueError("focus_conv: H and W must be even")
    u8 = img.dtype == torch.uint8
    kind = 1 if u8 else (2 if img.dtype == torch.float16 else 0)
    out = new_nhwc(B, H // 2, W // 2, pk.n, dtype, img.device)
    lib = _lib.load()
    args = (img.data_ptr(), kind, img.stride(0), img.stride(1), img.stride(2), 1.0 / 255.0 if u8 else 1.0,
            pk.w.data_ptr(), pk.kpad, _bias_ptr(pk), out.data_ptr(),
            _view_ld(out, "focus_conv out"), 0, B, H, W, pk.n, act, _dt(dtype), _stream())
    rows = B * (H // 2) * (W // 2)
    abytes = img.numel() * es + rows * pk.n_valid * 2 + pk.w.numel() * 2
    # counted with the GEMM family (it is the same implicit-GEMM MFMA work, on a dedicated kernel)
    st = _timed(f"conv_focus_k3s1_n{pk.n}_K{pk.kpad}", rows * pk.flops_per_row, abytes, lambda: lib.cft_focus_conv(*args))
    _lib.check(st, "cft_focus_conv")
    return out


def spp_maxpool(buf, C, ks):
    """In-place: buf [B,4C,H,W] NHWC, channels [0,C) already hold x; fills the three pooled slices."""
    _require_cuda(buf, "spp_maxpool")
    if buf.dim() != 4 or buf.shape[1] != 4 * C:
        raise ValueError(f"spp_maxpool: buf must be [B, {4 * C}, H, W] (x and its three pooled slices), got {tuple(buf.shape)}")
    B, C4, H, W = buf.shape
    ld = _out_view(buf, buf, "spp_maxpool")
    st = _lib.load().cft_spp_maxpool(buf.data_ptr(), B, H, W, C, ld, ks[0], ks[1], ks[2], _dt(buf.dtype), _stream())
    _lib.check(st, "cft_spp_maxpool")
    return buf


def copy_channels(src, dst, up=0):
    """dst[b, :, y, x] = src[b, :, y >> up, x >> up] (dst is usually a channel slice of a concat buffer)."""
    _require_cuda(src, "copy_channels")
    _is(dst, src.dtype, "copy_channels dst")
    src, ldi = as_nhwc(src)
    ldo = _out_view(dst, src, "copy_channels dst")
    B, C, Ho, Wo = dst.shape
    if src.shape[0] != B or src.shape[1] != C or (src.shape[2] << up) != Ho or (src.shape[3] << up) != Wo:
        raise ValueError(f"copy_channels: {tuple(src.shape)} -> {tuple(dst.shape)} with up={up}")
    st = _lib.load().cft_copy_channels(src.data_ptr(), ldi, 0, dst.data_ptr(), ldo, 0, B, Ho, Wo, C, up, _dt(dst.dtype), _stream())
    _lib.check(st, "cft_copy_channels")
    return dst


def add(a, b, out=None):
    _require_cuda(a, "add")
    _on(b, a, "add b")
    _dt(a.dtype)
    _is(b, a.dtype, "add b")
    if a.shape != b.shape:
        raise ValueError(f"add: {tuple(a.shape)}/{a.dtype} vs {tuple(b.shape)}/{b.dtype}")
    a, lda = as_nhwc(a)
    b, ldb = as_nhwc(b)
    B, C, H, W = a.shape
    if out is None:
        out = new_nhwc(B, H, W, C, a.dtype, a.device)
        ldo = C
    else:
        _is(out, a.dtype, "add out")
        ldo = _out_view(out, a, "add out", (B, C, H, W))
    st = _lib.load().cft_add(a.data_ptr(), lda, 0, b.data_ptr(), ldb, 0, out.data_ptr(), ldo, 0, B * H * W, C, _dt(a.dtype), _stream())
    _lib.check(st, "cft_add")
    return out


ANCHOR_GRID = (8, 8)      # the reference's default GPT grid: the kernels of the 8x8 path (cft_gpt_tokenize, cft_attention, ...)


def token_grid(tokens, grid=None):
    """The anchor grid (va, ha) of a GPT token tensor [B, 2*va*ha, C]: ``grid`` when given, else the ``anchor_grid`` attribute that
    ``GPT.forward`` sets on the tokens it hands to its consumers, else the 8 x 8 default.  (The token count alone does not fix the grid:
    4 x 16 and 8 x 8 both have 128 tokens.)"""
    return tuple(grid) if grid is not None else getattr(tokens, "anchor_grid", ANCHOR_GRID)


def _grid(grid):
    va, ha = (int(g) for g in grid)
    if va < 1 or ha < 1 or va * ha > 1024:
        raise NotImplementedError(f"anchor grid {va}x{ha}: supported grids have 1 <= vert_anchors, horz_anchors and "
                                  f"vert_anchors * horz_anchors <= 1024 (T = 2 * va * ha <= 2048 tokens)")
    return va, ha


def _grid_entry(lib, name, va, ha):
    """(function, label, extra arguments) of a GPT token kernel on a va x ha anchor grid: the specialised 8 x 8 kernel ``name``, or
    ``name_grid`` with its (va, ha) arguments on any other grid."""
    if (va, ha) == (8, 8):
        return getattr(lib, name), name, ()
    return getattr(lib, name + "_grid"), name + "_grid", (va, ha)


def gpt_tokenize(rgb, ir, pos_emb, grid=ANCHOR_GRID):
    """-> float32 tokens [B, 2*va*ha, C] (adaptive average pool of both streams to the ``grid`` = (va, ha) anchors, + pos_emb)."""
    _require_cuda(rgb, "gpt_tokenize")
    va, ha = _grid(grid)
    _on(ir, rgb, "gpt_tokenize ir")
    _dt(rgb.dtype)
    _is(ir, rgb.dtype, "gpt_tokenize ir")
    if rgb.dim() != 4 or ir.shape != rgb.shape:
        raise ValueError(f"gpt_tokenize: the two streams must be [B,C,H,W] tensors of one shape, got {tuple(rgb.shape)} and {tuple(ir.shape)}")
    T = 2 * va * ha
    _vec(pos_emb, rgb, (T, rgb.shape[1]), "gpt_tokenize pos_emb")
    rgb, ld_r = as_nhwc(rgb)
    ir, ld_i = as_nhwc(ir)
    B, C, H, W = rgb.shape
    tokens = torch.empty((B, T, C), dtype=torch.float32, device=rgb.device)
    lib = _lib.load()
    fn, label, grid_args = _grid_entry(lib, "cft_gpt_tokenize", va, ha)
    st = _timed("cft_tokenize", 0.0, 2.0 * B * H * W * C * rgb.element_size() + B * T * C * 4,
                lambda: fn(rgb.data_ptr(), ld_r, 0, ir.data_ptr(), ld_i, 0, pos_emb.data_ptr(), tokens.data_ptr(),
                           B, H, W, C, *grid_args, _dt(rgb.dtype), _stream()))
    _lib.check(st, label)
    return tokens


def layernorm(x, gamma, beta, out_dtype, eps=1e-5):
    """x float32 [rows, C] -> out_dtype [rows, C]."""
    _require_cuda(x, "layernorm")
    _is(x, torch.float32, "layernorm x")
    _dt(out_dtype)
    if x.dim() != 2 or not x.is_contiguous() or x.data_ptr() % 16:
        raise ValueError(f"layernorm: x must be a contiguous, 16-byte aligned [rows, C] tensor, got {tuple(x.shape)} with strides {tuple(x.stride())}")
    rows, C = x.shape
    _vec(gamma, x, (C,), "layernorm gamma")
    _vec(beta, x, (C,), "layernorm beta")
    out = torch.empty((rows, C), dtype=out_dtype, device=x.device)
    lib = _lib.load()
    st = _timed("cft_layernorm", 0.0, rows * C * (4.0 + out.element_size()),
                lambda: lib.cft_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, C, eps, _dt(out_dtype), _stream()))
    _lib.check(st, "cft_layernorm")
    return out


def attention(qkv, B, heads, dk, dkp, pdrop=0.0, T=128, general=False):
    """qkv [B*T, 3*heads*dkp] -> [B*T, heads*dkp].  ``pdrop`` > 0: training-mode dropout of the attention probabilities inside the
    kernel.  T = 128 runs the single-tile kernel (cft_attention), any other T (1 .. 2048) the flash-style one (cft_attention_tokens);
    ``general=True`` forces the latter at T = 128 too."""
    _require_cuda(qkv, "attention")
    _dt(qkv.dtype)
    if tuple(qkv.shape) != (B * T, 3 * heads * dkp) or not qkv.is_contiguous() or qkv.data_ptr() % 16 or dkp < dk:
        raise ValueError(f"attention: qkv must be a contiguous, 16-byte aligned [{B * T}, {3 * heads * dkp}] tensor (B * T rows of q | k | v, "
                         f"heads x dkp each), got {tuple(qkv.shape)} with strides {tuple(qkv.stride())}")
    out = torch.empty((B * T, heads * dkp), dtype=qkv.dtype, device=qkv.device)
    lib = _lib.load()
    seed = next_dropout_seed() if pdrop > 0 else 0
    flops, abytes = 4.0 * T * T * dk * heads * B, 4.0 * B * T * heads * dkp * qkv.element_size()
    if T == 128 and not general:
        st = _timed("cft_attention", flops, abytes,
                    lambda: lib.cft_attention(qkv.data_ptr(), out.data_ptr(), B, heads, dk, dkp, _dt(qkv.dtype), float(pdrop), seed, _stream()))
        _lib.check(st, "cft_attention")
    else:
        st = _timed("cft_attention_tokens", flops, abytes,
                    lambda: lib.cft_attention_tokens(qkv.data_ptr(), out.data_ptr(), B, T, heads, dk, dkp, _dt(qkv.dtype), float(pdrop), seed,
                                                     _stream()))
        _lib.check(st, "cft_attention_tokens")
    return out


def gpt_upsample_add(tokens, s, base, H, W, dtype, grid=None):
    """bilinear(va x ha -> HxW) of stream ``s`` of ``tokens`` [B, 2*va*ha, C] (+ base) -> NHWC [B,C,H,W]; ``grid`` = (va, ha), by default
    ``token_grid(tokens)``."""
    _require_cuda(tokens, "gpt_upsample_add")
    grid = token_grid(tokens, grid)
    va, ha = _grid(grid)
    if isinstance(tokens, torch.Tensor) and tokens.dtype != torch.float32:
        raise TypeError(f"gpt_upsample_add: tokens must be float32, got {tokens.dtype}")
    if s not in (0, 1):
        raise ValueError(f"gpt_upsample_add: stream index must be 0 or 1, got {s}")
    _dt(dtype)
    if not gpt_dual_tokens_ok(tokens, grid):
        raise ValueError(f"gpt_upsample_add: tokens must be a contiguous, 16-byte aligned fp32 [B, {2 * va * ha}, C] tensor (C % 4 == 0), "
                         f"got {tuple(tokens.shape)} {tokens.dtype}")
    B, T, C = tokens.shape
    out = new_nhwc(B, H, W, C, dtype, tokens.device)
    bp, ldb = None, 0
    if base is not None:
        _on(base, tokens, "gpt_upsample_add base")
        _is(base, dtype, "gpt_upsample_add base")
        if tuple(base.shape) != (B, C, H, W):
            raise ValueError(f"gpt_upsample_add: base has shape {tuple(base.shape)}, expected {(B, C, H, W)}")
        base, ldb = as_nhwc(base)
        bp = base.data_ptr()
    lib = _lib.load()
    fn, label, grid_args = _grid_entry(lib, "cft_gpt_upsample_add", va, ha)
    st = _timed("cft_upsample_add", 0.0, (2.0 if bp else 1.0) * B * H * W * C * out.element_size(),
                lambda: fn(tokens.data_ptr(), s, bp, ldb, 0, out.data_ptr(), C, 0, B, H, W, C, *grid_args, _dt(dtype), _stream()))
    _lib.check(st, label)
    return out


def gpt_dual_tokens_ok(tokens, grid=None):
    """What ``cft_gpt_upsample_add2`` (and the ``_grid`` de-tokenisers) hard-code about the token tensor: [B, 2*va*ha, C] (two streams x
    va x ha anchors; 128 at the default 8 x 8), fp32, contiguous, C a multiple of 4 and a 16-byte aligned base (rows are read as float4)."""
    va, ha = (int(g) for g in token_grid(tokens, grid))
    return (isinstance(tokens, torch.Tensor) and _is_cuda(tokens) and tokens.dim() == 3 and tokens.shape[1] == 2 * va * ha
            and tokens.dtype == torch.float32 and tokens.is_contiguous() and tokens.shape[2] % 4 == 0 and tokens.data_ptr() % 16 == 0)


def gpt_upsample_add_dual(tokens, base0, base1, H, W, dtype, sum_out=None, want_sum=True, grid=None):
    """Both streams of a CFT block and the Add behind them in one kernel (cft_gpt_upsample_add2, or cft_gpt_upsample_add2_grid on a
    ``grid`` other than 8 x 8): returns (base0 + up(tokens[:, :va*ha]), base1 + up(tokens[:, va*ha:]), their sum or None); ``sum_out``:
    write the sum there (e.g. a channel slice of a planned concat buffer)."""
    _require_cuda(tokens, "gpt_upsample_add_dual")
    grid = token_grid(tokens, grid)
    va, ha = _grid(grid)
    if isinstance(tokens, torch.Tensor) and tokens.dtype != torch.float32:
        raise TypeError(f"gpt_upsample_add_dual: tokens must be float32, got {tokens.dtype}")
    _dt(dtype)
    if not gpt_dual_tokens_ok(tokens, grid):
        raise ValueError(f"gpt_upsample_add_dual: tokens must be a contiguous, 16-byte aligned fp32 [B, {2 * va * ha}, C] tensor (C % 4 == 0), "
                         f"got {tuple(tokens.shape)} {tokens.dtype}")
    B, T, C = tokens.shape
    for bse in (base0, base1):
        _on(bse, tokens, "gpt_upsample_add_dual base")
        _is(bse, dtype, "gpt_upsample_add_dual base")
        if tuple(bse.shape) != (B, C, H, W):
            raise ValueError(f"gpt_upsample_add_dual: base has shape {tuple(bse.shape)}, expected {(B, C, H, W)}")
    base0, ldb0 = as_nhwc(base0)
    base1, ldb1 = as_nhwc(base1)
    out0 = new_nhwc(B, H, W, C, dtype, tokens.device)
    out1 = new_nhwc(B, H, W, C, dtype, tokens.device)
    sp, lds = None, 0
    if want_sum:
        if sum_out is None:
            sum_out = new_nhwc(B, H, W, C, dtype, tokens.device)
        _is(sum_out, dtype, "gpt_upsample_add_dual sum_out")
        lds = _out_view(sum_out, tokens, "gpt_upsample_add_dual sum_out", (B, C, H, W))
        sp = sum_out.data_ptr()
    else:
        sum_out = None
    lib = _lib.load()
    fn, label, grid_args = _grid_entry(lib, "cft_gpt_upsample_add2", va, ha)
    st = _timed("cft_upsample_add", 0.0, (5.0 if want_sum else 4.0) * B * H * W * C * out0.element_size(),
                lambda: fn(tokens.data_ptr(), base0.data_ptr(), ldb0, 0, base1.data_ptr(), ldb1, 0, out0.data_ptr(), C, 0, out1.data_ptr(), C, 0,
                           sp, lds, 0, B, H, W, C, *grid_args, _dt(dtype), _stream()))
    _lib.check(st, label)
    return out0, out1, sum_out


def detect_decode(logits, raw, pred, anchors_px, na, no, stride, row0):
    """logits [B, ldl, ny, nx] NHWC float32; raw [B,na,ny,nx,no]; pred [B,rows,no] (filled at row0)."""
    _require_cuda(logits, "detect_decode")
    for t, what in ((logits, "logits"), (raw, "raw"), (pred, "pred")):
        _on(t, logits, f"detect_decode {what}")
        _is(t, torch.float32, f"detect_decode {what}")
    if logits.dim() != 4:
        raise ValueError(f"detect_decode: logits must be [B, ldl, ny, nx], got {tuple(logits.shape)}")
    B, ldl, ny, nx = logits.shape
    if _view_ld(logits, "detect_decode logits") != ldl or ldl < na * no or logits.data_ptr() % 16:
        raise ValueError(f"detect_decode: logits must be a dense, 16-byte aligned NHWC tensor of >= {na * no} channels")
    if tuple(raw.shape) != (B, na, ny, nx, no) or not raw.is_contiguous() or raw.data_ptr() % 16 or pred.data_ptr() % 16:
        raise ValueError(f"detect_decode: raw must be a contiguous {(B, na, ny, nx, no)} tensor, got {tuple(raw.shape)}")
    if pred.dim() != 3 or pred.shape[0] != B or pred.shape[2] != no or not pred.is_contiguous() or row0 < 0 or row0 + na * ny * nx > pred.shape[1]:
        raise ValueError(f"detect_decode: pred must be a contiguous [{B}, rows, {no}] tensor with rows >= row0 + {na * ny * nx}, got {tuple(pred.shape)} (row0 {row0})")
    _vec(anchors_px, logits, (na * 2,), "detect_decode anchors_px")
    st = _lib.load().cft_detect_decode(logits.data_ptr(), ldl, raw.data_ptr(), pred.data_ptr(), anchors_px.data_ptr(),
                                       B, ny, nx, na, no, float(stride), row0, pred.shape[1], _stream())
    _lib.check(st, "cft_detect_decode")


def pair_batch_u8(desc_dev, desc_host, out, color=114):
    """One launch assembles the uint8 [B, 6, H, W] RGB + IR batch ``out`` from a table of cft_pair_desc_t rows (cft_pair_batch_u8):
    ``desc_dev`` [B, 64] uint8 on the device is what the kernel reads, ``desc_host`` the same bytes on the host is what the guards read."""
    _require_cuda(out, "pair_batch_u8")
    _require_cuda(desc_dev, "pair_batch_u8")
    B = out.shape[0]
    if out.dtype != torch.uint8 or out.dim() != 4 or out.shape[1] != 6 or not out.is_contiguous():
        raise ValueError(f"pair_batch_u8: out must be a contiguous uint8 [B, 6, H, W] tensor, got {out.dtype} {tuple(out.shape)}")
    for t, what in ((desc_dev, "desc_dev"), (desc_host, "desc_host")):
        if t.dtype != torch.uint8 or tuple(t.shape) != (B, _lib._consts["CFT_PAIR_DESC_BYTES"]) or not t.is_contiguous():
            raise ValueError(f"pair_batch_u8: {what} must be a contiguous uint8 [{B}, {_lib._consts['CFT_PAIR_DESC_BYTES']}] tensor")
    if desc_host.is_cuda:
        raise ValueError("pair_batch_u8: desc_host must be a host tensor")
    st = _lib.load().cft_pair_batch_u8(desc_dev.data_ptr(), desc_host.data_ptr(), B, out.data_ptr(), out.shape[2], out.shape[3], int(color), _stream())
    _lib.check(st, "cft_pair_batch_u8")
    return out


def augment_batch_u8(desc_dev, desc_host, luts, out):
    """One launch assembles the augmented uint8 [B, 6, H, W] RGB + IR training batch ``out`` from a table of cft_aug_desc_t rows
    (cft_augment_batch_u8): ``desc_dev`` [B, 400] uint8 on the device is what the kernel reads, ``desc_host`` the same bytes on the host
    is what the guards read, ``luts`` uint8 [B, 2, 3, 256] on the device the HSV look-up tables of every image and stream."""
    _require_cuda(out, "augment_batch_u8")
    _require_cuda(desc_dev, "augment_batch_u8")
    _require_cuda(luts, "augment_batch_u8")
    B, nbytes = out.shape[0], _lib._consts["CFT_AUG_DESC_BYTES"]
    if out.dtype != torch.uint8 or out.dim() != 4 or out.shape[1] != 6 or not out.is_contiguous():
        raise ValueError(f"augment_batch_u8: out must be a contiguous uint8 [B, 6, H, W] tensor, got {out.dtype} {tuple(out.shape)}")
    for t, what in ((desc_dev, "desc_dev"), (desc_host, "desc_host")):
        if t.dtype != torch.uint8 or tuple(t.shape) != (B, nbytes) or not t.is_contiguous():
            raise ValueError(f"augment_batch_u8: {what} must be a contiguous uint8 [{B}, {nbytes}] tensor")
    if desc_host.is_cuda:
        raise ValueError("augment_batch_u8: desc_host must be a host tensor")
    if luts.dtype != torch.uint8 or tuple(luts.shape) != (B, 2, 3, 256) or not luts.is_contiguous():
        raise ValueError(f"augment_batch_u8: luts must be a contiguous uint8 [{B}, 2, 3, 256] tensor")
    st = _lib.load().cft_augment_batch_u8(desc_dev.data_ptr(), desc_host.data_ptr(), luts.data_ptr(), B, out.data_ptr(), out.shape[2], out.shape[3], _stream())
    _lib.check(st, "cft_augment_batch_u8")
    return out


BOX_WORDS = 16        # 32-bit words per detection slot of cft_detect_boxes (include/cft_hip.h)


def detect_boxes(dets, counts, geom, nc, crop_gain=1.02, crop_pad=10, square=False, flag=None):
    """cft_detect_boxes on the batched_nms output: ``(boxes int32 [B, max_det, 16], hist int32 [B, nc], flag int32 [1])``, all on the
    device; the four float words 12..15 of a slot are read with ``boxes[..., 12:].view(torch.float32)``.  ``flag`` is ORed into."""
    for t in (dets, counts, geom):
        _require_cuda(t, "detect_boxes")
    if dets.dtype != torch.float32 or dets.dim() != 3 or dets.shape[2] != 6 or not dets.is_contiguous() or dets.shape[0] == 0 or dets.shape[1] == 0:
        raise ValueError(f"detect_boxes: dets must be a contiguous float32 [B, max_det, 6] tensor, got {dets.dtype} {tuple(dets.shape)}")
    B, max_det = dets.shape[0], dets.shape[1]
    if counts.dtype != torch.int32 or tuple(counts.shape) != (B,) or not counts.is_contiguous():
        raise ValueError(f"detect_boxes: counts must be a contiguous int32 [{B}] tensor")
    if geom.dtype != torch.float32 or tuple(geom.shape) != (B, 5) or not geom.is_contiguous():
        raise ValueError(f"detect_boxes: geom must be a contiguous float32 [{B}, 5] tensor")
    boxes = torch.empty((B, max_det, BOX_WORDS), dtype=torch.int32, device=dets.device)
    hist = torch.empty((B, int(nc)), dtype=torch.int32, device=dets.device)
    if flag is None:
        flag = torch.zeros((1,), dtype=torch.int32, device=dets.device)
    st = _lib.load().cft_detect_boxes(dets.data_ptr(), counts.data_ptr(), B, max_det, geom.data_ptr(), int(nc), float(crop_gain), float(crop_pad),
                                      int(bool(square)), boxes.data_ptr(), hist.data_ptr(), flag.data_ptr(), _stream())
    _lib.check(st, "cft_detect_boxes")
    return boxes, hist, flag


def detect_render(desc_dev, desc_host, boxes, colors, text_color, thickness, flags, names=None, name_len=None, atlas=None):
    """cft_detect_render: draws the slots of ``boxes`` [B, max_det, 16] into the images of the table (``desc_dev`` [B, 48] uint8 on the
    device, ``desc_host`` the same bytes on the host), in place.  ``colors`` uint8 [nc, 3], ``names`` uint8 [nc, L], ``name_len`` int32
    [nc], ``atlas`` uint8 [96, gh, gw], all on the device; ``text_color`` three bytes."""
    nb = _lib._consts["CFT_RENDER_DESC_BYTES"]
    B = boxes.shape[0]
    for t, what in ((desc_dev, "desc_dev"), (desc_host, "desc_host")):
        if t.dtype != torch.uint8 or tuple(t.shape) != (B, nb) or not t.is_contiguous():
            raise ValueError(f"detect_render: {what} must be a contiguous uint8 [{B}, {nb}] tensor")
    if desc_host.is_cuda:
        raise ValueError("detect_render: desc_host must be a host tensor")
    if boxes.dtype != torch.int32 or boxes.dim() != 3 or boxes.shape[2] != BOX_WORDS or not boxes.is_contiguous():
        raise ValueError("detect_render: boxes must be the contiguous int32 [B, max_det, 16] output of detect_boxes")
    if colors.dtype != torch.uint8 or colors.dim() != 2 or colors.shape[1] != 3 or not colors.is_contiguous():
        raise ValueError("detect_render: colors must be a contiguous uint8 [nc, 3] tensor")
    nc = colors.shape[0]
    dev = [desc_dev, boxes, colors]
    L = gh = gw = 0
    if flags & _lib._consts["CFT_RENDER_LABELS"]:
        if names is None or name_len is None or atlas is None:
            raise ValueError("detect_render: labels need names, name_len and atlas")
        if names.dtype != torch.uint8 or names.dim() != 2 or names.shape[0] != nc or not names.is_contiguous():
            raise ValueError(f"detect_render: names must be a contiguous uint8 [{nc}, L] tensor")
        if name_len.dtype != torch.int32 or tuple(name_len.shape) != (nc,) or not name_len.is_contiguous():
            raise ValueError(f"detect_render: name_len must be a contiguous int32 [{nc}] tensor")
        if atlas.dtype != torch.uint8 or atlas.dim() != 3 or atlas.shape[0] != 96 or not atlas.is_contiguous():
            raise ValueError("detect_render: atlas must be a contiguous uint8 [96, gh, gw] tensor")
        L, gh, gw = names.shape[1], atlas.shape[1], atlas.shape[2]
        dev += [names, name_len, atlas]
    for t in dev:
        _require_cuda(t, "detect_render")
    tc = int(text_color[0]) | int(text_color[1]) << 8 | int(text_color[2]) << 16
    ptr = lambda t: t.data_ptr() if t is not None else None
    st = _lib.load().cft_detect_render(desc_dev.data_ptr(), desc_host.data_ptr(), B, boxes.data_ptr(), boxes.shape[1], colors.data_ptr(), nc, tc,
                                       int(thickness), int(flags), ptr(names), ptr(name_len), L, ptr(atlas), gh, gw, _stream())
    _lib.check(st, "cft_detect_render")


_MOSAIC_DTYPES = {torch.uint8: "CFT_MOSAIC_U8", torch.float16: "CFT_MOSAIC_F16", torch.float32: "CFT_MOSAIC_F32"}


def _hwc_u8(t, what):
    _require_cuda(t, what)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.stride(2) != 1 or t.stride(1) != 3:
        raise ValueError(f"{what}: a mosaic must be an HWC uint8 CUDA tensor with contiguous pixels")


def mosaic_compose(images, c0, bs, ns, h, w, resize, out, maxkey=None):
    """cft_mosaic_compose: channels [c0, c0 + 3) of the first ``bs`` images of the (possibly strided) ``[B, C, H, W]`` uint8 / fp16 / fp32
    batch into the HWC uint8 mosaic ``out`` [ns*h, ns*w, 3].  ``maxkey`` int32 [1]: device scratch for the maximum of image 0."""
    _require_cuda(images, "mosaic_compose")
    _hwc_u8(out, "mosaic_compose")
    if images.dim() != 4 or images.dtype not in _MOSAIC_DTYPES:
        raise ValueError(f"mosaic_compose: images must be a [B, C, H, W] uint8, float16 or float32 tensor, got {images.dtype} {tuple(images.shape)}")
    if tuple(out.shape) != (ns * h, ns * w, 3):
        raise ValueError(f"mosaic_compose: out must be [{ns * h}, {ns * w}, 3], got {tuple(out.shape)}")
    if maxkey is None:
        maxkey = torch.empty((1,), dtype=torch.int32, device=images.device)
    B, C, H, W = images.shape
    st = _lib.load().cft_mosaic_compose(images.data_ptr(), _lib._consts[_MOSAIC_DTYPES[images.dtype]], B, C, H, W, *images.stride(), int(c0), int(bs),
                                        int(ns), int(h), int(w), int(bool(resize)), out.data_ptr(), out.stride(0), maxkey.data_ptr(), _stream())
    _lib.check(st, "cft_mosaic_compose")
    return out


def mosaic_slots(targets, bs, cap, nc, h, w, sf, flag=None):
    """cft_mosaic_slots: ``targets`` is a contiguous float32 / float64 ``[nt, 6 or 7]`` CUDA tensor (image, class, x, y, w, h[, conf]) or the
    ``(dets [B, max_det, 6] float32, counts [B] int32)`` pair of ``batched_nms``.  Returns ``(slots int32 [bs, cap, 16], flag int32 [1])``
    on the device; ``flag`` is ORed into (CFT_MOSAIC_BAD_CLASS, CFT_MOSAIC_OVERFLOW)."""
    import ctypes
    pair = isinstance(targets, (tuple, list))
    first = targets[0] if pair else targets
    _require_cuda(first, "mosaic_slots")
    slots = torch.empty((int(bs), int(cap), BOX_WORDS), dtype=torch.int32, device=first.device)
    if flag is None:
        flag = torch.zeros((1,), dtype=torch.int32, device=first.device)
    sfd = ctypes.c_double(float(sf))
    if pair:
        dets, counts = targets
        _require_cuda(counts, "mosaic_slots")
        if dets.dtype != torch.float32 or dets.dim() != 3 or dets.shape[2] != 6 or not dets.is_contiguous() or dets.shape[1] == 0:
            raise ValueError(f"mosaic_slots: dets must be a contiguous float32 [B, max_det, 6] tensor, got {dets.dtype} {tuple(dets.shape)}")
        if counts.dtype != torch.int32 or tuple(counts.shape) != (dets.shape[0],) or not counts.is_contiguous():
            raise ValueError(f"mosaic_slots: counts must be a contiguous int32 [{dets.shape[0]}] tensor")
        args = (None, 0, 7, 1, dets.data_ptr(), counts.data_ptr(), dets.shape[0], dets.shape[1])
    else:
        t = targets
        if t.dtype not in (torch.float32, torch.float64) or t.dim() != 2 or t.shape[1] not in (6, 7) or not t.is_contiguous() or t.shape[0] == 0:
            raise ValueError(f"mosaic_slots: rows must be a contiguous float32 / float64 [nt > 0, 6 or 7] tensor, got {t.dtype} {tuple(t.shape)}")
        args = (t.data_ptr(), t.shape[0], t.shape[1], int(t.dtype == torch.float64), None, None, 0, 0)
    st = _lib.load().cft_mosaic_slots(*args, int(bs), int(cap), int(nc), int(h), int(w), ctypes.byref(sfd), slots.data_ptr(), flag.data_ptr(), _stream())
    _lib.check(st, "cft_mosaic_slots")
    return slots, flag


def mosaic_finish(mosaic, mosaic_ir, bs, ns, h, w, codes=None, name_len=None, atlas=None):
    """cft_mosaic_finish: file names (``codes`` uint8 [bs, 40], ``name_len`` int32 [bs], ``atlas`` uint8 [96, gh, gw]; None: no text) and the
    white cell borders into one or two mosaics, in place, one launch."""
    gh = gw = 0
    for m in (mosaic,) if mosaic_ir is None else (mosaic, mosaic_ir):
        _hwc_u8(m, "mosaic_finish")
        if tuple(m.shape) != (ns * h, ns * w, 3):
            raise ValueError(f"mosaic_finish: a mosaic must be [{ns * h}, {ns * w}, 3], got {tuple(m.shape)}")
    if codes is not None:
        nch = _lib._consts["CFT_MOSAIC_NAME_CHARS"]
        if codes.dtype != torch.uint8 or tuple(codes.shape) != (bs, nch) or not codes.is_contiguous():
            raise ValueError(f"mosaic_finish: codes must be a contiguous uint8 [{bs}, {nch}] tensor")
        if name_len is None or name_len.dtype != torch.int32 or tuple(name_len.shape) != (bs,) or not name_len.is_contiguous():
            raise ValueError(f"mosaic_finish: name_len must be a contiguous int32 [{bs}] tensor")
        if atlas is None or atlas.dtype != torch.uint8 or atlas.dim() != 3 or atlas.shape[0] != 96 or not atlas.is_contiguous():
            raise ValueError("mosaic_finish: atlas must be a contiguous uint8 [96, gh, gw] tensor")
        for t in (codes, name_len, atlas):
            _require_cuda(t, "mosaic_finish")
        gh, gw = atlas.shape[1], atlas.shape[2]
    ptr = lambda t: t.data_ptr() if t is not None else None
    st = _lib.load().cft_mosaic_finish(mosaic.data_ptr(), ptr(mosaic_ir), mosaic.stride(0), mosaic_ir.stride(0) if mosaic_ir is not None else 0, int(bs),
                                       int(ns), int(h), int(w), ptr(codes), ptr(name_len) if codes is not None else None,
                                       ptr(atlas) if codes is not None else None, gh, gw, _stream())
    _lib.check(st, "cft_mosaic_finish")


def mosaic_area(src, dh, dw):
    """cft_mosaic_area: the INTER_AREA reduction of an HWC uint8 mosaic to ``[dh, dw, 3]`` (a new tensor), at most 4x per axis."""
    _hwc_u8(src, "mosaic_area")
    sh, sw = src.shape[0], src.shape[1]
    r = _lib._consts["CFT_PAIR_MAX_REDUCTION"]
    if not (0 < dh <= sh and 0 < dw <= sw and dh * r >= sh and dw * r >= sw):
        raise ValueError(f"mosaic_area: {sh}x{sw} -> {dh}x{dw} is not a reduction by 1x to {r}x per axis")
    dst = torch.empty((int(dh), int(dw), 3), dtype=torch.uint8, device=src.device)
    st = _lib.load().cft_mosaic_area(src.data_ptr(), src.stride(0), sh, sw, dst.data_ptr(), dst.stride(0), int(dh), int(dw), _stream())
    _lib.check(st, "cft_mosaic_area")
    return dst


# ------------------------------------------------------------------------------ test-time augmentation
_TTA_DTYPES = {torch.uint8: "CFT_TTA_U8", torch.float16: "CFT_TTA_F16", torch.float32: "CFT_TTA_F32"}


def tta_view_size(H, W, ratio, gs):
    """``((hs, ws), (Ho, Wo))`` of one view: the scaled and the padded size of the reference's ``scale_img`` (utils/torch_utils.py:252-256)."""
    import math
    return (int(H * ratio), int(W * ratio)), tuple(math.ceil(x * ratio / gs) * gs for x in (H, W))


def tta_view(img, ratio, gs, flip=False, out=None):
    """cft_tta_view: the (possibly strided) ``[B, 3, H, W]`` uint8 / fp16 / fp32 batch -> one augmented view, fp32 ``[B, 3, Ho, Wo]``:
    optional left-right flip, bilinear resize by ``ratio``, right / bottom padding with 0.447 to multiples of ``gs``."""
    import ctypes
    _require_cuda(img, "tta_view")
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype not in _TTA_DTYPES:
        raise ValueError(f"tta_view: images must be a [B, 3, H, W] uint8, float16 or float32 tensor, got {img.dtype} {tuple(img.shape)}")
    B, _, H, W = img.shape
    if gs < 1:
        raise ValueError(f"tta_view: gs must be >= 1, got {gs}")
    _, (Ho, Wo) = tta_view_size(H, W, float(ratio), int(gs))
    if out is None:
        out = torch.empty((B, 3, Ho, Wo), dtype=torch.float32, device=img.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, Ho, Wo) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"tta_view: out must be a contiguous float32 CUDA tensor [{B}, 3, {Ho}, {Wo}]")
    r = ctypes.c_double(float(ratio))
    st = _lib.load().cft_tta_view(img.data_ptr(), _lib._consts[_TTA_DTYPES[img.dtype]], B, H, W, *img.stride(), ctypes.byref(r), int(gs),
                                  int(bool(flip)), out.data_ptr(), Ho, Wo, _stream())
    _lib.check(st, "cft_tta_view")
    return out


def tta_merge(preds, scales, flips, img_w, out=None):
    """cft_tta_merge: the three views' fp32 predictions ``[B, n_v, no]`` -> ``[B, sum n_v, no]``; columns 0-3 divided by the view's scale,
    column 0 of a flipped view replaced by ``img_w - x``."""
    if len(preds) != 3 or len(scales) != 3 or len(flips) != 3:
        raise ValueError("tta_merge: three views, three scales, three flips")
    for p in preds:
        _require_cuda(p, "tta_merge")
        if p.dtype != torch.float32 or p.dim() != 3 or not p.is_contiguous() or p.shape[0] != preds[0].shape[0] or p.shape[2] != preds[0].shape[2]:
            raise ValueError(f"tta_merge: predictions must be contiguous float32 [B, n, no] tensors of one B and no, got {p.dtype} {tuple(p.shape)}")
    B, _, no = preds[0].shape
    n = [p.shape[1] for p in preds]
    if out is None:
        out = torch.empty((B, sum(n), no), dtype=torch.float32, device=preds[0].device)
    elif out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != B or out.shape[2] != no or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"tta_merge: out must be a contiguous float32 CUDA tensor [{B}, n, {no}]")
    mask = sum(1 << v for v, f in enumerate(flips) if f)
    st = _lib.load().cft_tta_merge(preds[0].data_ptr(), preds[1].data_ptr(), preds[2].data_ptr(), B, n[0], n[1], n[2], no, float(scales[0]),
                                   float(scales[1]), float(scales[2]), mask, float(img_w), out.data_ptr(), out.shape[1], _stream())
    _lib.check(st, "cft_tta_merge")
    return out


# ------------------------------------------------------------------------------ training-mode forward
_dropout_state = {"seed": 0x5EED, "calls": 0}


def manual_dropout_seed(seed):
    """Seed of the counter-based dropout masks (every dropout call of a forward draws seed + call index)."""
    _dropout_state["seed"], _dropout_state["calls"] = int(seed), 0


def next_dropout_seed():
    _dropout_state["calls"] += 1
    return (_dropout_state["seed"] * 0x9E3779B1 + _dropout_state["calls"]) & 0xFFFFFFFFFFFFFFFF


def dropout_(x, p):
    """In-place nn.Dropout(p) in training mode on a contiguous tensor (cft_dropout)."""
    _require_cuda(x, "dropout_")
    if p <= 0.0:
        return x
    _dt(x.dtype)
    if not x.is_contiguous() or x.data_ptr() % 16 or x.numel() == 0:
        raise ValueError("dropout_: tensor must be contiguous, 16-byte aligned and not empty")
    if not 0.0 < p < 1.0:
        raise ValueError(f"dropout_: p must be in [0, 1), got {p}")
    st = _lib.load().cft_dropout(x.data_ptr(), x.numel(), float(p), next_dropout_seed(), _dt(x.dtype), _stream())
    _lib.check(st, "cft_dropout")
    return x


def add_rows_(x, y):
    """x += y for two [rows, C] tensors of one dtype (the CFT residual stream in training mode)."""
    _require_cuda(x, "add_rows_")
    _dt(x.dtype)
    _is(y, x.dtype, "add_rows_ y")
    _rows_ld(x, x, "add_rows_ x")
    _rows_ld(y, x, "add_rows_ y", x.shape)
    rows, C = x.shape
    st = _lib.load().cft_add(x.data_ptr(), x.stride(0), 0, y.data_ptr(), y.stride(0), 0, x.data_ptr(), x.stride(0), 0, rows, C, _dt(x.dtype), _stream())
    _lib.check(st, "cft_add(rows)")
    return x


def batchnorm_train(y32, C, bn, act, residual=None, out=None, out_dtype=None):
    """act(BatchNorm2d(y32)) with BATCH statistics (+ residual) and the running-statistics update of ``bn``
    (an nn.BatchNorm2d in training mode): y32 is the fp32 conv output [B, pad8(C), H, W] (NHWC)."""
    _require_cuda(y32, "batchnorm_train")
    _is(y32, torch.float32, "batchnorm_train input")
    if y32.dim() != 4 or not 0 < C <= y32.shape[1]:
        raise ValueError(f"batchnorm_train: input must be [B, pad8({C}), H, W], got {tuple(y32.shape)}")
    B, Cp, H, W = y32.shape
    ldx = _out_view(y32, y32, "batchnorm_train input")
    if out is None:
        out_dtype = out_dtype or torch.float32
        out = new_nhwc(B, H, W, Cp, out_dtype, y32.device)[:, :C] if Cp != C else new_nhwc(B, H, W, C, out_dtype, y32.device)
    elif out_dtype is not None:
        _is(out, out_dtype, "batchnorm_train out")
    ldy = _out_view(out, y32, "batchnorm_train out", (B, C, H, W))
    cp8 = -(-C // 8) * 8         # the kernel stores (and reads the shortcut in) whole granules up to pad8(C): they must lie inside the pixel
    if out.storage_offset() % ldy + cp8 > ldy:
        raise ValueError(f"batchnorm_train: out needs room for pad8({C}) = {cp8} channels inside each pixel")
    track = bn.track_running_stats and bn.running_mean is not None
    for t in (bn.weight, bn.bias) + ((bn.running_mean, bn.running_var) if track else ()):     # (no running statistics: track_running_stats=False)
        _vec(t, y32, (C,), "batchnorm_train BatchNorm parameters / running statistics")
    rp, ldr, rdt = None, 0, CFT_F32
    if residual is not None:
        if residual.dtype not in (out.dtype, torch.float32):
            raise TypeError(f"batchnorm_train: residual is {residual.dtype}, expected the output dtype {out.dtype} or float32")
        ldr, rp, rdt = _out_view(residual, y32, "batchnorm_train residual", (B, C, H, W)), residual.data_ptr(), _dt(residual.dtype)
        if residual.storage_offset() % ldr + cp8 > ldr:
            raise ValueError(f"batchnorm_train: residual needs room for pad8({C}) = {cp8} channels inside each pixel")
    lib = _lib.load()
    M = B * H * W
    ws = torch.empty((lib.cft_batchnorm_train_workspace(M, C),), dtype=torch.uint8, device=y32.device)
    if bn.momentum is not None:
        mom = float(bn.momentum)
    else:   # torch: momentum=None is the cumulative moving average, factor 1 / num_batches_tracked (after the increment)
        mom = 1.0 / (int(bn.num_batches_tracked) + 1) if (track and bn.num_batches_tracked is not None) else 0.0
    st = lib.cft_batchnorm_train(y32.data_ptr(), ldx, 0, M, C, bn.weight.data_ptr(), bn.bias.data_ptr(),
                                 bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None,
                                 mom, float(bn.eps), rp, ldr, 0, rdt, out.data_ptr(), ldy, 0, act, _dt(out.dtype),
                                 ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "cft_batchnorm_train")
    if track and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return out
