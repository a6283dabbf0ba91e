"""The per-element oracles of ``exact_ref`` checked on the CPU: on seeded conv / attention outputs computed on the host the way the
kernels compute them, each of a set of plausible kernel mistakes is REJECTED by the per-element check (bound + correct-rounding rate)
while ``helpers.rel_err`` within ``helpers.tol`` still ACCEPTS it.  Plus a known answer of the dropout hash replica and a static check
of the asm GEMM's accumulator registers in the compiler's output."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
import helpers
from helpers import rel_err, tol

FLOOR = {torch.bfloat16: 0.99, torch.float16: 0.95}      # host-side floors (the device floors live in test_gpu_kernel_oracles.py)


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


LOW_BIAS = {torch.bfloat16: 0.01, torch.float16: 0.002, torch.float32: 1e-5}     # what rel_err cannot see at each tol(dtype)


def _conv_case(dtype, seed=0):
    """3x3 conv, 64 -> 32 channels, ragged M; channel 5 is a low-magnitude channel (tiny weights, bias LOW_BIAS) and the last
    image row carries small activations.  -> (x, w, b, ref64 [M, N], absacc, fp32 result [M, N] as the kernel forms it)."""
    B, C, H, W, N = 2, 64, 9, 11, 32
    x = _rnd(B, C, H, W, seed=seed)
    x[-1, :, -2:, :] *= 0.1
    x = x.to(dtype).float()
    w = _rnd(N, C, 3, 3, seed=seed + 1, scale=0.9 / math.sqrt(C * 9))     # (keeps the maximum, 3.4, near the top of its binade)
    w[5] *= 0.002
    w = w.to(dtype).float()
    b = _rnd(N, seed=seed + 2, scale=0.1)
    b[5] = LOW_BIAS[dtype]
    ref, absacc, _ = X.conv_ref(x, w, b, 1)
    y32 = F.conv2d(x, w, b, 1, 1).permute(0, 2, 3, 1).reshape(-1, N).double().numpy()      # fp32 accumulation
    return ref, absacc, y32, C * 9


def _judge(got, ref, absacc, K, dtype):
    bound = X.gemm_bound(ref, absacc, K, dtype)
    per_element = X.passes(got, ref, bound, dtype, FLOOR[dtype])
    loose = rel_err(torch.as_tensor(got), torch.as_tensor(ref)) < tol(dtype)
    return per_element, loose


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_correct_kernel_output_passes(dtype):
    ref, absacc, y32, K = _conv_case(dtype)
    good = X.rne(y32, dtype)
    assert _judge(good, ref, absacc, K, dtype) == (True, True)
    r = X.check(good, ref, X.gemm_bound(ref, absacc, K, dtype), dtype)
    assert r["rate"] > 0.995


def test_rne_is_one_rounding():
    """rne() matches torch's conversion from fp32 inputs and rounds ties to even."""
    x = _rnd(100000, seed=3).numpy().astype(np.float32)
    for dt in (torch.bfloat16, torch.float16):
        assert np.array_equal(X.rne(x.astype(np.float64), dt), torch.from_numpy(x).to(dt).double().numpy())
    assert X.rne(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]), torch.bfloat16).tolist() == [1.0, 1.0 + 2.0 ** -6]
    assert X.rne(np.array([2.0 ** -25, 3 * 2.0 ** -26]), torch.float16).tolist() == [0.0, 2.0 ** -24]      # subnormal ties


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_mutation_round_toward_zero(dtype):
    ref, absacc, y32, K = _conv_case(dtype)
    assert _judge(X.rtz(y32, dtype), ref, absacc, K, dtype) == (False, True)


def test_mutation_double_rounding_through_fp16():
    dtype = torch.bfloat16
    ref, absacc, y32, K = _conv_case(dtype)
    bad = X.rne(X.rne(y32, torch.float16), torch.bfloat16)
    assert _judge(bad, ref, absacc, K, dtype) == (False, True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_mutation_bias_dropped_on_a_low_magnitude_channel(dtype):
    ref, absacc, y32, K = _conv_case(dtype)
    y = y32.copy()
    y[:, 5] -= LOW_BIAS[dtype]
    assert _judge(X.rne(y, dtype), ref, absacc, K, dtype) == (False, True)


@pytest.mark.parametrize("dtype,factor", [(torch.bfloat16, 1.02), (torch.float16, 1.003)], ids=["bf16", "f16"])
def test_mutation_ragged_edge_row_off(dtype, factor):
    """One row of the ragged last tile 2 % off (bf16; 0.3 % for fp16, whose tol is tighter)."""
    ref, absacc, y32, K = _conv_case(dtype)
    y = y32.copy()
    y[-1] *= factor                    # the last row of the last (ragged) tile
    got = X.rne(y, dtype)
    bound = X.gemm_bound(ref, absacc, K, dtype)
    assert not X.passes(got, ref, bound, dtype)
    assert rel_err(torch.as_tensor(got), torch.as_tensor(ref)) < tol(dtype)


def _attn_operands(dtype, B=2, heads=2, dk=20, dkp=32, sharp=1.0, seed=5):
    q, k, v = (_rnd(B, heads, 128, dkp, seed=seed + i) for i in range(3))
    q[..., dk:] = 0
    k[..., dk:] = 0
    v[..., dk:] = 0
    q, k, v = (t.to(dtype).float() for t in (q * sharp, k, v))
    return q, k, v


def _attn_kernel_like(q, k, v, dk, dtype, keep=None, pdrop=0.0, normalise_first=False):
    """The kernel's fp32 pipeline on the host; ``normalise_first`` = the mutation that rounds P after normalising."""
    scale = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(dk), dtype=torch.float32))
    s = (q @ k.transpose(-1, -2)) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    den = e.sum(-1, keepdim=True)
    if keep is not None:
        e = e * torch.as_tensor(keep, dtype=torch.float32) * float(X.drop_threshold(pdrop)[1])
    if normalise_first:
        o = e.div(den).to(dtype).float() @ v
    else:
        o = (e.to(dtype).float() @ v) * (1.0 / den)
    return o.to(dtype).double().numpy()


def test_attention_model_accepts_the_kernel_pipeline_and_rejects_late_rounding_of_p():
    dtype = torch.bfloat16
    q, k, v = _attn_operands(dtype)
    ref, bound = X.attention_ref(q, k, v, 20, dtype)
    good = _attn_kernel_like(q, k, v, 20, dtype)
    assert X.passes(good, ref, bound, dtype, FLOOR[dtype])
    bad = _attn_kernel_like(q, k, v, 20, dtype, normalise_first=True)
    assert not X.passes(bad, ref, bound, dtype, FLOOR[dtype])
    true_softmax = torch.softmax((q @ k.transpose(-1, -2)).double() / math.sqrt(20), -1) @ v.double()
    assert rel_err(torch.as_tensor(bad), true_softmax) < tol(dtype)


def test_attention_dropout_same_mask_for_every_head_is_rejected():
    """A mask indexed without the head (every head drops the same keys) keeps the drop rate and the unbiasedness that the statistical
    test of GPT dropout checks; the exact host-replicated mask tells it apart."""
    dtype, p, seed = torch.bfloat16, 0.1, 1234
    q, k, v = _attn_operands(dtype, heads=4)
    keep = X.attention_mask(seed, 2, 4, p)
    wrong = np.ascontiguousarray(np.broadcast_to(keep[:, :1], keep.shape))
    assert abs((~wrong).mean() - p) < 0.01 and abs((~keep).mean() - p) < 0.01        # same statistics
    ref, bound = X.attention_ref(q, k, v, 20, dtype, keep=keep, pdrop=p)
    assert X.passes(_attn_kernel_like(q, k, v, 20, dtype, keep=keep, pdrop=p), ref, bound, dtype, FLOOR[dtype])
    assert not X.passes(_attn_kernel_like(q, k, v, 20, dtype, keep=wrong, pdrop=p), ref, bound, dtype, FLOOR[dtype])
    assert not np.array_equal(wrong, keep)


def test_hash_replica_known_answer():
    """splitmix64 seeded with 0: first output 0xE220A8397B1DCDAF (the published test vector); cft_hash32 is its upper half."""
    assert int(X.splitmix64(0, 0)) == 0xE220A8397B1DCDAF
    assert int(X.hash32(0, 0)) == 0xE220A839
    h = X.hash32(0x5EED, np.arange(1 << 16, dtype=np.uint64))
    assert abs(float(h.mean()) / 2 ** 32 - 0.5) < 0.01                      # uniform
    t, inv = X.drop_threshold(0.1)
    assert int(t) == int(float(np.float32(0.1)) * 2 ** 32) and inv == np.float32(1) / np.float32(0.9)


def test_dropout_replica_rounds_once():
    x = _rnd(4096, seed=9).to(torch.bfloat16).float()
    y = X.dropout_ref(x, 77, 0.5, torch.bfloat16)
    keep = X.dropout_mask(77, 4096, 0.5)
    assert np.array_equal(y[~keep], np.zeros((~keep).sum()))
    assert np.array_equal(y[keep], (x.numpy()[keep] * np.float32(2.0)).astype(np.float64))     # x 2 is exact


# ------------------------------------------------------------------------------ asm GEMM accumulators
ASM_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multispectral-object-detection_amd", "csrc", "conv_gemm_asm.hip")
AGPR = re.compile(r"\ba\[?\d+")


def agprs_outside_asm_blocks(text):
    """(instruction lines naming an AGPR operand outside ;;#ASMSTART ... ;;#ASMEND, count inside) of a device .s file."""
    outside, inside, in_block = [], 0, False
    for line in text.splitlines():
        s = line.strip()
        if s.startswith(";;#ASMSTART"):
            in_block = True
            continue
        if s.startswith(";;#ASMEND"):
            in_block = False
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        code = s.split(";")[0]
        parts = code.split(None, 1)
        if len(parts) < 2 or not AGPR.search(parts[1]):
            continue
        if in_block:
            inside += 1
        else:
            outside.append(s)
    return outside, inside


def test_agpr_scan_flags_a_write_outside_an_asm_block():
    text = "\n".join([
        "kern:", ";;#ASMSTART", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]", ";;#ASMEND",
        "\tv_accvgpr_write_b32 a5, v1", "\ts_endpgm"])
    outside, inside = agprs_outside_asm_blocks(text)
    assert inside == 1 and outside == ["v_accvgpr_write_b32 a5, v1"]


@pytest.fixture(scope="module")
def asm_listing():
    return helpers.device_asm(ASM_SRC)


def _expected_kernel_count():
    """What the source instantiates: conv_gemm_asm_kernel<T, MASKED, MT0, MT1> for 2 dtypes x 2 forms x the cases of launch_asm_tile,
    plus every other __global__ of the file once per 16-bit dtype."""
    src = open(ASM_SRC).read()
    body = src[src.index("static int launch_asm_tile("):]
    body = body[:body.index("\n}\n")]
    tiles = len(re.findall(r"return launch_asm_t<", body))
    others = len(re.findall(r"__global__", src)) - 1
    return 2 * 2 * tiles + 2 * others


def test_asm_gemm_accumulators_stay_in_asm_blocks(asm_listing):
    """The asm GEMM keeps its accumulators a0-a127 live across separate inline-asm statements, a dependency the compiler cannot see:
    if it ever allocated an AGPR itself, or spilled, a tile would come out wrong on the GPU.  Check it in the compiler's output: no
    scratch, no spills, no AGPR operand outside an inline-asm block, and every instantiated kernel present."""
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    kernels = _lib.kernel_notes(asm_listing)
    assert len(kernels) == _expected_kernel_count(), sorted(kernels)
    for name, m in kernels.items():
        assert m["private_segment_fixed_size"] == 0, name
        assert m["vgpr_spill_count"] == 0, name
        assert m["sgpr_spill_count"] == 0, name
    outside, inside = agprs_outside_asm_blocks(asm_listing)
    assert outside == [], outside[:10]
    assert inside > 1000
    # The allocation must hold every accumulator the asm names (a0-a127, CONV_ASM_CLOBBERS).  On gfx950, VGPRs and AGPRs share one
    # register file and the AGPRs start at accum_offset, so an under-sized AGPR block would alias the accumulators with other registers.
    hi = max([int(up) for up in re.findall(r"\ba\[\d+:(\d+)\]", asm_listing)] + [int(n) for n in re.findall(r"\ba(\d+)\b", asm_listing)])
    assert hi == 127, hi
    for name, m in kernels.items():
        assert m["agpr_count"] >= hi + 1, (name, m["agpr_count"])
    blocks = re.findall(r"\.amdhsa_next_free_vgpr (\d+)\s*\n(?:.*\n){0,3}?\s*\.amdhsa_accum_offset (\d+)", asm_listing)
    assert len(blocks) == len(kernels)
    for nfv, acc in blocks:
        assert int(nfv) - int(acc) >= hi + 1, (nfv, acc)
