"""The fused Bottleneck kernels after their instruction diet (csrc/bottleneck.hip, profiles/bottleneck_valu.md): every address the
diet re-derived - x requests redirected to the zero page, zero-written padding of the t patch, the precomputed patch addresses of
the 3x3 taps, 32-bit shortcut / store offsets, tile ids divided by reciprocal - against the two cft_conv2d launches, bit for bit.

Shapes are the smallest at which each path can go wrong (128 channels: 8 x 16-pixel tiles, 64 channels: 16 x 16): one full tile, a
1-pixel ragged row and column of tiles, a map smaller than a tile, an interior tile with all eight neighbours, and a map with a
ragged tile in both directions.  B = 2 makes a tile's successor lie in the next image; x and y are the two channel halves of one
2C-wide buffer, so both strides differ from C and the offsets are not zero."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B = 2
SHAPES = {128: [(8, 16), (9, 17), (7, 5), (16, 48), (24, 18)],
          64: [(16, 16), (17, 33), (5, 7), (48, 48), (18, 20)]}
CASES = [(C, hw) for C in (128, 64) for hw in SHAPES[C]]


def _packs(ops, C, dtype, dev):
    g = torch.Generator().manual_seed(100 + C)
    # biases well away from 0: SiLU(b1) != 0, so a halo pixel outside the image that is not forced to t = 0 shows in the border
    pk1 = ops.pack_conv(torch.randn(C, C, 1, 1, generator=g) / C ** 0.5, torch.randn(C, generator=g) * 0.5 + 0.25, dtype, device=dev)
    pk2 = ops.pack_conv(torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5), torch.randn(C, generator=g) * 0.5, dtype, device=dev)
    return pk1, pk2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shortcut", [True, False], ids=["shortcut", "plain"])
@pytest.mark.parametrize("C,hw", CASES, ids=[f"c{C}-{h}x{w}" for C, (h, w) in CASES])
def test_bottleneck_diet_is_bit_identical(dev, C, hw, shortcut, dtype):
    from msod_amd import ops
    H, W = hw
    pk1, pk2 = _packs(ops, C, dtype, dev)
    g = torch.Generator().manual_seed(7 * H + W)
    wide = ops.new_nhwc(B, H, W, 2 * C, dtype, dev)
    wide.copy_(torch.randn(wide.shape, generator=g).to(dev))
    x, y = wide[:, :C], wide[:, C:]
    x_before = x.float().cpu()
    assert ops.bottleneck_kernel_covers(x, pk1, pk2, 1, 1)
    want = ops.conv2d(ops.conv2d(x, pk1, 1), pk2, 1, residual=x if shortcut else None).float().cpu()
    ops.bottleneck(x, pk1, pk2, shortcut, out=y)          # y starts as noise: a pixel the kernel does not store stays wrong
    torch.cuda.synchronize()
    assert torch.equal(y.float().cpu(), want)
    assert torch.equal(x.float().cpu(), x_before), "input slice untouched"
