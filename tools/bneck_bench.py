"""Time cft_bottleneck against the two cft_conv2d launches it replaces.
    python tools/bneck_bench.py [C] [--fused-only] [--iters N]    C = 64 (160x160 stage) or 128 (80x80 stage), batch 64
--fused-only skips the two-launch timing: the fused kernel alone, as a counter run wants it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msod_amd  # noqa: E402,F401
from msod_amd import ops  # noqa: E402


def timeit(fn, iters=20, repeats=3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    ap = argparse.ArgumentParser()
    ap.add_argument("C", type=int, nargs="?", default=64, choices=(64, 128))
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--iters", type=int, default=20, help="launches per timing of the fused kernel")
    args = ap.parse_args()
    C, iters = args.C, args.iters
    B, H, W = (64, 160, 160) if C == 64 else (64, 80, 80)
    cat = ops.new_nhwc(B, H, W, 2 * C, torch.bfloat16, dev)
    cat.copy_(torch.randn(cat.shape, device=dev))
    x = cat[:, :C]
    pk1 = ops.pack_conv(torch.randn(C, C, 1, 1, generator=g) / C ** 0.5, torch.randn(C, generator=g) * 0.1, torch.bfloat16, device=dev)
    pk2 = ops.pack_conv(torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5), torch.randn(C, generator=g) * 0.1, torch.bfloat16, device=dev)
    out = ops.new_nhwc(B, H, W, C, torch.bfloat16, dev)
    t = ops.new_nhwc(B, H, W, C, torch.bfloat16, dev)
    flops = 2.0 * B * H * W * C * C * 10
    res = {"C": C, "gflop": flops / 1e9}
    if not args.fused_only:
        us = timeit(lambda: ops.conv2d(ops.conv2d(x, pk1, 1, out=t), pk2, 1, residual=x, out=out))
        res["two_launches_us"] = round(us, 1)
        print(f"two launches: {us:.1f} us  ({flops / us / 1e6:.0f} TFLOP/s)")
    us = timeit(lambda: ops.bottleneck(x, pk1, pk2, True, out=out), iters=iters)
    res["fused_us"] = round(us, 1)
    print(f"fused: {us:.1f} us  ({flops / us / 1e6:.0f} TFLOP/s)")
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    json.dump(res, open(os.path.join(ROOT, "gpurun_out", f"bneck_bench_c{C}.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
