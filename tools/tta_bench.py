"""Time the two test-time-augmentation kernels next to the three forwards they sit between, on one [64, 3, 640, 640] batch.

    python tools/tta_bench.py [--cfg yolov5l] [--batch 64] [--size 640] [--runs 20] [--u8]

Prints one JSON line; every ``*_ms`` is the median of ``--runs`` timed runs and ``*_ms_min`` their minimum:
  view83_ms / view67_ms   cft_tta_view of the mirrored 0.83 view (544 x 544 at 640) and of the 0.67 view (448 x 448);
  merge_ms                cft_tta_merge of the three prediction tensors;
  forward_ms              the three captured forwards (640, 544 and 448 pixels), replayed back to back, bf16 compute;
  augment_ms              model(x, augment=True) as a whole;
  kernels_over_forwards   (view83 + view67 + merge) / forward, medians.
HIP events around each stage, warm-up first.  Record the line in profiles/single_stream.md when it has been run on an MI355X, marked as
one run; no target is set on it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msod_amd  # noqa: E402,F401
from msod_amd import ops  # noqa: E402
from msod_amd.models.yolo import TTA_FLIPS, TTA_SCALES, Model  # noqa: E402
from msod_amd.utils.seeded import seeded_state_dict  # noqa: E402


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4), round(min(ms), 4)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cfg", default="yolov5l")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--u8", action="store_true", help="a uint8 batch, as the loader hands it over, instead of fp32")
    opt = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    model = Model(opt.cfg + ".yaml", nc=3)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    model = model.to(dev).fuse().eval()
    gs = int(model.stride.max())
    B, S = opt.batch, opt.size
    x = torch.rand((B, 3, S, S), generator=torch.Generator().manual_seed(0))
    x = ((x * 255).to(torch.uint8) if opt.u8 else x).to(dev)
    with torch.no_grad():
        graphs = model.capture_augment(B, S, S, x.dtype)
        views = [ops.tta_view(x, s, gs, flip=f == 3) for s, f in zip(TTA_SCALES[1:], TTA_FLIPS[1:])]
        preds = [model(v)[0].clone() for v in [x] + views]
        out = {"cfg": opt.cfg, "batch": B, "size": S, "input": str(x.dtype), "compute": str(model.compute_dtype), "runs": opt.runs,
               "view_shapes": [list(v.shape[2:]) for v in views], "rows": [p.shape[1] for p in preds], "graphs": len(graphs)}
        for key, (s, f, v) in zip(("view83", "view67"), zip(TTA_SCALES[1:], TTA_FLIPS[1:], views)):
            out[key + "_ms"], out[key + "_ms_min"] = timed(lambda: ops.tta_view(x, s, gs, flip=f == 3, out=v), opt.runs)
        merged = torch.empty((B, sum(p.shape[1] for p in preds), preds[0].shape[2]), dtype=torch.float32, device=dev)
        out["merge_ms"], out["merge_ms_min"] = timed(lambda: ops.tta_merge(preds, TTA_SCALES, [f == 3 for f in TTA_FLIPS], S, out=merged), opt.runs)
        out["forward_ms"], out["forward_ms_min"] = timed(lambda: [model(v) for v in [x] + views], opt.runs)
        out["augment_ms"], out["augment_ms_min"] = timed(lambda: model(x, augment=True), opt.runs)
    out["kernels_over_forwards"] = round((out["view83_ms"] + out["view67_ms"] + out["merge_ms"]) / out["forward_ms"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
