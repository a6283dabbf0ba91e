"""Time the device stage of detect on one batch of 64 pairs of 640 x 512 originals with 300 detections each.

    python tools/detect_bench.py [--batch 64] [--runs 30] [--dets 300]

Prints one JSON line with, per batch of 64:
  boxes_ms_per_64        cft_detect_boxes on the batched_nms output;
  render_ms_per_64       cft_detect_render into both streams' originals (thickness 2, labels with confidence);
  d2h_ms_per_64          the one device-to-host copy of the box buffer;
  python_loop_ms_per_64  the reference-style loop on GPU tensors (detect_twostream.py:129-144: scale_coords, round, unique, and per
                         detection xyxy2xywh / gn and the tolist() round trip), without any drawing.
HIP events around each stage, warm-up, median of ``--runs`` timed runs (the Python loop: wall clock around a synchronised run).
Record the line under profiles/ when it has been run on an MI355X; nothing in the documents rests on it until then."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.ops import detect_boxes  # noqa: E402
from msod_amd.utils.general import scale_coords, xyxy2xywh  # noqa: E402
from msod_amd.utils.metrics import geometry  # noqa: E402
from msod_amd.utils.plots import BoxRenderer  # noqa: E402


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
    return round(statistics.median(ms), 4)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--dets", type=int, default=300)
    opt = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, n, H, W, h0, w0, nc = opt.batch, opt.dets, 512, 640, 512, 640, 3
    g = np.random.default_rng(0)
    x1, y1 = g.uniform(0, W - 8, (B, n)), g.uniform(0, H - 8, (B, n))
    dets = np.stack([x1, y1, x1 + g.uniform(4, 200, (B, n)), y1 + g.uniform(4, 200, (B, n)), np.sort(g.uniform(0, 1, (B, n)))[:, ::-1],
                     g.integers(0, nc, (B, n))], 2).astype(np.float32)
    dets_d = torch.from_numpy(dets).to(dev)
    counts = torch.full((B,), n, dtype=torch.int32, device=dev)
    geom = geometry([((h0, w0), None)] * B, (H, W)).to(dev)
    originals = [tuple(torch.zeros((h0, w0, 3), dtype=torch.uint8, device=dev) for _ in range(2)) for _ in range(B)]
    renderer = BoxRenderer(["person", "car", "bicycle"], dev, 2, hide_conf=False)
    boxes, hist, flag = detect_boxes(dets_d, counts, geom, nc)
    res = {"batch": B, "dets_per_image": n, "original": f"{w0}x{h0}"}
    res["boxes_ms_per_64"] = timed(lambda: detect_boxes(dets_d, counts, geom, nc), opt.runs)
    res["render_ms_per_64"] = timed(lambda: renderer(boxes, [o[0] for o in originals], [o[1] for o in originals]), opt.runs)
    res["d2h_ms_per_64"] = timed(lambda: boxes.cpu(), opt.runs)

    def python_loop():
        lines = 0
        for b in range(B):
            det = dets_d[b].clone()
            det[:, :4] = scale_coords((H, W), det[:, :4], (h0, w0, 3)).round()
            for c in det[:, -1].unique():
                (det[:, -1] == c).sum().item()
            gn = torch.tensor((h0, w0, 3))[[1, 0, 1, 0]].to(dev)
            for *xyxy, conf, cls in reversed(det):
                xywh = (xyxy2xywh(torch.tensor(xyxy, device=dev).view(1, 4)) / gn).view(-1).tolist()
                lines += len(('%g ' * 6).rstrip() % (cls, *xywh, conf))
        return lines
    python_loop()
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        python_loop()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    res["python_loop_ms_per_64"] = round(statistics.median(t), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
