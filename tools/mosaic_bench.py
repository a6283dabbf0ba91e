"""Time the stages of plot_images on one [16, 6, 512, 640] uint8 batch with 300 predictions per image (the padded NMS form).

    python tools/mosaic_bench.py [--runs 30] [--dets 300] [--no-host]

Prints one JSON line; every ``*_ms`` is the median of ``--runs`` timed runs and ``*_ms_min`` their minimum:
  compose_ms    cft_mosaic_compose for both streams (each with its maximum reduction in front);
  slots_ms      cft_mosaic_slots, output_to_target fused in;
  render_ms     cft_detect_render over the 16 cells of both mosaics (thickness 3, labels with ' d.d');
  finish_ms     cft_mosaic_finish: file names and borders, both mosaics in one launch;
  area_ms       cft_mosaic_area of both 2048 x 2560 mosaics to 1024 x 1280;
  d2h_ms        the two device-to-host copies of the reduced mosaics;
  host_loop_ms  the numpy restatement of the whole function on the same input (tests/mosaic_ref.py), wall clock, one run.
HIP events around each stage, warm-up first.  Record the line in profiles/mosaic.md when it has been run on an MI355X; nothing in the
documents rests on it until then."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msod_amd  # noqa: E402,F401
from msod_amd import ops  # noqa: E402
from msod_amd.utils import plots as P  # noqa: E402


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
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    opt = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, C, H, W, n, names = 16, 6, 512, 640, opt.dets, ["person", "car", "bicycle"]
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (B, C, H, W), dtype=np.uint8)
    x1, y1 = rng.uniform(0, W - 8, (B, n)), rng.uniform(0, H - 8, (B, n))
    dets = np.stack([x1, y1, x1 + rng.uniform(4, 200, (B, n)), y1 + rng.uniform(4, 200, (B, n)), np.sort(rng.uniform(0, 1, (B, n)))[:, ::-1],
                     rng.integers(0, len(names), (B, n))], 2).astype(np.float32)
    counts = np.full((B,), n, np.int32)
    paths = [f"/data/val/images/{i:06d}.jpg" for i in range(B)]
    img_d, pair = torch.from_numpy(images).to(dev), (torch.from_numpy(dets).to(dev), torch.from_numpy(counts).to(dev))

    g = P.mosaic_geometry(B, H, W)
    rnd = P._mosaic_renderer(tuple(names), dev)
    mosaics = [torch.empty((g.ns * g.h, g.ns * g.w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    maxkey = torch.empty((1,), dtype=torch.int32, device=dev)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    codes, lens = P._path_codes(paths, g.bs, dev)

    def compose():
        for s, m in enumerate(mosaics):
            ops.mosaic_compose(img_d, 3 * s, g.bs, g.ns, g.h, g.w, g.resize, m, maxkey)
    compose()
    slots, _ = ops.mosaic_slots(pair, g.bs, n, len(names), g.h, g.w, g.sf, flag)
    desc_dev, desc_host = P.cell_descriptors(mosaics, g)
    res = {"batch": f"{B}x{C}x{H}x{W} uint8", "dets_per_image": n, "mosaic": f"{g.ns * g.w}x{g.ns * g.h}", "saved": f"{g.out_w}x{g.out_h}"}

    def put(key, pair_):
        res[key + "_ms"], res[key + "_ms_min"] = pair_
    put("compose", timed(compose, opt.runs))
    put("slots", timed(lambda: ops.mosaic_slots(pair, g.bs, n, len(names), g.h, g.w, g.sf, flag), opt.runs))
    put("render", timed(lambda: P.detect_render(desc_dev, desc_host, slots, rnd.colors, rnd.text_color, 3, P.mosaic_render_flags(True), rnd.names,
                                                rnd.name_len, rnd.atlas), opt.runs))
    put("finish", timed(lambda: ops.mosaic_finish(mosaics[0], mosaics[1], g.bs, g.ns, g.h, g.w, codes, lens, rnd.atlas), opt.runs))
    put("area", timed(lambda: [ops.mosaic_area(m, g.out_h, g.out_w) for m in mosaics], opt.runs))
    small = [ops.mosaic_area(m, g.out_h, g.out_w) for m in mosaics]
    put("d2h", timed(lambda: [m.cpu() for m in small], opt.runs))
    put("plot_images_device", timed(lambda: P.plot_images_device(img_d, pair, paths, names), opt.runs))
    if not opt.no_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import mosaic_ref
        t0 = time.perf_counter()
        mosaic_ref.plot_images_ref(images, (dets, counts), paths, names, atlas=P.glyph_atlas(), cap=n)
        res["host_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
