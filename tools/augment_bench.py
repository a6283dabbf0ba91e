"""Time cft_augment_batch_u8 on one all-mosaic uint8 [64, 6, 640, 640] training batch and, in the same run, cft_pair_batch_u8 at the
same output size.

    python tools/augment_bench.py [--batch 64] [--size 640] [--runs 30] [--save DIR]

A synthetic on-disk dataset of 640 x 512 PNG pairs with random boxes is written to a temporary directory; the augmented loader
(hyp.scratch values: mosaic 1.0, scale 0.5, translate 0.1, HSV, fliplr 0.5) plans its first batch, the originals are made
device-resident, and the one launch is timed with HIP events (warm-up, median and minimum of ``--runs``); table and look-up tables are
uploaded outside the timed region.  The validation launch letterboxes the same originals to the same [B, 6, size, size].  ``--save DIR``
writes the first three batches of the loader as train_batch{0,1,2}.jpg through ``plot_images``, as train.py:339-342 does.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.ops import augment_batch_u8, pair_batch_u8  # noqa: E402
from msod_amd.utils import datasets as D  # noqa: E402

HYP = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 0.0, "translate": 0.1, "scale": 0.5, "shear": 0.0, "perspective": 0.0,
       "flipud": 0.0, "fliplr": 0.5, "mosaic": 1.0}


def timed(fn, runs, warmup=5):
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
    return statistics.median(ms), min(ms)


def write_dataset(root, n, w0=640, h0=512):
    from PIL import Image
    g = np.random.RandomState(0)
    y, x = np.mgrid[0:h0, 0:w0]
    for stream in ("rgb", "ir"):
        os.makedirs(os.path.join(root, stream, "images"))
        os.makedirs(os.path.join(root, stream, "labels"))
    for k in range(n):
        boxes = [(g.randint(0, 3), g.uniform(0.2, 0.8), g.uniform(0.2, 0.8), g.uniform(0.05, 0.3), g.uniform(0.05, 0.3)) for _ in range(6)]
        for stream in ("rgb", "ir"):
            img = ((x * (k % 5 + 1) + y * (k % 3 + 1))[..., None] + g.randint(0, 32, (h0, w0, 3))).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, stream, "images", f"{k:04d}.png"), compress_level=1)
            with open(os.path.join(root, stream, "labels", f"{k:04d}.txt"), "w") as f:
                f.writelines("%d %.4f %.4f %.4f %.4f\n" % b for b in boxes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--save", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, max(B, 3 * 16 if a.save else B))
        paths = os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images")
        opt = SimpleNamespace(single_cls=False)
        loader, ds = D.create_train_dataloader_rgb_ir(*paths, S, B, 32, opt, HYP, workers=16)
        plans = loader.plan_batch(0, 0)
        sources = {k: tuple(torch.from_numpy(x).to(dev) for x in ds.load_pair(k)) for k in sorted({t["index"] for p in plans for t in p["tiles"]})}
        table, luts, (H, W) = D.build_augment_descriptors(plans)
        D._fill_aug_sources(table, plans, sources)
        host = torch.from_numpy(table.view(np.uint8).reshape(B, -1)).pin_memory()
        table_dev, luts_dev = host.to(dev), torch.from_numpy(luts).to(dev)
        out = torch.empty((B, 6, H, W), dtype=torch.uint8, device=dev)
        aug = timed(lambda: augment_batch_u8(table_dev, host, luts_dev, out), a.runs)

        # the validation launch at the same output size: the same originals letterboxed into [B, 6, S, S]
        val, _ = D.create_dataloader_rgb_ir(*paths, S, B, 32, opt)
        desc, HW = val.dataset.build_descriptors(val.batch_indices(0))
        D._fill_sources(desc, [sources.get(i) or tuple(torch.from_numpy(x).to(dev) for x in ds.load_pair(i)) for i in val.batch_indices(0)])
        vhost = torch.from_numpy(desc.view(np.uint8).reshape(B, -1)).pin_memory()
        vdev, vout = vhost.to(dev), torch.empty((B, 6, HW[0], HW[1]), dtype=torch.uint8, device=dev)
        pair = timed(lambda: pair_batch_u8(vdev, vhost, vout), a.runs)

        res = {"batch": [B, 6, H, W], "originals": "640x512", "mosaic_rows": sum(p["mosaic"] for p in plans), "distinct_pairs": len(sources),
               "augment_ms_median": round(aug[0], 4), "augment_ms_min": round(aug[1], 4), "augment_Mpix_per_s": round(B * H * W / aug[0] / 1e3, 1),
               "pair_batch": [B, 6, HW[0], HW[1]], "pair_batch_ms_median": round(pair[0], 4), "pair_batch_ms_min": round(pair[1], 4),
               "ratio": round(aug[0] / pair[0], 2)}
        if a.save:
            from msod_amd.utils.plots import plot_images
            os.makedirs(a.save, exist_ok=True)
            small, _ = D.create_train_dataloader_rgb_ir(*paths, S, 16, 32, opt, HYP, workers=16)
            for b, (img, targets, files, _) in enumerate(small):
                if b == 3:
                    break
                plot_images(img, targets, files, os.path.join(a.save, f"train_batch{b}.jpg"))
            res["saved"] = sorted(f for f in os.listdir(a.save) if f.startswith("train_batch"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
