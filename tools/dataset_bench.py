"""Time the assembly of one uint8 [64, 6, 512, 640] RGB + IR batch from device-resident originals.

    python tools/dataset_bench.py [--batch 64] [--runs 30] [--loader]

Two batches: 640 x 512 originals (copy mode, the FLIR-aligned case) and 1280 x 1024 originals (INTER_AREA, integer scale 2; and
1279 x 1023, the fractional path).  Each is assembled (a) by ONE cft_pair_batch_u8 launch and (b) the way the package did it before
that kernel existed: the ``letterbox_pair`` loop, two cft_letterbox_u8 launches per pair - for the 1280 x 1024 originals that loop
computes cv2's INTER_LINEAR, not INTER_AREA (it has no area mode), so it is a cost comparison only.  HIP events around the whole
batch, warm-up, median of ``--runs`` timed runs.  ``--loader`` adds the sustained rate of the PairLoader in pairs/s over a synthetic
on-disk dataset of 128 pairs of 640 x 512 PNGs (written to a temporary directory), uncached and device-cached.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.ops import pair_batch_u8  # noqa: E402
from msod_amd.utils import datasets as D  # noqa: E402


# the augmentation hyper-parameters of the reference's data/hyp.scratch.yaml
AUGMENT_HYP = dict(mosaic=1.0, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.0, fliplr=0.5)


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


def batch_case(B, h0, w0, h, w, mode, dev, runs):
    H, W = 512, 640
    g = torch.Generator(device="cpu").manual_seed(h0 + w0)
    src = [tuple(torch.randint(0, 256, (h0, w0, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(2)) for _ in range(B)]
    desc = np.zeros(B, D.PAIR_DESC)
    top, left = (H - h) // 2, (W - w) // 2
    for r in desc:
        r["h0"], r["w0"], r["h"], r["w"], r["top"], r["left"], r["mode"] = h0, w0, h, w, top, left, mode
    D._fill_sources(desc, src)
    host = torch.from_numpy(desc.view(np.uint8).reshape(B, -1)).pin_memory()
    table = host.to(dev)
    out = torch.empty((B, 6, H, W), dtype=torch.uint8, device=dev)
    one = timed(lambda: pair_batch_u8(table, host, out), runs)
    # the letterbox_pair loop sees what the reference's letterbox sees: BGR images; it resizes (linear) when the source is larger
    loop_out = torch.empty((B, 6, H, W), dtype=torch.uint8, device=dev)

    def loop():
        for b, (rgb, ir) in enumerate(src):
            D.letterbox_pair(rgb, ir, new_shape=(H, W), stride=32, auto=False, scaleup=False, out=loop_out[b])
    per_pair = timed(loop, runs)
    moved = B * 2 * (h0 * w0 * 3) + B * 6 * H * W
    return {"source": f"{w0}x{h0}", "resized": f"{w}x{h}", "mode": D.PAIR_MODE_NAMES[mode], "one_launch_ms_median": round(one[0], 4),
            "one_launch_ms_min": round(one[1], 4), "letterbox_pair_loop_ms_median": round(per_pair[0], 4), "letterbox_pair_loop_ms_min": round(per_pair[1], 4),
            "bytes_moved": moved, "one_launch_GBps": round(moved / one[0] / 1e6, 1), "speedup": round(per_pair[0] / one[0], 2)}


def loader_rate(B, dev, passes=2):
    from PIL import Image
    g = np.random.RandomState(0)
    with tempfile.TemporaryDirectory() as root:
        for stream in ("rgb", "ir"):
            os.makedirs(os.path.join(root, stream, "images"))
        y, x = np.mgrid[0:512, 0:640]
        for k in range(128):
            for stream in ("rgb", "ir"):
                img = ((x * (k % 5 + 1) + y * (k % 3 + 1))[..., None] + g.randint(0, 32, (512, 640, 3))).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(root, stream, "images", f"{k:04d}.png"), compress_level=1)
        out = {}
        rgb, ir, opt = os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), SimpleNamespace(single_cls=False)

        def rate(key, loader, pairs):
            rates = []
            for _ in range(passes + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in loader:
                    pass
                torch.cuda.synchronize()
                rates.append(pairs / (time.perf_counter() - t0))
            out[key + "_pairs_per_s"] = round(statistics.median(rates[1:]), 1)       # the first pass warms up (and fills the cache)
            out[key + "_first_pass_pairs_per_s"] = round(rates[0], 1)

        for name, cache in (("uncached", False), ("device_cached", 'device')):
            loader, ds = D.create_dataloader_rgb_ir(rgb, ir, 640, B, 32, opt, pad=0.5, rect=True, cache=cache, workers=16)
            rate(name, loader, len(ds))
            # the training loader: mosaics of four pairs each (no labels in this tree), so a pass decodes most pairs several times uncached
            loader, ds = D.create_train_dataloader_rgb_ir(rgb, ir, 640, B, 32, opt, AUGMENT_HYP, cache=cache, workers=16)
            rate("augmented_" + name, loader, len(ds))
        pairs = D.LoadImagePairs(rgb, ir, 640, 32, batch_size=B, workers=16, device=dev)
        rate("detect", pairs, len(pairs.pairs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--loader", action="store_true")
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "batch": opt.batch, "runs": opt.runs, "cases": [
        batch_case(opt.batch, 512, 640, 512, 640, D.PAIR_COPY, dev, opt.runs),
        batch_case(opt.batch, 1024, 1280, 512, 640, D.PAIR_AREA, dev, opt.runs),
        batch_case(opt.batch, 1023, 1279, 511, 639, D.PAIR_AREA, dev, opt.runs)]}
    if opt.loader:
        res["loader"] = loader_rate(opt.batch, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
