"""Measure the JPEG decoder (csrc/jpeg.hip, utils/jpeg.py) against PIL and write the results as markdown.

    python tools/jpeg_bench.py [--host-only] [--pairs 128] [--passes 3] [--windows 5] [--out profiles/jpeg_decode.md]

Three parts, one run:
  1. host, one thread: cft_jpeg_entropy (Huffman half only, into preallocated buffers) against PIL's full decode of the same bytes
     (``np.array(Image.open(...).convert('RGB'))`` from memory); needs no GPU (``--host-only`` stops here);
  2. device: cft_jpeg_decode_u8 on 64 pairs (128 files) of 640 x 512 whose coefficients are already on the device - HIP events
     around the call, warm-up, median of ``--runs``;
  3. loader: the sustained rate of create_dataloader_rgb_ir over ``--pairs`` JPEG pairs of 640 x 512, rect=True, batch 64, 16 threads,
     uncached, with decode='pil' (the behaviour without this decoder) and decode='device' alternating in one process on the same files.
The files are synthesised: the fixture images of tests/golden/dataset enlarged to 640 x 512 (bicubic) plus Gaussian noise (sigma 6),
RGB saved at quality 90 4:2:0, IR as grayscale quality 90.  Entropy-decode cost grows with the bits per pixel, so it depends on
content and quality: other files give other numbers.  Prints one JSON line."""
import argparse
import io
import json
import os
import platform
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msod_amd  # noqa: E402,F401
from msod_amd.utils import jpeg as J  # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "golden", "dataset")
W0, H0 = 640, 512


def write_dataset(root, pairs):
    from PIL import Image
    rng = np.random.RandomState(0)
    names = sorted(os.listdir(os.path.join(FIXTURES, "rgb", "images")))
    for stream in ("rgb", "ir"):
        os.makedirs(os.path.join(root, stream, "images"))
        os.makedirs(os.path.join(root, stream, "labels"))
    for k in range(pairs):
        for stream in ("rgb", "ir"):
            with Image.open(os.path.join(FIXTURES, stream, "images", names[k % len(names)])) as im:
                a = np.asarray(im.convert("RGB").resize((W0, H0), Image.BICUBIC), dtype=np.float32)
            a = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
            path = os.path.join(root, stream, "images", f"pair{k:04d}.jpg")
            if stream == "rgb":
                Image.fromarray(a).save(path, quality=90, subsampling=2)
            else:
                Image.fromarray(a).convert("L").save(path, quality=90)
            with open(os.path.join(root, stream, "labels", f"pair{k:04d}.txt"), "w") as f:
                f.write("0 0.5 0.5 0.25 0.25\n")


def read_blobs(root, pairs):
    blobs = []
    for k in range(pairs):
        for stream in ("rgb", "ir"):
            with open(os.path.join(root, stream, "images", f"pair{k:04d}.jpg"), "rb") as f:
                blobs.append(f.read())
    return blobs


def host_part(blobs, passes):
    from PIL import Image
    infos = [J.jpeg_info(b) for b in blobs]
    assert all(i is not None for i in infos)
    bufs = [(np.empty(int(i["ncoef"]), np.int16), np.empty(192, np.uint16)) for i in infos]
    res = {}
    for kind, sel in (("rgb_420", slice(0, None, 2)), ("ir_gray", slice(1, None, 2))):
        bs, is_, fs = blobs[sel], infos[sel], bufs[sel]
        ent, pil = [], []
        for _ in range(passes):
            t0 = time.perf_counter()
            for b, i, (c, q) in zip(bs, is_, fs):
                assert J.jpeg_entropy(b, i, c, q)
            t1 = time.perf_counter()
            for b in bs:
                with Image.open(io.BytesIO(b)) as im:
                    np.array(im.convert("RGB"))
            t2 = time.perf_counter()
            ent.append((t1 - t0) / len(bs) * 1e3)
            pil.append((t2 - t1) / len(bs) * 1e3)
        res[kind] = {"files": len(bs), "kbytes_per_file": round(sum(len(b) for b in bs) / len(bs) / 1024, 1),
                     "entropy_ms": round(min(ent), 3), "pil_full_decode_ms": round(min(pil), 3), "ratio": round(min(ent) / min(pil), 3)}
    return res


def device_part(blobs, runs):
    import torch
    dev = torch.device("cuda:0")
    infos = [J.jpeg_info(b) for b in blobs]
    plan = J.decode_plan(infos)
    total = plan.upload_bytes
    pinned = torch.empty(total, dtype=torch.uint8).pin_memory()
    for k, (b, i) in enumerate(zip(blobs, infos)):
        assert J.entropy_staged(b, i, pinned.numpy(), plan, k)
    staged = pinned.to(dev)
    outs = [torch.empty((int(i["height"]), int(i["width"]), 3), dtype=torch.uint8, device=dev) for i in infos]
    table = np.zeros(len(blobs), dtype=J.JPEG_DESC)
    planes = J.fill_decode_rows(table, plan, infos, range(len(blobs)), staged.data_ptr(), [(o.data_ptr(), o.stride(0)) for o in outs])
    table_host = torch.from_numpy(table.view(np.uint8).reshape(-1)).pin_memory()
    table_dev = table_host.to(dev)
    ws = torch.empty(planes, dtype=torch.uint8, device=dev)
    fn = lambda: J.jpeg_decode_u8(table_dev, table_host, len(blobs), ws)  # noqa: E731
    for _ in range(5):
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
    from PIL import Image
    for k in (0, 1, len(blobs) - 1):
        with Image.open(io.BytesIO(blobs[k])) as im:
            assert np.array_equal(outs[k].cpu().numpy(), np.array(im.convert("RGB"))), "device decode differs from PIL"
    return {"files": len(blobs), "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "runs": runs,
            "upload_mbytes": round(total / 2 ** 20, 1), "output_mbytes": round(sum(o.numel() for o in outs) / 2 ** 20, 1),
            "device": f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}"}


def loader_part(root, pairs, windows, reps=5):
    """Both decoders in one process on the same files: after one warm-up pass each, ``windows`` timed windows per decoder, alternating
    pil / device; a window is ``reps`` consecutive passes over the dataset and ends in a device synchronise."""
    import contextlib
    import torch
    from msod_amd.utils import datasets as D
    loaders, rates = {}, {"pil": [], "device": []}
    for decode in rates:
        with contextlib.redirect_stdout(io.StringIO()):
            loader, _ = D.create_dataloader_rgb_ir(os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), 640, 64, 32,
                                                   SimpleNamespace(single_cls=False), rect=True, workers=16)
        loaders[decode] = D.use_device_jpeg(loader, enabled=decode == "device")
        for _ in loader:                                 # warms the staging buffers up; not counted
            pass
    for _ in range(windows):
        for decode, loader in loaders.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for _ in range(reps):
                for img, _, _, _ in loader:
                    n += img.shape[0]
            torch.cuda.synchronize()
            rates[decode].append(n / (time.perf_counter() - t0))
    res = {k: {"pairs_per_s_median": round(statistics.median(v), 1), "pairs_per_s_windows": [round(r, 1) for r in v]} for k, v in rates.items()}
    res["pairs_per_window"] = pairs * reps
    res["device_over_pil"] = round(res["device"]["pairs_per_s_median"] / res["pil"]["pairs_per_s_median"], 3)
    return res


def markdown(r):
    L = ["# JPEG decoding: host Huffman half, device pixel half, against PIL", "",
         f"Written by `tools/jpeg_bench.py`: ONE run on one box ({r['host']}, the loader on 16 decode threads"
         + (f", {r['device']['device']}" if "device" in r else ", no GPU: host part only") + ").  Files: the fixture images of",
         "tests/golden/dataset enlarged to 640 x 512 (bicubic) plus Gaussian noise (sigma 6); RGB saved by PIL at quality 90 4:2:0, IR as",
         "grayscale quality 90.  Entropy-decode cost follows the bits per pixel, so other content or quality gives other numbers.", "",
         "## 1. Host, one thread: `cft_jpeg_entropy` against PIL's full decode", "",
         "| files | KiB / file | cft_jpeg_entropy ms / file | PIL full decode ms / file | ratio |", "|---|---|---|---|---|"]
    for k, v in r["host_part"].items():
        L.append(f"| {v['files']} {k} | {v['kbytes_per_file']} | {v['entropy_ms']} | {v['pil_full_decode_ms']} | {v['ratio']} |")
    L += ["", "Best of the passes, files read from memory.  PIL's figure includes its IDCT, upsampling, colour conversion, `convert('RGB')` and",
          "`np.array`; ours is the half that stays on the host."]
    if "device" in r:
        d = r["device"]
        L += ["", "## 2. Device: `cft_jpeg_decode_u8`, 64 pairs of 640 x 512 in one call", "",
              f"{d['files']} files, {d['upload_mbytes']} MiB of coefficients and tables in, {d['output_mbytes']} MiB of RGB out: median {d['median_ms']} ms, "
              f"min {d['min_ms']} ms over {d['runs']} runs (HIP events around the call, 5 warm-up calls), two launches.  Every run reads and writes the",
              "same buffers, so the planes and part of the input can stay in the 256 MiB Infinity Cache: a call on freshly uploaded coefficients,",
              "as in the loader, was not timed on its own."]
        lo = r["loader"]
        L += ["", "## 3. Loader: `create_dataloader_rgb_ir`, uncached, rect=True, batch 64, 16 threads", "",
              f"Timed windows of {lo['pairs_per_window']} pairs each (consecutive passes over the same files, host clock, device synchronise at both ends),",
              "the two decoders alternating in one process after one warm-up pass each.", "",
              "| decode | pairs/s (median) | windows |", "|---|---|---|",
              f"| 'pil' (the behaviour without this decoder) | {lo['pil']['pairs_per_s_median']} | {lo['pil']['pairs_per_s_windows']} |",
              f"| 'device' | {lo['device']['pairs_per_s_median']} | {lo['device']['pairs_per_s_windows']} |", "",
              f"device / pil = {lo['device_over_pil']}" + ("" if lo["device_over_pil"] > 1 else ": the device path is NOT faster than PIL on this box and these files.")]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.md"))
    a = ap.parse_args()
    res = {"host": platform.processor() or platform.machine()}
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, a.pairs)
        blobs = read_blobs(root, min(a.pairs, 64))
        res["host_part"] = host_part(blobs, a.passes)
        if not a.host_only:
            res["device"] = device_part(blobs, a.runs)
            res["loader"] = loader_part(root, a.pairs, a.windows)
    with open(a.out, "w") as f:
        f.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
