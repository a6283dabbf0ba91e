"""Measure the JPEG encoder (csrc/jpeg_encode.hip, utils/jpeg.py) against PIL and write the results as markdown.

    python tools/jpeg_encode_bench.py [--host-only] [--pairs 64] [--passes 3] [--runs 100] [--windows 5] [--out profiles/jpeg_encode.md]

Four parts, one run, every comparison against PIL in the same run:
  1. host, one thread: cft_jpeg_write (headers + Huffman coding of coefficients that are already there, into a preallocated buffer)
     against PIL's whole ``Image.fromarray(a).save(buf, 'JPEG')`` of the same image; needs no GPU (``--host-only`` stops here: the
     coefficients then come from cft_jpeg_entropy of PIL's file);
  2. device: cft_jpeg_encode_coef on 64 pairs (128 images) of 640 x 512 that are already on the device - HIP events around the call,
     warm-up, median of ``--runs``, buffers reused - beside the HBM floor of its traffic;
  3. the copy of those coefficients into pinned memory, HIP events likewise;
  4. detect: images/s of ``detect(opt)`` with saved images over ``--pairs`` .jpg pairs of 640 x 512, batch 8, the tiny fixture checkpoint,
     without and with ``device_jpeg``, alternating in one process on the same files; the written files are compared byte for byte.
The images are synthesised: the fixture images of tests/golden/dataset enlarged to 640 x 512 (bicubic) plus Gaussian noise (sigma 6);
RGB as it is, IR with grey content (R = G = B), both three channels as detect draws them, written at PIL's defaults (quality 75,
4:2:0).  Huffman-coding cost follows the bits per pixel, so it depends on content and quality: other images give other numbers.
Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import platform
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msod_amd  # noqa: E402,F401
from msod_amd import _lib  # noqa: E402
from msod_amd.utils import jpeg as J  # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "golden", "dataset")
CKPT = os.path.join(ROOT, "tests", "golden", "ref_ckpt_tiny.pt")
W0, H0 = 640, 512
HBM_GBYTES_PER_S = 8000.0            # MI355X peak, for the floor quoted beside the device time


def images(pairs):
    """[(rgb, ir)] uint8 [512, 640, 3] arrays."""
    from PIL import Image
    rng = np.random.RandomState(0)
    names = sorted(os.listdir(os.path.join(FIXTURES, "rgb", "images")))
    out = []
    for k in range(pairs):
        pair = []
        for stream in ("rgb", "ir"):
            with Image.open(os.path.join(FIXTURES, stream, "images", names[k % len(names)])) as im:
                im = im.convert("RGB") if stream == "rgb" else im.convert("L").convert("RGB")
                a = np.asarray(im.resize((W0, H0), Image.BICUBIC), dtype=np.float32)
            noise = rng.normal(0, 6, a.shape if stream == "rgb" else a.shape[:2] + (1,))
            pair.append(np.clip(a + noise, 0, 255).astype(np.uint8))
        out.append(tuple(pair))
    return out


def pil_bytes(a):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG")
    return buf.getvalue()


def host_part(imgs, passes):
    lib = _lib.load()
    qtab = J.jpeg_quality_tables(75)
    res = {}
    for kind, sel in (("rgb", 0), ("ir_grey_content", 1)):
        arrs = [p[sel] for p in imgs]
        blobs = [pil_bytes(a) for a in arrs]
        work = []
        for b in blobs:                                    # the coefficients PIL's file holds: what the device half produces
            info = J.jpeg_info(b)
            coef, qt = np.empty(int(info["ncoef"]), np.int16), np.empty(192, np.uint16)
            assert J.jpeg_entropy(b, info, coef, qt) and np.array_equal(qt.reshape(3, 64), qtab)
            work.append((coef, info, np.empty(J.jpeg_write_bound(info), np.uint8)))
        ours, pil = [], []
        import ctypes
        n = ctypes.c_long(0)
        for _ in range(passes):
            t0 = time.perf_counter()
            for coef, info, out in work:
                assert lib.cft_jpeg_write(coef.ctypes.data, qtab.ctypes.data, info.ctypes.data, out.ctypes.data, out.size, ctypes.byref(n)) == 0
            t1 = time.perf_counter()
            for a in arrs:
                pil_bytes(a)
            t2 = time.perf_counter()
            ours.append((t1 - t0) / len(arrs) * 1e3)
            pil.append((t2 - t1) / len(arrs) * 1e3)
        assert all(J.jpeg_write(c, qtab, i) == b for (c, i, _), b in zip(work[:4], blobs[:4])), "cft_jpeg_write differs from PIL"
        res[kind] = {"files": len(arrs), "kbytes_per_file": round(sum(len(b) for b in blobs) / len(blobs) / 1024, 1),
                     "write_ms": round(min(ours), 3), "pil_save_ms": round(min(pil), 3), "ratio": round(min(ours) / min(pil), 3)}
    return res


def _event_ms(fn, runs, warm=5):
    import torch
    for _ in range(warm):
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
    return ms


def device_part(imgs, runs):
    import torch
    dev = torch.device("cuda:0")
    flat = [torch.from_numpy(a).to(dev) for p in imgs for a in p]
    qtab = J.jpeg_quality_tables(75)
    infos = [J.jpeg_layout(W0, H0, 3, 2, 2) for _ in flat]
    per = int(infos[0]["ncoef"])
    coef = torch.empty(per * len(flat), dtype=torch.int16, device=dev)
    pinned = torch.empty(per * len(flat), dtype=torch.int16).pin_memory()
    tabs_host = torch.from_numpy(qtab.view(np.uint8).reshape(-1).copy()).pin_memory()
    tabs_dev = tabs_host.to(dev)
    table = np.zeros(len(flat), dtype=J.JPEG_ENC_DESC)
    for k, (row, t, info) in enumerate(zip(table, flat, infos)):
        row["src"], row["qtab"], row["qtab_host"], row["coef"], row["src_stride"] = t.data_ptr(), tabs_dev.data_ptr(), tabs_host.data_ptr(), coef.data_ptr() + 2 * per * k, t.stride(0)
        J.fill_geometry(row, info)
    table_host = torch.from_numpy(table.view(np.uint8).reshape(-1)).pin_memory()
    table_dev = table_host.to(dev)
    enc = _event_ms(lambda: J.jpeg_encode_coef(table_dev, table_host, len(flat)), runs)
    cp = _event_ms(lambda: pinned.copy_(coef, non_blocking=True), runs)
    torch.cuda.synchronize()
    host = pinned.numpy()
    for k in (0, 1, len(flat) - 1):
        a = flat[k].cpu().numpy()
        assert J.jpeg_write(host[per * k:per * (k + 1)], qtab, infos[k]) == pil_bytes(a), "device encode differs from PIL"
    read_mb, write_mb = sum(t.numel() for t in flat) / 1e6, 2 * per * len(flat) / 1e6
    return {"files": len(flat), "median_ms": round(statistics.median(enc), 4), "min_ms": round(min(enc), 4), "runs": runs,
            "read_mbytes": round(read_mb, 1), "write_mbytes": round(write_mb, 1),
            "hbm_floor_ms": round((read_mb + write_mb) / HBM_GBYTES_PER_S, 4),
            "copy_median_ms": round(statistics.median(cp), 4), "copy_min_ms": round(min(cp), 4),
            "copy_gbytes_per_s": round(write_mb / statistics.median(cp), 1),
            "device": f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}"}


def detect_part(imgs, windows):
    """detect(opt) with saved images, PIL and device encoding alternating on the same files, one warm-up run each."""
    import torch
    from PIL import Image
    from msod_amd import compat
    from msod_amd.detect import detect, make_parser
    rates = {"pil": [], "device": []}
    with tempfile.TemporaryDirectory() as root:
        for stream in ("rgb", "ir"):
            os.makedirs(os.path.join(root, stream))
        for k, (rgb, ir) in enumerate(imgs):
            Image.fromarray(rgb).save(os.path.join(root, "rgb", f"pair{k:04d}.jpg"), quality=90)
            Image.fromarray(ir).save(os.path.join(root, "ir", f"pair{k:04d}.jpg"), quality=90)
        model = compat.attempt_load(CKPT, map_location="cpu")
        last = {}

        def run(kind, name):
            opt = make_parser().parse_args(["--weights", CKPT, "--source1", os.path.join(root, "rgb"), "--source2", os.path.join(root, "ir"), "--img-size", "640",
                                            "--conf-thres", "0.25", "--batch-size", "8", "--project", os.path.join(root, "runs"), "--name", name])
            opt.device_jpeg = kind == "device"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                last[kind] = detect(opt, model=model, log=lambda *_: None)
            torch.cuda.synchronize()
            return 2 * len(imgs) / (time.perf_counter() - t0)
        for kind in rates:
            run(kind, f"warm_{kind}")
        for w in range(windows):
            for kind in rates:
                rates[kind].append(run(kind, f"{kind}{w}"))
        names = sorted(f for f in os.listdir(last["pil"]) if f.endswith(".jpg"))
        assert len(names) == 2 * len(imgs)
        for f in names:
            with open(os.path.join(last["pil"], f), "rb") as a, open(os.path.join(last["device"], f), "rb") as b:
                assert a.read() == b.read(), f"{f}: the device path wrote other bytes than PIL"
    res = {k: {"images_per_s_median": round(statistics.median(v), 1), "images_per_s_windows": [round(r, 1) for r in v]} for k, v in rates.items()}
    res["images_per_window"] = 2 * len(imgs)
    res["device_over_pil"] = round(res["device"]["images_per_s_median"] / res["pil"]["images_per_s_median"], 3)
    return res


def markdown(r):
    L = ["# JPEG encoding: device colour / DCT / quantisation, host Huffman half, against PIL", "",
         f"Written by `tools/jpeg_encode_bench.py`: ONE run on one box ({r['host']}"
         + (f", {r['device']['device']}" if "device" in r else ", no GPU: host part only") + ").  Images: the fixture images of",
         "tests/golden/dataset enlarged to 640 x 512 (bicubic) plus Gaussian noise (sigma 6); RGB in colour, IR with grey content (R = G = B), both three",
         "channels, written at PIL's defaults (quality 75, 4:2:0).  Huffman-coding cost follows the bits per pixel, so other content or quality gives",
         "other numbers.", "",
         "## 1. Host, one thread: `cft_jpeg_write` against PIL's whole `save`", "",
         "| files | KiB / file | cft_jpeg_write ms / file | PIL save ms / file | ratio |", "|---|---|---|---|---|"]
    for k, v in r["host_part"].items():
        L.append(f"| {v['files']} {k} | {v['kbytes_per_file']} | {v['write_ms']} | {v['pil_save_ms']} | {v['ratio']} |")
    L += ["", "Best of the passes, into memory.  PIL's figure includes its colour conversion, downsampling, DCT and quantisation; ours is the half that",
          "stays on the host, fed the coefficients PIL's own file holds."]
    if "device" in r:
        d = r["device"]
        L += ["", "## 2. Device: `cft_jpeg_encode_coef`, 64 pairs of 640 x 512 in one launch", "",
              f"{d['files']} images, {d['read_mbytes']} MB of pixels in, {d['write_mbytes']} MB of int16 coefficients out: median {d['median_ms']} ms, min {d['min_ms']} ms over "
              f"{d['runs']} runs (HIP events around the call, 5 warm-up calls).  The HBM floor of that traffic at {HBM_GBYTES_PER_S / 1000:g} TB/s is {d['hbm_floor_ms']} ms.",
              "Every run reads and writes the same buffers, so part of them can stay in the 256 MiB Infinity Cache: a call on freshly drawn images, as in",
              "detect, was not timed on its own.", "",
              "## 3. The copy of the coefficients into pinned memory", "",
              f"{d['write_mbytes']} MB, one non-blocking copy: median {d['copy_median_ms']} ms, min {d['copy_min_ms']} ms ({d['copy_gbytes_per_s']} GB/s).  "
              "It is as many bytes as the pixels PIL's path copies (int16 coefficients of 1.5 samples per pixel, 3 bytes per pixel either way)."]
        t = r["detect"]
        L += ["", "## 4. `detect(opt)` with saved images, batch 8, img-size 640, the tiny fixture checkpoint", "",
              f"Timed runs over {t['images_per_window']} images each (host clock around the whole call, device synchronise at both ends), PIL and device encoding",
              "alternating in one process after one warm-up run each; the files of the last two runs are equal byte for byte.", "",
              "| saved images encoded by | images/s (median) | windows |", "|---|---|---|",
              f"| PIL (the default) | {t['pil']['images_per_s_median']} | {t['pil']['images_per_s_windows']} |",
              f"| `device_jpeg` | {t['device']['images_per_s_median']} | {t['device']['images_per_s_windows']} |", "",
              f"device / pil = {t['device_over_pil']}" + ("" if t["device_over_pil"] > 1 else ": the device path is NOT faster than PIL end to end on this box and these images.")]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.md"))
    a = ap.parse_args()
    res = {"host": platform.processor() or platform.machine()}
    imgs = images(a.pairs)
    res["host_part"] = host_part(imgs[:32], a.passes)
    if not a.host_only:
        res["device"] = device_part(imgs[:64] if len(imgs) >= 64 else imgs, a.runs)
        res["detect"] = detect_part(imgs, a.windows)
    with open(a.out, "w") as f:
        f.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
