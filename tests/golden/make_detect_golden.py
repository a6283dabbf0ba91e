"""Generate ``tests/golden/detect/detect_cases.pt``: what the reference's ``detect_twostream.py`` computes between
``non_max_suppression`` and its files, on a handful of small synthetic NMS outputs.

Runs ONLY in the build container (needs the reference checkout, ``make_golden.REF``).  The reference's own ``scale_coords``,
``clip_coords``, ``xyxy2xywh``, ``xywh2xyxy``, ``save_one_box`` and ``increment_path`` (utils/general.py) run unmodified on the CPU, with
the usual empty stand-ins for cv2 and torchvision; a stand-in ``cv2.imwrite`` records the crop it was handed (the image is an index
image, so the crop says which rectangle it is).  ``detect()`` itself needs cv2 for its input and drawing, so the loop around those
functions (detect_twostream.py:129-153) is restated here, line for line.  The argparse defaults of :198-221 are read by executing
the ``parser.add_argument`` lines of the reference's file on a fresh parser.

    python tests/golden/make_detect_golden.py       # rewrites tests/golden/detect/detect_cases.pt

The file holds data only: inputs, rounded boxes, label-file lines, printed strings, label texts, crop rectangles, defaults.
"""
import argparse
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402

OUT = os.path.join(HERE, "detect", "detect_cases.pt")

NAMES3 = ["person", "car", "bicycle"]
NAMES80 = [f"c{i}" for i in range(80)]


def letterbox_shape(h0, w0, img_size=640, stride=32):
    """img.shape[2:] of LoadImages' letterbox (auto=True, scale-up allowed; utils/datasets.py:1698-1728)."""
    r = min(img_size / h0, img_size / w0)
    nw, nh = int(round(w0 * r)), int(round(h0 * r))
    dw, dh = np.mod(img_size - nw, stride) / 2, np.mod(img_size - nh, stride) / 2
    return (nh + int(round(dh - 0.1)) + int(round(dh + 0.1)), nw + int(round(dw - 0.1)) + int(round(dw + 0.1)))


def cases():
    g = np.random.default_rng(7)
    out = []

    def rand_dets(n, H, W, nc, classes=None):
        x1, y1 = g.uniform(-8, W * 0.8, n), g.uniform(-8, H * 0.8, n)
        w, h = g.uniform(2, W * 0.5, n), g.uniform(2, H * 0.5, n)
        conf = np.sort(g.uniform(0.05, 0.99, n))[::-1]
        cls = g.integers(0, nc, n) if classes is None else np.asarray(classes)
        return np.stack([x1, y1, x1 + w, y1 + h, conf, cls], 1).astype(np.float32)

    # an ordinary landscape image, enlarged by the letterbox; class 0 three times, class 1 once, class 2 never
    out.append(("landscape_nc3", (480, 640), letterbox_shape(480, 640), NAMES3, rand_dets(4, *letterbox_shape(480, 640), 3, [0, 1, 0, 0])))
    # a large image reduced by the letterbox, 80 classes
    out.append(("reduced_nc80", (1080, 1920), letterbox_shape(1080, 1920), NAMES80, rand_dets(12, *letterbox_shape(1080, 1920), 80)))
    # gain 1, pad 0: coordinates exactly on .5 after scale_coords, so .round() shows half-to-even
    half = np.array([[0.5, 1.5, 10.5, 11.5, 0.875, 0], [2.5, 3.5, 20.5, 21.5, 0.625, 1], [4.5, 6.5, 12.5, 30.5, 0.375, 1],
                     [7.5, 0.5, 63.5, 8.5, 0.125, 2]], np.float32)
    out.append(("half_to_even", (64, 96), (64, 96), NAMES3, half))
    # clipped at all four borders (x2 == w0, y2 == h0), a zero-area box, a box wholly outside (it collapses onto the border)
    clip = np.array([[-5, -7, 30, 20, 0.95, 0], [70, 40, 140, 90, 0.9, 1], [96, 10, 120, 30, 0.85, 2], [40, 30, 40, 30, 0.8, 0],
                     [-20, 20, -4, 44, 0.7, 1], [10, 60.2, 50, 64, 0.005, 0], [3, 3, 95.6, 63.7, 0.995, 0]], np.float32)
    out.append(("clipped", (64, 96), (64, 96), NAMES3, clip))
    # a portrait image with padding left and right, one class
    out.append(("portrait_nc1", (100, 75), letterbox_shape(100, 75), ["person"], rand_dets(5, *letterbox_shape(100, 75), 1)))
    # no detections
    out.append(("empty", (48, 64), letterbox_shape(48, 64), NAMES3, np.zeros((0, 6), np.float32)))
    return out


def reference_defaults():
    """The defaults of detect_twostream.py:198-221: its own add_argument lines executed on a fresh parser."""
    parser = argparse.ArgumentParser()
    with open(os.path.join(make_golden.REF, "detect_twostream.py")) as fh:
        lines = [l.strip() for l in fh if l.strip().startswith("parser.add_argument(")]
    for l in lines:
        exec(l.split("  #")[0], {"parser": parser})
    return vars(parser.parse_args([]))


def main():
    make_golden.install_reference()
    import cv2
    from utils.general import clip_coords, increment_path, save_one_box, scale_coords, xywh2xyxy, xyxy2xywh  # noqa: F401

    handed = []
    cv2.imwrite = lambda path, crop: handed.append((path, np.array(crop)))
    golden = {"defaults": reference_defaults(), "cases": {}}
    for name, im0_shape, img_shape, names, dets in cases():
        h0, w0 = im0_shape
        im0s = np.zeros((h0, w0, 3), np.int32)                    # pixel (y, x) = (y, x, 0): a crop tells its rectangle
        im0s[..., 0], im0s[..., 1] = np.arange(h0)[:, None], np.arange(w0)[None, :]
        det = torch.from_numpy(dets.copy())
        gn = torch.tensor(im0s.shape)[[1, 0, 1, 0]]
        rec = {"im0_shape": im0_shape, "img_shape": img_shape, "names": names, "dets": torch.from_numpy(dets.copy()), "s": "",
               "lines": [], "lines_conf": [], "labels_conf": [], "crops": [], "crops_square": [], "rounded": torch.zeros((0, 4))}
        with tempfile.TemporaryDirectory() as tmp:
            save_dir = Path(tmp)
            s = ''
            if len(det):
                det[:, :4] = scale_coords(img_shape, det[:, :4], im0s.shape).round()
                for c in det[:, -1].unique():
                    n = (det[:, -1] == c).sum()  # detections per class
                    s += f"{n} {names[int(c)]}{'s' * (n > 1)}, "  # add to string
                for *xyxy, conf, cls in reversed(det):
                    xywh = (xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn).view(-1).tolist()  # normalized xywh
                    for save_conf, key in ((False, "lines"), (True, "lines_conf")):
                        line = (cls, *xywh, conf) if save_conf else (cls, *xywh)  # label format
                        rec[key].append(('%g ' * len(line)).rstrip() % line + '\n')
                    c = int(cls)  # integer class
                    rec["labels_conf"].append(f'{names[c]} {conf:.2f}')
                    for square, key in ((False, "crops"), (True, "crops_square")):
                        handed.clear()
                        save_one_box(xyxy, im0s, file=save_dir / 'crops' / names[c] / 'stem.jpg', BGR=True, square=square)
                        crop = handed[0][1]
                        assert handed[0][0].endswith('.jpg')
                        hh, ww = crop.shape[:2]
                        y1, x1 = (int(crop[0, 0, 0]), int(crop[0, 0, 1])) if hh and ww else (-1, -1)
                        rec[key].append((y1, x1, hh, ww))
                rec["rounded"] = det[:, :4].clone()
            rec["s"] = s
        golden["cases"][name] = rec

    # the cases show what they were built for
    c = golden["cases"]
    assert c["empty"]["s"] == "" and not c["empty"]["lines"]
    assert c["half_to_even"]["rounded"][0].tolist() == [0.0, 2.0, 10.0, 12.0] and c["half_to_even"]["rounded"][1].tolist() == [2.0, 4.0, 20.0, 22.0]
    r = c["clipped"]["rounded"]
    assert r[:, 0].min() == 0 and r[:, 1].min() == 0 and r[:, 2].max() == 96 and r[:, 3].max() == 64
    assert (r[3, 0] == r[3, 2]) and (r[3, 1] == r[3, 3])
    assert c["landscape_nc3"]["s"] == "3 persons, 1 car, "
    assert "person 0.00" in c["clipped"]["labels_conf"] and "person 1.00" in c["clipped"]["labels_conf"]      # float32(0.005) < 0.005, float32(0.995) > 0.995
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(golden, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    for k, v in c.items():
        print(k, v["img_shape"], repr(v["s"]), v["labels_conf"][:3], v["crops"][:2])
    print(golden["defaults"])


if __name__ == "__main__":
    main()
