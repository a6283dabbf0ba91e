"""Writes ``tests/golden/augment/augment_cases.pt``: what the REFERENCE's augmented dataset returns for the fixture ``tests/golden/dataset``.

    python tests/golden/make_augment_golden.py cases REF   # REF = a checkout of the reference

Runs the reference's own ``LoadMultiModalImagesAndLabels(augment=True)`` (utils/datasets.py:820-1288, with load_mosaic_RGB_IR,
random_perspective_rgb_ir, augment_hsv, letterbox) on a temporary copy of the fixture.  cv2 is absent, so its calls are bound to
restatements: ``imread`` / ``resize`` / ``copyMakeBorder`` as tests/golden/make_dataset_golden.py binds them, ``getRotationMatrix2D``
(closed form), ``warpAffine``, ``cvtColor``, ``split``, ``merge`` and ``LUT`` to tests/augment_ref.py; ``np.int = int``.  Every other line
executed - the draws and their order, tile placement, labels, box_candidates, flips, packing - is the reference's.  Only recorded
data is written.

Cases (each at batch_size 4, stride 32): (a) the values of hyp.scratch.yaml at img_size 64 and 32; (b) degrees 10, shear 5, flipud .5,
mosaic .5 (both branches in one pass); (c) rect=True (HSV and flips only); (d) scale = translate = degrees = shear = 0 and all HSV gains 0
(the warp is an integer translation, the look-up tables identity).  Per seed k: ``random.seed(k); np.random.seed(k)``, one pass over
the dataset, per item the image (zlib), labels_out, shapes and the branch taken, and after the pass the next ``random.random()`` and
``np.random.random()``.  A seed is recorded only if every accept decision of its pass - the comparisons of box_candidates and every
``random() < p`` - is clear of its threshold by a relative 1e-9: change the seed, not the margin."""
import os
import random
import shutil
import sys
import tempfile
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_dataset_golden as MD  # noqa: E402

OUT = os.path.join(HERE, "augment")
MARGIN = 1e-9

SCRATCH = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 0.0, "translate": 0.1, "scale": 0.5, "shear": 0.0, "perspective": 0.0,
           "flipud": 0.0, "fliplr": 0.5, "mosaic": 1.0, "mixup": 0.0}
# name, img_size, rect, seeds recorded, hyp (few seeds and small images keep the file small)
CASES = [
    ("a64", 64, False, 1, dict(SCRATCH)),
    ("a32", 32, False, 1, dict(SCRATCH)),
    ("b64", 64, False, 2, dict(SCRATCH, degrees=10.0, shear=5.0, flipud=0.5, mosaic=0.5)),
    ("c64", 64, True, 1, dict(SCRATCH, flipud=0.5)),
    ("d64", 64, False, 1, dict(SCRATCH, scale=0.0, translate=0.0, degrees=0.0, shear=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0)),
]


class Unclear(Exception):
    pass


def clear(value, threshold):
    if np.any(np.abs(np.asarray(value, dtype=np.float64) - threshold) <= MARGIN * max(abs(threshold), 1e-300)):
        raise Unclear(f"{value} against {threshold}")


def write_cases(ref):
    MD.install_reference(ref)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import augment_ref as AR
    cv2 = sys.modules["cv2"]
    cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = AR.COLOR_BGR2HSV, AR.COLOR_HSV2BGR
    for name in ("getRotationMatrix2D", "warpAffine", "cvtColor", "split", "merge", "LUT"):
        setattr(cv2, name, getattr(AR, name))
    import utils.datasets as D  # the reference

    stats = {"dropped": 0, "draws": []}
    ref_candidates = D.box_candidates

    def watched_candidates(box1, box2, wh_thr=2, ar_thr=20, area_thr=0.1, eps=1e-16):
        w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
        w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
        clear(w2, wh_thr), clear(h2, wh_thr), clear(w2 * h2 / (w1 * h1 + eps), area_thr), clear(np.maximum(w2 / (h2 + eps), h2 / (w2 + eps)), ar_thr)
        keep = ref_candidates(box1, box2, wh_thr=wh_thr, ar_thr=ar_thr, area_thr=area_thr, eps=eps)
        stats["dropped"] += int((~keep).sum())
        return keep

    D.box_candidates = watched_candidates
    ref_random = random.random

    def watched_random():
        v = ref_random()
        stats["draws"].append(v)
        return v

    tmp = tempfile.mkdtemp()
    root = os.path.join(tmp, "dataset")
    shutil.copytree(MD.OUT, root)
    rel = lambda p: os.path.relpath(p, root)      # noqa: E731
    cases, nbytes = [], 0
    seen = {"dropped": 0, "empty": 0, "flipud": 0, "fliplr": 0, "mosaic": 0, "letterbox": 0}
    for name, img_size, rect, nseeds, hyp in CASES:
        for d, _, fs in os.walk(root):
            for f in fs:
                if f.endswith(".cache"):
                    os.remove(os.path.join(d, f))
        ds = D.LoadMultiModalImagesAndLabels(os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), img_size, 4, augment=True,
                                             hyp=hyp, rect=rect, stride=32, pad=0.0)
        case = {"name": name, "img_size": img_size, "rect": rect, "hyp": hyp, "batch_size": 4, "stride": 32, "n": len(ds),
                "img_files_rgb": [rel(p) for p in ds.img_files_rgb], "passes": []}
        seed = 0
        while len(case["passes"]) < nseeds:
            seed += 1
            assert seed < 200, "no clear seed"
            random.seed(seed)
            np.random.seed(seed)
            stats["dropped"], stats["draws"] = 0, []
            random.random = watched_random
            try:
                items = []
                for i in range(len(ds)):
                    before = len(stats["draws"])
                    img, labels_out, path, shapes = ds[i]
                    draws = stats["draws"][before:]
                    branch = "mosaic" if shapes is None else "letterbox"
                    # the decisions of this item, in order: [mosaic] flipud fliplr
                    thresholds = ([hyp["mosaic"]] if ds.mosaic else []) + [hyp["flipud"], hyp["fliplr"]]
                    assert len(draws) == len(thresholds), (draws, thresholds)
                    for v, t in zip(draws, thresholds):
                        clear(v, t)
                    items.append({"zlib": zlib.compress(img.numpy().tobytes(), 9), "shape": tuple(img.shape), "labels_out": labels_out.clone(),
                                  "shapes": MD.plain(shapes) if shapes is not None else None, "branch": branch, "path": rel(path),
                                  "flipud": bool(draws[-2] < hyp["flipud"]), "fliplr": bool(draws[-1] < hyp["fliplr"])})
            except Unclear as e:
                print(f"{name}: seed {seed} skipped ({e})")
                continue
            finally:
                random.random = ref_random
            case["passes"].append({"seed": seed, "items": items, "next_random": random.random(), "next_np_random": float(np.random.random()),
                                   "dropped": stats["dropped"]})
            seen["dropped"] += stats["dropped"]
            for it in items:
                seen["empty"] += int(len(it["labels_out"]) == 0)
                seen["flipud"] += int(it["flipud"])
                seen["fliplr"] += int(it["fliplr"])
                seen[it["branch"]] += 1
                nbytes += len(it["zlib"])
            print(name, "seed", seed, [it["branch"][0] + ("u" if it["flipud"] else "") + ("l" if it["fliplr"] else "") + str(len(it["labels_out"])) for it in items],
                  "dropped", stats["dropped"])
        cases.append(case)
    print(seen)
    assert seen["dropped"] and seen["empty"] and seen["flipud"] and seen["fliplr"] and seen["mosaic"] and seen["letterbox"], "the recording must cover every decision"
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "augment_cases.pt")
    torch.save({"cases": cases, "numpy": np.__version__, "margin": MARGIN}, path)
    shutil.rmtree(tmp)
    print(f"{len(cases)} cases, {nbytes / 1e3:.0f} kB of deflated images -> {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "cases":
        write_cases(sys.argv[2])
    else:
        sys.exit(__doc__)
