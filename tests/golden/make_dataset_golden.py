"""Writes the paired RGB + IR fixture dataset ``tests/golden/dataset/`` and ``tests/golden/dataset/dataset_cases.pt``.

    python tests/golden/make_dataset_golden.py fixture     # the PNG pairs and the label files (seeded, no reference needed)
    python tests/golden/make_dataset_golden.py cases REF   # the recording, REF = a checkout of the reference

``cases`` runs the REFERENCE's own ``LoadMultiModalImagesAndLabels`` and ``collate_fn`` (utils/datasets.py:820-1288) on a temporary
copy of the fixture (the reference writes ``.cache`` files beside its labels).  cv2 is absent, so its calls are bound to
restatements: ``cv2.imread`` to a PIL reader (RGB reversed to BGR), ``cv2.resize`` to oracle/letterbox_oracle.py (INTER_LINEAR) and
tests/dataset_ref.py (INTER_AREA), ``cv2.copyMakeBorder`` to oracle/letterbox_oracle.py; ``np.int = int`` in this process (the
reference predates numpy 2).  Every other line executed - lists, label checks, rect sort, batch shapes, targets, shapes, packing -
is the reference's.  Only recorded data is written.

The sizes (w x h): 64x64 (r == 1 at img_size 64: copy), 128x96 / 96x128 (integer-scale area, both orientations), 100x75, 47x33,
33x47 (fractional area, int() truncation, odd widths: row strides that are no multiple of 4), 40x32 and 12x10 (enlarged at 64:
linear, the clamped edge taps).  Two pairs the reference ignores as corrupted are there on purpose: 7x5 (its "<10 pixels" check) and
50x50 whose label file repeats a row.  Labels: one empty file, one missing file, one class >= nc (for single_cls)."""
import os
import shutil
import sys
import tempfile
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "dataset")
NC = 2

# name, width, height, labels (None = no file, [] = empty file)
PAIRS = [
    ("p0_64x64", 64, 64, [(0, .30, .35, .40, .30), (1, .70, .60, .35, .50), (0, .50, .80, .60, .25)]),
    ("p1_128x96", 128, 96, [(1, .25, .30, .30, .40), (0, .60, .50, .50, .55), (1, .80, .75, .25, .35), (0, .45, .20, .70, .30)]),
    ("p2_96x128", 96, 128, [(0, .50, .50, .45, .65), (1, .30, .75, .40, .30), (0, .72, .25, .33, .42)]),
    ("p3_100x75", 100, 75, [(3, .40, .45, .55, .40), (0, .75, .70, .30, .45), (1, .20, .25, .28, .36)]),
    ("p4_47x33", 47, 33, []),
    ("p5_33x47", 33, 47, None),
    ("p6_40x32", 40, 32, [(1, .55, .50, .50, .60), (0, .25, .30, .35, .38), (1, .70, .72, .42, .44)]),
    ("p7_12x10", 12, 10, [(0, .50, .50, .60, .70), (1, .35, .40, .45, .50)]),
    ("p8_7x5", 7, 5, [(0, .50, .50, .50, .50)]),
    ("p9_50x50_dup", 50, 50, [(0, .50, .50, .40, .40), (1, .30, .30, .20, .20), (0, .50, .50, .40, .40)]),
]


def pattern(w, h, seed):
    """A seeded image that PNG compresses: per-channel ramps, a coarse checker and a sparse speckle."""
    g = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 3), np.uint8)
    for c in range(3):
        a, b, o = g.randint(1, 7), g.randint(1, 7), g.randint(0, 256)
        blk = g.randint(2, 6)
        v = x * a + y * b + o + ((x // blk + y // blk) % 2) * g.randint(20, 90)
        img[..., c] = v % 256
    speck = g.rand(h, w) < 0.06
    img[speck] = g.randint(0, 256, (int(speck.sum()), 3))
    return img


def write_fixture():
    from PIL import Image
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    for k, (name, w, h, labels) in enumerate(PAIRS):
        for s, stream in enumerate(("rgb", "ir")):
            os.makedirs(os.path.join(OUT, stream, "images"), exist_ok=True)
            os.makedirs(os.path.join(OUT, stream, "labels"), exist_ok=True)
            img = pattern(w, h, 100 * s + k)
            if stream == "ir":                       # a thermal frame: one channel, stored as a greyscale PNG
                Image.fromarray(img[..., 0], "L").save(os.path.join(OUT, stream, "images", name + ".png"), optimize=True)
            else:
                Image.fromarray(img, "RGB").save(os.path.join(OUT, stream, "images", name + ".png"), optimize=True)
            if labels is not None:
                with open(os.path.join(OUT, stream, "labels", name + ".txt"), "w") as f:
                    f.writelines("%d %.2f %.2f %.2f %.2f\n" % l for l in labels)
    with open(os.path.join(OUT, "data.yaml"), "w") as f:
        f.write("# paths relative to this file\n# one label holds a class >= nc on purpose (the single_cls case): tools/val.py takes this file with --single-cls only\n"
                "val_rgb: rgb/images\nval_ir: ir/images\nnc: %d\nnames: ['person', 'car']\n" % NC)
    print("fixture:", sum(len(fs) for _, _, fs in os.walk(OUT)), "files,",
          sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(OUT) for f in fs), "bytes")


def read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def install_reference(ref):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import letterbox_oracle as LO
    import dataset_ref as DR
    np.int = int
    for name in ("cv2", "torchvision", "seaborn"):
        sys.modules.setdefault(name, types.ModuleType(name))
    cv2 = sys.modules["cv2"]
    cv2.setNumThreads = lambda n: None
    cv2.INTER_LINEAR, cv2.INTER_AREA, cv2.BORDER_CONSTANT = LO.INTER_LINEAR, DR.INTER_AREA, LO.BORDER_CONSTANT
    cv2.imread = lambda path: np.ascontiguousarray(read_rgb(path)[:, :, ::-1])      # BGR, as cv2 gives
    cv2.resize = lambda img, dsize, interpolation: (DR.resize_area if interpolation == DR.INTER_AREA else LO.resize)(img, dsize, interpolation=interpolation)
    cv2.copyMakeBorder = LO.copyMakeBorder
    sys.path.insert(0, ref)


def plain(x):
    """Nested tuples of numpy / python scalars -> python floats and ints (what the recording holds and the tests compare)."""
    if isinstance(x, (tuple, list)):
        return tuple(plain(v) for v in x)
    return x.item() if isinstance(x, np.generic) else x


def tie_share(root, files, img_size):
    """Share of the fractional-area output pixels whose float64 value lies within 2^-10 of a tie (must stay <= 0.5 %)."""
    import dataset_ref as DR
    marked = total = 0
    for f in files:
        for stream in ("rgb", "ir"):
            img = read_rgb(os.path.join(root, f.replace("rgb" + os.sep, stream + os.sep, 1)))
            h0, w0 = img.shape[:2]
            r = img_size / max(h0, w0)
            if r >= 1:
                continue
            dsize = (int(w0 * r), int(h0 * r))
            if DR.is_integer_scale((h0, w0), (dsize[1], dsize[0])):
                continue
            m = DR.near_tie(img, dsize)
            marked, total = marked + int(m.sum()), total + m.size
    return marked, total


def write_cases(ref):
    install_reference(ref)
    from utils.datasets import LoadMultiModalImagesAndLabels  # the reference
    tmp = tempfile.mkdtemp()
    root = os.path.join(tmp, "dataset")
    shutil.copytree(OUT, root)
    rel = lambda p: os.path.relpath(p, root)      # noqa: E731
    blocks, block_ids, cases = [], {}, []

    def block_id(t):
        key = (tuple(t.shape), t.numpy().tobytes())
        if key not in block_ids:
            block_ids[key] = len(blocks)
            blocks.append(t.clone())
        return block_ids[key]

    combos = [(s, rect, pad, bs, False) for s in (32, 64) for rect in (False, True) for pad in (0.0, 0.5) for bs in (1, 4)]
    combos.append((64, True, 0.5, 4, True))
    for img_size, rect, pad, bs, single_cls in combos:
        for d, _, fs in os.walk(root):
            for f in fs:
                if f.endswith(".cache"):
                    os.remove(os.path.join(d, f))
        ds = LoadMultiModalImagesAndLabels(os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), img_size, bs, rect=rect,
                                           pad=pad, stride=32, single_cls=single_cls)
        assert [rel(p).replace("rgb", "ir", 1) for p in ds.img_files_rgb] == [rel(p) for p in ds.img_files_ir]
        case = {"img_size": img_size, "rect": rect, "pad": pad, "batch_size": bs, "single_cls": single_cls, "stride": 32,
                "img_files_rgb": [rel(p) for p in ds.img_files_rgb], "img_files_ir": [rel(p) for p in ds.img_files_ir],
                "shapes": torch.from_numpy(ds.shapes.copy()), "labels": [torch.from_numpy(l.copy()) for l in ds.labels],
                "batch_rgb": torch.from_numpy(np.asarray(ds.batch_rgb).astype(np.int64)), "n": len(ds),
                "batch_shapes_rgb": torch.from_numpy(ds.batch_shapes_rgb.astype(np.int64)) if rect else None, "batches": []}
        for lo in range(0, len(ds), bs):
            img, targets, paths, shapes = ds.collate_fn([ds[i] for i in range(lo, min(lo + bs, len(ds)))])
            case["batches"].append({"blocks": [block_id(b) for b in img], "targets": targets.clone(), "paths": [rel(p) for p in paths],
                                    "shapes": plain(shapes)})
        cases.append(case)
        print(img_size, rect, pad, bs, single_cls, "->", len(ds), "pairs,", len(case["batches"]), "batches,",
              [tuple(blocks[b["blocks"][0]].shape[1:]) for b in case["batches"]])
    ties = {}
    for img_size in (32, 64):
        marked, total = tie_share(root, cases[0]["img_files_rgb"], img_size)
        ties[img_size] = (marked, total)
        print(f"img_size {img_size}: {marked} of {total} fractional-area pixels within 2^-10 of a tie ({100.0 * marked / max(total, 1):.3f} %)")
        assert marked <= 0.005 * total, "change the fixture images, not the cap"
    path = os.path.join(OUT, "dataset_cases.pt")
    # the blocks are mostly border and pattern: deflated they keep the file far below the size limit for a committed file
    blocks = [{"shape": tuple(b.shape), "zlib": zlib.compress(b.numpy().tobytes(), 9)} for b in blocks]
    torch.save({"cases": cases, "blocks": blocks, "near_tie": ties, "nc": NC, "numpy": np.__version__}, path)
    shutil.rmtree(tmp)
    print(f"{len(cases)} cases, {len(blocks)} distinct blocks -> {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "fixture":
        write_fixture()
    elif len(sys.argv) > 2 and sys.argv[1] == "cases":
        write_cases(sys.argv[2])
    else:
        sys.exit(__doc__)
