"""Host tests (no GPU) of the paired RGB + IR dataset of utils/datasets.py against the reference's own run recorded in
tests/golden/dataset/dataset_cases.pt, and of the INTER_AREA restatement tests/dataset_ref.py."""
import contextlib
import inspect
import io
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dataset_ref as DR

ROOT, CASES, BLOCKS = DR.load_cases()
IDS = [DR.case_id(c) for c in CASES]


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        out = fn(*a, **k)
    return out, buf.getvalue()


def rel(p):
    return os.path.relpath(p, ROOT)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dataset_fields_equal_the_reference(c):
    ds, text = quiet(DR.make_dataset, ROOT, c)
    assert [rel(p) for p in ds.img_files_rgb] == c["img_files_rgb"] and [rel(p) for p in ds.img_files_ir] == c["img_files_ir"]
    assert len(ds) == ds.n == c["n"] and list(ds.indices_rgb) == list(range(c["n"]))
    assert ds.shapes.dtype == np.float64 and np.array_equal(ds.shapes, c["shapes"].numpy())
    assert len(ds.labels) == len(c["labels"])
    for got, want in zip(ds.labels, c["labels"]):
        assert got.dtype == np.float32 and got.shape == tuple(want.shape) and np.array_equal(got, want.numpy())
    assert np.array_equal(ds.batch_rgb, c["batch_rgb"].numpy())
    if c["rect"]:
        assert np.array_equal(ds.batch_shapes_rgb, c["batch_shapes_rgb"].numpy())
    # the two pairs the reference ignores as corrupted: the <10 pixel image and the label file with a repeated row
    assert text.count("WARNING: Ignoring corrupted image and/or label") == 2 and "duplicate labels" in text and "<10 pixels" in text
    assert ds.scan_results == (6, 1, 1, 2, 10)           # found, missing, empty, corrupted, total
    assert not [f for _, _, fs in os.walk(ROOT) for f in fs if f.endswith(".cache")]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_batch_targets_paths_and_shapes_equal_the_reference(c):
    from msod_amd.utils.datasets import PairLoader
    ds, _ = quiet(DR.make_dataset, ROOT, c)
    loader = PairLoader.__new__(PairLoader)              # the batch partition only: no device is touched
    loader.dataset, loader.batch_size = ds, min(c["batch_size"], len(ds))
    assert (len(ds) + loader.batch_size - 1) // loader.batch_size == len(c["batches"])
    for b, want in enumerate(c["batches"]):
        targets, paths, shapes = ds.batch_targets(loader.batch_indices(b))
        assert targets.dtype == torch.float32 and targets.device.type == "cpu" and torch.equal(targets, want["targets"])
        assert [rel(p) for p in paths] == want["paths"]
        assert DR.plain(shapes) == want["shapes"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_descriptor_builder_yields_the_recorded_geometry(c):
    """(h, w, top, left, mode) of every pair, read back from the recorded blocks: the grey border fixes top / left / h / w (the
    fixture images hold no 114-grey row or column at their edges), the original and resized sizes fix the mode."""
    from msod_amd.utils import datasets as D
    ds, _ = quiet(DR.make_dataset, ROOT, c)
    bs = min(c["batch_size"], len(ds))
    for b, want in enumerate(c["batches"]):
        idx = list(range(b * bs, min((b + 1) * bs, len(ds))))
        desc, (H, W) = ds.build_descriptors(idx)
        assert desc.dtype == D.PAIR_DESC and len(desc) == len(idx)
        for row, i, blk, shp in zip(desc, idx, want["blocks"], want["shapes"]):
            block = BLOCKS[blk].numpy()
            assert block.shape == (6, H, W)
            inside = (block != 114).any(0)
            ys, xs = np.where(inside.any(1))[0], np.where(inside.any(0))[0]
            (h0, w0), ((rh, rw), _) = shp
            assert (row["h0"], row["w0"]) == (h0, w0) == (int(ds.shapes[i][1]), int(ds.shapes[i][0]))
            assert (row["top"], row["left"], row["h"], row["w"]) == (ys[0], xs[0], ys[-1] - ys[0] + 1, xs[-1] - xs[0] + 1)
            assert (row["h"] / h0, row["w"] / w0) == (rh, rw)
            r = c["img_size"] / max(h0, w0)
            assert D.PAIR_MODE_NAMES[int(row["mode"])] == ("copy" if r == 1 else "area" if r < 1 else "linear")
    modes = {int(m) for b in range(len(c["batches"])) for m in ds.build_descriptors(list(range(b * bs, min((b + 1) * bs, len(ds)))))[0]["mode"]}
    assert modes == ({D.PAIR_COPY, D.PAIR_LINEAR, D.PAIR_AREA} if c["img_size"] == 64 else {D.PAIR_LINEAR, D.PAIR_AREA})


def test_single_cls_zeroes_the_class_column():
    c = next(c for c in CASES if c["single_cls"])
    plain_case = next(p for p in CASES if not p["single_cls"] and all(p[k] == c[k] for k in ("img_size", "rect", "pad", "batch_size")))
    assert max(l[:, 0].max().item() for l in plain_case["labels"] if len(l)) >= 2          # the fixture holds a class >= nc
    ds, _ = quiet(DR.make_dataset, ROOT, c)
    assert all((l[:, 0] == 0).all() for l in ds.labels)


def _copy_fixture(tmp_path):
    root = str(tmp_path / "dataset")
    shutil.copytree(ROOT, root, ignore=shutil.ignore_patterns("*.pt"))
    return root


def _labels_of(root, stem, text):
    for stream in ("rgb", "ir"):
        with open(os.path.join(root, stream, "labels", stem + ".txt"), "w") as f:
            f.write(text)


@pytest.mark.parametrize("text,why", [("0 0.5 0.5 0.2\n", "5 columns"), ("0 0.5 -0.5 0.2 0.2\n", "negative"), ("0 0.5 0.5 1.2 0.2\n", "non-normalized"),
                                      ("0 0.5 0.5 0.2 0.2\n0 0.5 0.5 0.2 0.2\n", "duplicate")])
def test_label_checks_ignore_the_pair_as_the_reference_does(tmp_path, text, why):
    from msod_amd.utils.datasets import LoadMultiModalImagesAndLabels, verify_image_label
    root = _copy_fixture(tmp_path)
    _labels_of(root, "p0_64x64", text)
    with pytest.raises(AssertionError, match=why):
        verify_image_label(os.path.join(root, "rgb", "images", "p0_64x64.png"), os.path.join(root, "rgb", "labels", "p0_64x64.txt"))
    ds, out = quiet(LoadMultiModalImagesAndLabels, os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), 64, 4)
    assert len(ds) == 7 and not any("p0_64x64" in p for p in ds.img_files_rgb + ds.img_files_ir) and why in out
    assert not [f for _, _, fs in os.walk(root) for f in fs if f.endswith(".cache")]


def test_missing_and_empty_label_files_are_empty_labels():
    ds, _ = quiet(DR.make_dataset, ROOT, CASES[0])
    by_name = {os.path.basename(p): l for p, l in zip(ds.img_files_rgb, ds.labels)}
    for name in ("p4_47x33.png", "p5_33x47.png"):
        assert by_name[name].shape == (0, 5) and by_name[name].dtype == np.float32


def test_image_lists_from_a_txt_file_and_a_list(tmp_path):
    from msod_amd.utils.datasets import LoadMultiModalImagesAndLabels
    root = _copy_fixture(tmp_path)
    names = ["p1_128x96.png", "p6_40x32.png"]
    for stream in ("rgb", "ir"):
        with open(os.path.join(root, stream + ".txt"), "w") as f:
            f.writelines(f"./{stream}/images/{n}\n" for n in names)
    ds, _ = quiet(LoadMultiModalImagesAndLabels, os.path.join(root, "rgb.txt"), os.path.join(root, "ir.txt"), 64, 4)
    assert [os.path.basename(p) for p in ds.img_files_rgb] == names == [os.path.basename(p) for p in ds.img_files_ir]
    ds2, _ = quiet(LoadMultiModalImagesAndLabels, [os.path.join(root, "rgb.txt")], [os.path.join(root, "ir.txt")], 64, 4)
    assert ds2.img_files_rgb == ds.img_files_rgb


def test_guards():
    from msod_amd.utils.datasets import LoadMultiModalImagesAndLabels, create_dataloader_rgb_ir
    rgb, ir = os.path.join(ROOT, "rgb", "images"), os.path.join(ROOT, "ir", "images")
    with pytest.raises(NotImplementedError, match="augment=True"):
        LoadMultiModalImagesAndLabels(rgb, ir, 64, 4, augment=True)
    with pytest.raises(NotImplementedError, match="quad=True"):
        create_dataloader_rgb_ir(rgb, ir, 64, 4, 32, SimpleNamespace(single_cls=False), quad=True)


def test_a_pair_of_two_sizes_raises(tmp_path):
    from PIL import Image
    from msod_amd.utils.datasets import LoadMultiModalImagesAndLabels
    root = _copy_fixture(tmp_path)
    Image.new("L", (60, 64)).save(os.path.join(root, "ir", "images", "p0_64x64.png"))
    with pytest.raises(ValueError, match="unaligned pair"):
        quiet(LoadMultiModalImagesAndLabels, os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), 64, 4)


def test_a_letterbox_that_would_resize_is_found_where_the_table_is_built():
    """Never for the shapes the class builds (every recorded case passes through build_descriptors above); with a batch shape forced
    below the resized images the builder raises LetterboxResizes, and targets / shapes follow the letterbox's own ratio and pad."""
    from msod_amd.utils import datasets as D
    c = next(c for c in CASES if c["img_size"] == 64 and c["rect"] and c["batch_size"] == 4 and c["pad"] == 0)
    ds, _ = quiet(DR.make_dataset, ROOT, c)
    ds.batch_shapes_rgb = np.full_like(ds.batch_shapes_rgb, 32)
    assert issubclass(D.LetterboxResizes, AssertionError)
    with pytest.raises(D.LetterboxResizes, match="resize"):
        ds.build_descriptors([0, 1, 2, 3])
    for i in range(4):
        h0, w0, h, w, top, left, mode, (H, W), ratio, pad = ds.pair_geometry(i)
        assert (H, W) == (32, 32) and ratio[0] == ratio[1] == min(32 / h, 32 / w) < 1
        assert top == int(round((32 - int(round(h * ratio[0]))) / 2 - 0.1)) and left == int(round((32 - int(round(w * ratio[0]))) / 2 - 0.1))
        labels, shapes = ds.item_targets(i)
        assert shapes == ((h0, w0), ((h / h0, w / w0), pad))
        if len(labels):
            xywh = ds.labels[i][:, 1:].astype(np.float64)
            want_x = (ratio[0] * w * xywh[:, 0] + pad[0]) / 32
            assert np.allclose(labels[:, 2].numpy(), want_x, atol=1e-5) and np.allclose(labels[:, 4].numpy(), ratio[0] * w * xywh[:, 2] / 32, atol=1e-5)


def test_a_reduction_beyond_the_kernels_cap_is_refused_before_any_work(tmp_path):
    from PIL import Image
    from msod_amd.utils import datasets as D
    assert D.PAIR_MAX_REDUCTION == 4
    root = _copy_fixture(tmp_path)
    for stream in ("rgb", "ir"):
        Image.new("RGB", (130, 40)).save(os.path.join(root, stream, "images", "p0_64x64.png"))
    rgb, ir = os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images")
    with pytest.raises(ValueError, match=r"130x40.*more than 4x per axis"):
        quiet(D.LoadMultiModalImagesAndLabels, rgb, ir, 32, 4)
    ds, _ = quiet(D.LoadMultiModalImagesAndLabels, rgb, ir, 40, 4)                       # 130x40 -> 39 or 40 x 12 is within the cap
    assert len(ds) == 8


def test_importing_the_module_does_not_import_pil():
    import subprocess
    import sys
    code = "import sys; import msod_amd.utils.datasets; assert not [m for m in sys.modules if m == 'PIL' or m.startswith('PIL.')], 'PIL imported'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_rank_shards_are_contiguous_batch_ranges():
    from msod_amd.distributed import shard_bounds
    from msod_amd.utils.datasets import create_dataloader_rgb_ir
    rgb, ir = os.path.join(ROOT, "rgb", "images"), os.path.join(ROOT, "ir", "images")
    seen = []
    for rank in range(3):
        (loader, ds), _ = quiet(create_dataloader_rgb_ir, rgb, ir, 64, 1, 32, SimpleNamespace(single_cls=False), rank=rank, world_size=3, workers=64)
        assert loader.workers == 16 and list(loader.batch_range) == list(range(*shard_bounds(8, rank, 3))) and len(loader) == len(loader.batch_range)
        seen += list(loader.batch_range)
    assert seen == list(range(8))


# ------------------------------------------------------------------------------ the INTER_AREA restatement
def _noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# Sizes at which a 16 x 16 super-sampling is exact: every cell boundary d * ssize / dsize is a multiple of 1/16, so each sample lies
# wholly in one output cell and the plain mean of the samples IS the box average (no covered fraction is below cv2's 1e-3 cut-off
# either).  Both sides are then the same real number up to float64 rounding: a few hundred operations on values <= 255, each off by
# <= 255 * 2^-53, stay below 1e-11; the bound asked is 1e-9.  At other sizes the samples straddle the boundaries by up to 1/32 of a
# pixel, an error of the sampling, not of the restatement - the smooth-ramp case bounds it: each edge of a box moves by at most 1/32
# pixel, so the mean of a ramp of slope g per pixel moves by at most g / 32 per axis.
EXACT = 1e-9


@pytest.mark.parametrize("src,dst", [((75, 100), (48, 64)), ((100, 75), (64, 48)), ((50, 25), (32, 16)), ((36, 45), (32, 40)), ((20, 30), (16, 24))])
def test_area_restatement_equals_the_supersampled_box_filter(src, dst):
    img = _noise(*src, seed=src[0] + dst[1])
    real = DR.resize_area_real(img, (dst[1], dst[0]))
    brute = DR.box_filter_supersampled(img, (dst[1], dst[0]), ss=16)
    print("max |restatement - supersampled| =", np.abs(real - brute).max())
    assert np.abs(real - brute).max() <= EXACT
    clear = np.abs(brute - np.floor(brute) - 0.5) > EXACT                                 # not a tie of the brute-force value itself
    assert clear.mean() > 0.99 and np.array_equal(DR.resize_area(img, (dst[1], dst[0]))[clear], np.rint(brute)[clear].astype(np.uint8))


@pytest.mark.parametrize("src,dst", [((33, 47), (22, 32)), ((47, 33), (32, 22))])
def test_area_restatement_on_a_ramp_at_sizes_off_the_sample_grid(src, dst):
    y, x = np.mgrid[0:src[0], 0:src[1]]
    img = np.stack([2 * x + 2 * y, 3 * x + y, x + 3 * y], -1)                             # slopes <= 3 per pixel, no wrap at these sizes
    assert img.max() < 256
    img = img.astype(np.uint8)
    real = DR.resize_area_real(img, (dst[1], dst[0]))
    brute = DR.box_filter_supersampled(img, (dst[1], dst[0]), ss=16)
    print("max |restatement - supersampled| per channel =", np.abs(real - brute).max(axis=(0, 1)))
    assert (np.abs(real - brute).max(axis=(0, 1)) <= np.array([2 + 2, 3 + 1, 1 + 3]) / 32 + EXACT).all()     # (slope in x + slope in y) / 32


@pytest.mark.parametrize("src,dst", [((96, 128), (48, 64)), ((128, 96), (32, 24)), ((12, 30), (4, 10)), ((9, 8), (3, 8))])
def test_integer_scales_are_the_exact_block_mean_with_halves_up(src, dst):
    img = _noise(*src, seed=src[1])
    iy, ix = src[0] // dst[0], src[1] // dst[1]
    sums = img.astype(np.int64).reshape(dst[0], iy, dst[1], ix, 3).sum(axis=(1, 3))
    want = (2 * sums + iy * ix) // (2 * iy * ix)
    assert np.array_equal(DR.resize_area(img, (dst[1], dst[0])), want.astype(np.uint8))
    assert not DR.near_tie(img, (dst[1], dst[0])).any()
    half = np.full((2, 2, 3), 0, np.uint8)
    half[0, 0] = 1
    half[0, 1] = 1                                                                        # mean 0.5 -> 1
    assert DR.resize_area(half, (1, 1)).tolist() == [[[1, 1, 1]]]


def test_area_tab_weights_sum_to_one_and_follow_the_integer_sizes():
    for ssize, dsize in [(100, 64), (47, 32), (33, 22), (75, 48), (1280, 640), (1024, 500)]:
        tab = DR.area_tab(ssize, dsize)
        assert tab.shape == (dsize, ssize) and np.allclose(tab.sum(1), 1.0, atol=2e-3 / (ssize / dsize))     # cv2 drops slivers <= 1e-3
        assert (tab >= 0).all() and ((tab > 0).sum(1) <= np.ceil(ssize / dsize) + 1).all()


def test_the_fixture_keeps_the_share_of_near_ties_under_the_cap():
    """<= 0.5 % of the fractional-area pixels of the committed fixture lie within 2^-10 of a tie: counted over the committed PNGs,
    and equal to what the generator counted and recorded."""
    from msod_amd.utils import datasets as D
    rec = torch.load(os.path.join(ROOT, "dataset_cases.pt"), weights_only=False)
    assert sorted(rec["near_tie"]) == [32, 64]
    for img_size, recorded in rec["near_tie"].items():
        ds, _ = quiet(DR.make_dataset, ROOT, next(c for c in CASES if c["img_size"] == img_size))
        marked = total = 0
        for i in range(len(ds)):
            h0, w0, h, w, _, _, mode, _, _, _ = ds.pair_geometry(i)
            if mode == D.PAIR_AREA and not DR.is_integer_scale((h0, w0), (h, w)):
                for img in ds.load_pair(i):
                    m = DR.near_tie(img, (w, h))
                    marked, total = marked + int(m.sum()), total + m.size
        print(f"img_size {img_size}: {marked} of {total} fractional-area pixels within 2^-10 of a tie")
        assert (marked, total) == tuple(recorded)
        assert total > 0 and marked <= 0.005 * total, (img_size, marked, total)


# ------------------------------------------------------------------------------ module surface
def test_module_surface():
    from msod_amd import _lib, ops
    from msod_amd.utils import datasets as D
    assert list(inspect.signature(D.LoadMultiModalImagesAndLabels.__init__).parameters)[1:] == [
        "path_rgb", "path_ir", "img_size", "batch_size", "augment", "hyp", "rect", "image_weights", "cache_images", "single_cls", "stride", "pad", "prefix"]
    sig = inspect.signature(D.LoadMultiModalImagesAndLabels.__init__).parameters
    assert (sig["img_size"].default, sig["batch_size"].default, sig["stride"].default, sig["pad"].default, sig["rect"].default) == (640, 16, 32, 0.0, False)
    assert list(inspect.signature(D.create_dataloader_rgb_ir).parameters) == [
        "path1", "path2", "imgsz", "batch_size", "stride", "opt", "hyp", "augment", "cache", "pad", "rect", "rank", "world_size", "workers",
        "image_weights", "quad", "prefix"]
    assert list(inspect.signature(D.img2label_paths).parameters) == ["img_paths"]
    assert list(inspect.signature(D.xywhn2xyxy).parameters) == ["x", "w", "h", "padw", "padh"]
    assert list(inspect.signature(ops.pair_batch_u8).parameters) == ["desc_dev", "desc_host", "out", "color"]
    a = os.sep.join(["", "d", "images", "val", "x.images.jpg"])
    assert D.img2label_paths([a]) == [os.sep.join(["", "d", "labels", "val", "x.images.txt"])]
    box = np.array([[0.5, 0.5, 0.2, 0.4]], np.float32)
    assert np.allclose(D.xywhn2xyxy(box, 100, 50, 3, 7), [[43, 22, 63, 42]])
    restype, argtypes = _lib.SIGNATURES["cft_pair_batch_u8"]
    assert len(argtypes) == 8 and _lib.ABI_VERSION >= 17 and D.PAIR_DESC.itemsize == 64
    # the existing functions keep their signatures
    assert list(inspect.signature(D.letterbox_pair).parameters) == ["img_rgb", "img_ir", "new_shape", "stride", "auto", "scaleup", "out"]
