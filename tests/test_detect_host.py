"""Host tests of the detect stage (no GPU): the restatement in tests/detect_ref.py against the reference's own results in
tests/golden/detect/detect_cases.pt, the hundredths routine against Python's formatting, the inference loaders' file discovery,
grouping and geometry, increment_path, the command line's defaults and refusals, and the ABI of the two new entry points."""
import ctypes
import os
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

import detect_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "detect", "detect_cases.pt")
DATA = os.path.join(ROOT, "tests", "golden", "dataset")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


case_inputs, check_case = detect_ref.case_inputs, detect_ref.check_case


@pytest.mark.parametrize("name", ["landscape_nc3", "reduced_nc80", "half_to_even", "clipped", "portrait_nc1", "empty"])
def test_restatement_equals_reference(golden, name):
    case = golden["cases"][name]
    dets, counts, geom = case_inputs(case)
    ref = detect_ref.boxes_ref(dets, counts, geom, len(case["names"]))
    assert ref["flag"] == 0
    check_case(case, ref, ref["hist"])
    sq = detect_ref.boxes_ref(dets, counts, geom, len(case["names"]), square=True)
    n = len(case["dets"])
    for r, (y1, x1, hh, ww) in zip(reversed(range(n)), case["crops_square"]):
        cx1, cy1, cx2, cy2 = (int(v) for v in sq["crop"][0, r])
        assert (max(cy2 - cy1, 0), max(cx2 - cx1, 0)) == (hh, ww) and (not (hh and ww) or (cy1, cx1) == (y1, x1))
    # pack / unpack of the kernel's buffer is lossless
    back = detect_ref.unpack_slots(detect_ref.pack_slots(ref))
    assert all(np.array_equal(back[k], ref[k]) for k in back)


def test_crop_rectangle_and_save_one_box(golden, tmp_path):
    import msod_amd  # noqa: F401
    from msod_amd.utils.general import crop_rectangle, save_one_box
    from PIL import Image
    for name in ("clipped", "landscape_nc3"):
        case = golden["cases"][name]
        n = len(case["dets"])
        for square, key in ((False, "crops"), (True, "crops_square")):
            for box, (y1, x1, hh, ww) in zip(reversed(case["rounded"].tolist()), case[key]):
                cx1, cy1, cx2, cy2 = crop_rectangle(box, case["im0_shape"], square=square)
                assert (max(cy2 - cy1, 0), max(cx2 - cx1, 0)) == (hh, ww) and (not (hh and ww) or (cy1, cx1) == (y1, x1))
    im = np.random.default_rng(0).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    p = save_one_box([20, 10, 50, 40], im, file=tmp_path / 'crops' / 'car' / 'a.jpg')
    assert p == tmp_path / 'crops' / 'car' / 'a.jpg' and Image.open(p).size == (41, 41)          # 30 * 1.02 + 10 = 40.6 around (35, 25): 14.7 .. 55.3 -> [14, 55)
    assert save_one_box([20, 10, 50, 40], im, file=tmp_path / 'crops' / 'car' / 'a.jpg') == tmp_path / 'crops' / 'car' / 'a2.jpg'
    assert save_one_box(None, im, file=tmp_path / 'b.jpg', rect=(5, 5, 5, 9)) is None and not (tmp_path / 'b.jpg').exists()


def test_hundredths_equals_python_formatting():
    vals = detect_ref.hundredths_cases()
    assert len(vals) > 5000 and np.float32(0.125) in vals and np.float32(0.995) in vals
    for v in vals:
        v = float(np.float32(v))
        want = f"{v:.2f}"
        h = detect_ref.hundredths(v)
        assert 0 <= h <= 100 and f"{h // 100}.{h // 10 % 10}{h % 10}" == want, (v, h, want)
    assert detect_ref.hundredths(1.5) == 100 and detect_ref.hundredths(-0.3) == 0 and detect_ref.hundredths(float("nan")) == 0


def test_load_images_discovery():
    import msod_amd  # noqa: F401
    from msod_amd.utils.datasets import LoadImages
    d = os.path.join(DATA, "rgb", "images")
    ds = LoadImages(d, img_size=64, stride=32)
    assert len(ds) == 10 and ds.files == sorted(ds.files) and all(f.endswith(".png") for f in ds.files) and ds.mode == "image"
    assert LoadImages(os.path.join(d, "p1*.png")).files == [os.path.join(d, "p1_128x96.png")]
    assert LoadImages(os.path.join(d, "p8_7x5.png")).nf == 1
    with pytest.raises(Exception, match="does not exist"):
        LoadImages(os.path.join(d, "nope"))
    with pytest.raises(AssertionError, match="No images"):
        LoadImages(os.path.join(DATA, "rgb", "labels"))


def test_load_images_refuses_videos(tmp_path):
    import msod_amd  # noqa: F401
    from msod_amd.utils.datasets import LoadImages
    (tmp_path / "a.mp4").write_bytes(b"")
    with pytest.raises(NotImplementedError, match="video"):
        LoadImages(str(tmp_path))


def test_load_image_pairs_grouping_and_geometry(tmp_path):
    import msod_amd  # noqa: F401
    from msod_amd.utils import datasets as D
    from PIL import Image
    ds = D.LoadImagePairs(os.path.join(DATA, "rgb", "images"), os.path.join(DATA, "ir", "images"), img_size=64, stride=32, batch_size=4)
    assert len(ds.pairs) == 10 and all(Path(a).name == Path(b).name for a, b in ds.pairs)
    assert ds.shapes[:4] == [(64, 64), (96, 128), (128, 96), (75, 100)]              # (h0, w0) from the file names' WxH
    assert ds.batches == [[i] for i in range(10)]                                     # ten different sizes: nothing to group
    # geometry is the reference letterbox's (auto=True, scale-up allowed): 7x5 is enlarged to 64 wide and padded to a stride multiple
    mode, (H, W, rh, rw, top, left) = ds.batch_mode([8])
    assert (H, W, rh, rw, top, left) == (64, 64, 46, 64, 9, 0) and mode == D.PAIR_LINEAR
    mode, g = ds.batch_mode([0])
    assert mode == D.PAIR_COPY and g == (64, 64, 64, 64, 0, 0)
    mode, g = ds.batch_mode([1])                                                      # 128x96 reduced to 64x48: not the pair kernel's enlarging resize
    assert mode is None and g == (64, 64, 48, 64, 8, 0)
    # grouping: consecutive pairs of one size share a batch, up to batch_size; a different size starts a new one
    for sub in ("a", "b"):
        (tmp_path / sub).mkdir()
        for i, (w, h) in enumerate([(20, 10), (20, 10), (20, 10), (10, 20), (20, 10)]):
            Image.new("RGB", (w, h), (i, i, i)).save(tmp_path / sub / f"{i}.png")
    ds = D.LoadImagePairs(str(tmp_path / "a"), str(tmp_path / "b"), img_size=32, batch_size=2)
    assert ds.batches == [[0, 1], [2], [3], [4]]
    assert D.LoadImagePairs(str(tmp_path / "a"), str(tmp_path / "b"), img_size=32, batch_size=8).batches == [[0, 1, 2], [3], [4]]
    Image.new("RGB", (21, 10)).save(tmp_path / "b" / "4.png")
    with pytest.raises(ValueError, match="one size"):
        D.LoadImagePairs(str(tmp_path / "a"), str(tmp_path / "b"), img_size=32)


def test_increment_path(tmp_path):
    import msod_amd  # noqa: F401
    from msod_amd.utils.general import increment_path
    p = tmp_path / "runs" / "exp"
    assert increment_path(p) == p and not p.exists()
    assert increment_path(p, mkdir=True) == p and p.is_dir()
    assert increment_path(p) == tmp_path / "runs" / "exp2"
    assert increment_path(p, exist_ok=True) == p
    (tmp_path / "runs" / "exp2").mkdir()
    (tmp_path / "runs" / "exp7").mkdir()
    assert increment_path(p) == tmp_path / "runs" / "exp8"
    assert increment_path(p, sep="_") == tmp_path / "runs" / "exp_2"
    f = tmp_path / "crops" / "car" / "im.jpg"
    assert increment_path(f, mkdir=True) == f and f.parent.is_dir()
    f.write_bytes(b"x")
    assert increment_path(f) == tmp_path / "crops" / "car" / "im2.jpg"
    # a parent directory that holds the stem followed by digits does not set the number (the reference's whole-path search would say 792)
    g = tmp_path / "e22a791e" / "a.jpg"
    assert increment_path(g, mkdir=True) == g
    g.write_bytes(b"x")
    assert increment_path(g) == tmp_path / "e22a791e" / "a2.jpg"
    (tmp_path / "e22a791e" / "a2.jpg").write_bytes(b"x")
    assert increment_path(g) == tmp_path / "e22a791e" / "a3.jpg"
    h = tmp_path / "e22a791e" / "a+b"                       # a stem with regex characters is matched literally
    h.mkdir()
    assert increment_path(h) == tmp_path / "e22a791e" / "a+b2"


def test_argparse_defaults_are_the_references(golden):
    import msod_amd  # noqa: F401
    from msod_amd.detect import make_parser
    got = vars(make_parser().parse_args([]))
    assert got.pop("batch_size") == 1
    assert got == golden["defaults"]
    opt = make_parser().parse_args(["--save-txt", "--save-conf", "--save-crop", "--nosave", "--classes", "0", "2", "--line-thickness", "3", "--batch-size", "4"])
    assert opt.save_txt and opt.save_conf and opt.save_crop and opt.nosave and opt.classes == [0, 2] and opt.line_thickness == 3 and opt.batch_size == 4


@pytest.mark.parametrize("argv", [["--view-img"], ["--update"], ["--augment"], ["--source1", "0"], ["--source1", "list.txt"],
                                  ["--source1", "rtsp://camera/1"], ["--source1", "HTTP://host/stream"]])
def test_refused_options_raise(argv, tmp_path):
    import msod_amd  # noqa: F401
    from msod_amd.detect import check_options, detect, make_parser
    opt = make_parser().parse_args(argv + ["--project", str(tmp_path / "runs")])
    with pytest.raises(NotImplementedError):
        check_options(opt)
    with pytest.raises(NotImplementedError):
        detect(opt)
    assert not (tmp_path / "runs").exists()                     # refused before anything is created


def test_colors_are_the_tableau_palette():
    import msod_amd  # noqa: F401
    from msod_amd.utils.plots import colors
    assert colors.n == 10 and colors(0) == (31, 119, 180) and colors(0, True) == (180, 119, 31) and colors(13) == colors(3) == (214, 39, 40)
    assert colors(9) == (23, 190, 207)


def test_glyph_atlas():
    import msod_amd  # noqa: F401
    from msod_amd.utils.plots import glyph_atlas
    a = glyph_atlas()
    assert a.dtype == np.uint8 and a.shape[0] == 96 and 1 <= a.shape[1] <= 64 and 1 <= a.shape[2] <= 64
    assert not (a[0] >= 128).any() and (a[ord("A") - 32] >= 128).any() and glyph_atlas() is a


def test_header_declares_the_detect_abi():
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    from msod_amd.utils import plots
    v, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["cft_detect_boxes"] == (i, [v, v, i, i, v, i, f, f, i, v, v, v, v])
    assert _lib.SIGNATURES["cft_detect_render"] == (i, [v, v, i, v, i, v, i, i, i, i, v, v, i, v, i, i, v])
    assert _lib.ABI_VERSION >= 18 and "detect.hip" in _lib.SOURCES
    assert _lib._consts["CFT_RENDER_DESC_BYTES"] == plots.RENDER_DESC.itemsize == 48
    assert (_lib._consts["CFT_RENDER_LABELS"], _lib._consts["CFT_RENDER_CONF"], _lib._consts["CFT_RENDER_MAX_NAME"]) == (1, 2, 32)


def test_render_ref_painters_order():
    """The restatement itself: the lower row wins where two boxes overlap, text over background over outline."""
    slots = detect_ref.unpack_slots(np.zeros((1, 2, 16), np.int32))
    slots["xyxy"][0] = [[4, 12, 20, 24], [10, 14, 30, 28]]
    slots["cls"][0], slots["valid"][0], slots["conf100"][0] = [0, 1], [1, 1], [57, 9]
    atlas = np.zeros((96, 7, 5), np.uint8)
    atlas[ord("a") - 32, 1:6, 2] = 255
    im = np.zeros((32, 40, 3), np.uint8)
    detect_ref.render_ref([im], slots, 0, [(10, 0, 0), (0, 20, 0)], (1, 2, 3), 1, True, False, ["a", "a"], atlas)
    assert tuple(im[14, 10]) == (0, 20, 0)                 # box 1's corner lies inside box 0's interior: nothing of box 0 covers it
    assert tuple(im[14, 20]) == (10, 0, 0)                 # box 0's right edge crosses box 1's top edge: row 0 wins
    assert tuple(im[12, 4]) == (10, 0, 0) and tuple(im[6, 6]) == (1, 2, 3) and tuple(im[6, 5]) == (10, 0, 0)   # outline, text, background
    assert tuple(im[2, 4]) == (10, 0, 0) and tuple(im[1, 4]) == (0, 0, 0) and tuple(im[12, 9]) == (10, 0, 0)
    assert tuple(im[11, 10]) == (0, 20, 0) and tuple(im[12, 12]) == (10, 0, 0)      # box 1's label background lies across box 0's top edge: row 0 wins there
