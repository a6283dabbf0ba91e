"""GPU tests of the detect driver on batches of more than one pair, of the inference loaders' output, of the device hundredths
routine on the whole tie list, and of ``Detections.save`` / ``crop`` / ``print`` / ``tolist``.

The source folders are built in a temporary directory from the PNGs of tests/golden/dataset/: three consecutive 100 x 75 pairs (the
letterbox REDUCES them at --img-size 96: two cft_letterbox_u8 launches per pair), two 40 x 32 pairs (it ENLARGES them: one
cft_pair_batch_u8 launch with two table rows) and one 64 x 64 pair."""
import io
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import detect_ref
from gpu_busy import busy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "dataset")
CKPT = os.path.join(ROOT, "tests", "golden", "ref_ckpt_tiny.pt")
NAMES = ["person", "car", "bicycle"]
PALETTE = [(31, 119, 180), (255, 127, 14), (44, 160, 44)]
TEXT = (255, 255, 225)
IMG_SIZE = 96
# new name -> (fixture stem, flip): pairs of one size are consecutive in sorted order
LAYOUT = [("a0", "p3_100x75", None), ("a1", "p3_100x75", 1), ("a2", "p3_100x75", 0), ("b0", "p6_40x32", None), ("b1", "p6_40x32", 1),
          ("c0", "p0_64x64", None)]


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("pairs")
    for stream in ("rgb", "ir"):
        (root / stream).mkdir()
        for new, stem, flip in LAYOUT:
            a = np.array(Image.open(os.path.join(DATA, stream, "images", stem + ".png")).convert("RGB"))
            if flip is not None:
                a = np.ascontiguousarray(np.flip(a, flip))
            Image.fromarray(a).save(root / stream / (new + ".png"))
    return root


def _decoded(folders, stream):
    from PIL import Image
    return [np.array(Image.open(folders / stream / (new + ".png")).convert("RGB")) for new, _, _ in LAYOUT]


def _letterbox_chw(dev, rgb):
    """The existing ``letterbox`` (auto=True, scale-up allowed, as LoadImages calls it) on an RGB original: it takes cv2's BGR order and
    writes the CHW RGB planes."""
    import msod_amd  # noqa: F401
    from msod_amd.utils.datasets import letterbox
    bgr = torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1])).to(dev)
    return letterbox(bgr, IMG_SIZE, stride=32, chw_rgb=True)[0]


def test_load_image_pairs_batches_equal_letterbox_pair(dev, folders):
    import msod_amd  # noqa: F401
    from msod_amd.utils import datasets as D
    rgb, ir = _decoded(folders, "rgb"), _decoded(folders, "ir")
    ds = D.LoadImagePairs(str(folders / "rgb"), str(folders / "ir"), IMG_SIZE, 32, batch_size=4, device=dev)
    assert ds.batches == [[0, 1, 2], [3, 4], [5]]
    assert ds.batch_mode([0, 1, 2])[0] is None and ds.batch_mode([3, 4])[0] == D.PAIR_LINEAR and ds.batch_mode([5])[0] == D.PAIR_LINEAR
    seen = 0
    for (paths, img6, originals, shapes), indices in zip(ds, ds.batches):
        B = len(indices)
        assert img6.dtype == torch.uint8 and img6.shape[:2] == (B, 6) and len(paths) == len(originals) == len(shapes) == B
        for k, i in enumerate(indices):
            assert Path(paths[k][0]).name == Path(paths[k][1]).name == LAYOUT[i][0] + ".png"
            assert shapes[k] == (rgb[i].shape[:2], None)
            assert np.array_equal(originals[k][0].cpu().numpy(), rgb[i]) and np.array_equal(originals[k][1].cpu().numpy(), ir[i])
            assert np.array_equal(ds.host_originals[k][0], rgb[i]) and np.array_equal(ds.host_originals[k][1], ir[i])
            # the yielded block equals the existing per-image letterbox of both streams, and letterbox_pair's block
            want = torch.cat((_letterbox_chw(dev, rgb[i]), _letterbox_chw(dev, ir[i])))
            assert tuple(want.shape) == tuple(img6[k].shape) and torch.equal(img6[k], want), (i, k)
            pair, _, _ = D.letterbox_pair(torch.from_numpy(np.ascontiguousarray(rgb[i][:, :, ::-1])).to(dev),
                                          torch.from_numpy(np.ascontiguousarray(ir[i][:, :, ::-1])).to(dev), IMG_SIZE, stride=32, auto=True, scaleup=True)
            assert torch.equal(img6[k], pair)
            seen += 1
    assert seen == 6
    assert tuple(img6.shape) == (1, 6, 96, 96)
    # batch size 1: the same blocks, one pair at a time
    load = lambda bs: [b[1] for b in D.LoadImagePairs(str(folders / "rgb"), str(folders / "ir"), IMG_SIZE, 32, batch_size=bs, device=dev)]   # noqa: E731
    ones, fours = load(1), load(4)
    assert [t.shape[0] for t in ones] == [1] * 6 and [t.shape[0] for t in fours] == [3, 2, 1]
    assert torch.equal(torch.cat(ones[:3]), fours[0]) and torch.equal(torch.cat(ones[3:5]), fours[1]) and torch.equal(ones[5], fours[2])


def test_load_image_pairs_reuses_a_slot_only_after_the_launch_that_read_it(dev, folders):
    """test_gpu_dataset.py's test of the same name, for this loader: one pair per batch, so consecutive batches differ in size and
    reuse the two slots; slow work is queued on the consumer stream before every batch and the loop body waits for nothing.  Every
    batch must still be its own, and - the slots being reused - every earlier batch's originals must still be its files afterwards."""
    import msod_amd  # noqa: F401
    from msod_amd.utils import datasets as D
    rgb, ir = _decoded(folders, "rgb"), _decoded(folders, "ir")
    ds = D.LoadImagePairs(str(folders / "rgb"), str(folders / "ir"), IMG_SIZE, 32, batch_size=1, device=dev)
    assert ds.batches == [[i] for i in range(6)]
    want = [D.letterbox_pair(torch.from_numpy(np.ascontiguousarray(rgb[i][:, :, ::-1])).to(dev),
                             torch.from_numpy(np.ascontiguousarray(ir[i][:, :, ::-1])).to(dev), IMG_SIZE, stride=32, auto=True, scaleup=True)[0] for i in range(6)]
    torch.cuda.synchronize()
    for what in ("first pass", "second pass"):
        kept, tail = [], None
        busy(dev)
        for paths, img6, originals, shapes in ds:
            kept.append((img6.clone(), originals))
            tail = busy(dev)
        pending = not torch.cuda.current_stream().query()                  # the host got here with consumer work still queued
        torch.cuda.synchronize()
        print(f"{what}: consumer stream still busy when the host finished: {pending}")
        assert len(kept) == 6 and tail is not None
        for i, (img6, originals) in enumerate(kept):
            assert tuple(img6.shape[1:]) == tuple(want[i].shape) and torch.equal(img6[0], want[i]), f"{what}: batch {i}"
            (o_rgb, o_ir), = originals
            assert np.array_equal(o_rgb.cpu().numpy(), rgb[i]) and np.array_equal(o_ir.cpu().numpy(), ir[i]), f"{what}: originals of batch {i}"


def test_load_images_on_the_gpu(dev, folders):
    import msod_amd  # noqa: F401
    from msod_amd.utils.datasets import LoadImages
    rgb = _decoded(folders, "rgb")
    ds = LoadImages(str(folders / "rgb"), IMG_SIZE, 32, device=dev)
    out = list(ds)
    assert len(out) == len(ds) == 6
    for (path, img, im0, cap), (new, _, _), want in zip(out, LAYOUT, rgb):
        assert Path(path).name == new + ".png" and cap is None
        assert im0.is_cuda and np.array_equal(im0.cpu().numpy(), want)
        ref = _letterbox_chw(dev, want)
        assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == tuple(ref.shape) and torch.equal(img, ref)
    assert tuple(out[0][1].shape) == (3, 96, 96) and tuple(out[3][1].shape) == (3, 96, 96)      # 100x75 -> 96x72 + 24; 40x32 -> 96x77 + 19


def _detect(folders, project, name, batch_size):
    import msod_amd  # noqa: F401
    from msod_amd.detect import detect, make_parser
    opt = make_parser().parse_args(["--weights", CKPT, "--source1", str(folders / "rgb"), "--source2", str(folders / "ir"), "--img-size", str(IMG_SIZE),
                                    "--conf-thres", "0.001", "--save-txt", "--save-conf", "--save-crop", "--project", str(project), "--name", name,
                                    "--batch-size", str(batch_size)])
    lines, record = [], []
    return Path(detect(opt, log=lines.append, record=record)), lines, record


@pytest.fixture(scope="module")
def runs(dev, folders, tmp_path_factory):
    project = tmp_path_factory.mktemp("runs")
    return {bs: _detect(folders, project, f"bs{bs}", bs) for bs in (1, 4)}


def _tree(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def test_detect_real_batches_equal_the_restatement(dev, folders, runs):
    """The --batch-size 4 run (batches of 3, 2 and 1 pairs): every image's box buffer, label file, printed line, drawn images and
    crops against tests/detect_ref.py on that image's NMS output - images 1 and 2 of a batch included."""
    import msod_amd  # noqa: F401
    from msod_amd.utils import datasets as D
    from msod_amd.utils.metrics import geometry
    from msod_amd.utils.plots import glyph_atlas
    from PIL import Image
    assert [len(b) for b in D.LoadImagePairs(str(folders / "rgb"), str(folders / "ir"), IMG_SIZE, 32, batch_size=4).batches] == [3, 2, 1]
    save_dir, lines, record = runs[4]
    rgb, ir = _decoded(folders, "rgb"), _decoded(folders, "ir")
    atlas = glyph_atlas()
    printed = [l for l in lines if "Done. (" in l and "x" in l.split(" ")[0]]
    assert len(record) == len(printed) == 6 and all(len(r["dets"]) > 0 for r in record)
    for i, (rec, line) in enumerate(zip(record, printed)):
        stem = LAYOUT[i][0]
        assert Path(rec["paths"][0]).stem == stem and rec["shape"] == rgb[i].shape[:2]
        n = len(rec["dets"])
        dets = np.zeros((1, 300, 6), np.float32)
        dets[0, :n] = rec["dets"].numpy()
        ref = detect_ref.boxes_ref(dets, np.array([n], np.int32), geometry([(rec["shape"], None)], rec["img_hw"]).numpy(), 3)
        assert np.array_equal(rec["slots"][None], detect_ref.pack_slots(ref)) and np.array_equal(rec["hist"], ref["hist"][0])
        assert (save_dir / "labels" / f"{stem}.txt").read_text() == "".join(detect_ref.label_lines(ref, 0, True))
        assert line.startswith('%gx%g ' % rec["img_hw"] + detect_ref.class_string(ref["hist"][0], NAMES) + "Done. (")
        want = [rgb[i].copy(), ir[i].copy()]
        detect_ref.render_ref(want, ref, 0, PALETTE, TEXT, 2, True, False, NAMES, atlas)
        for s, tag in enumerate(("rgb", "ir")):
            assert np.array_equal(rec["drawn"][s], want[s]), (i, tag)
            assert np.array_equal(np.array(Image.open(save_dir / f"{stem}_{tag}.png")), want[s])
        per_class = {}
        for r in reversed(range(n)):
            x1, y1, x2, y2 = (int(v) for v in ref["crop"][0, r])
            if x2 > x1 and y2 > y1:
                per_class.setdefault(NAMES[ref["cls"][0, r]], []).append((x1, y1, x2, y2))
        for cname, rects in per_class.items():
            for k, (x1, y1, x2, y2) in enumerate(rects):
                buf = io.BytesIO()
                Image.fromarray(rgb[i][y1:y2, x1:x2]).save(buf, "JPEG")            # the same encoder on the UNDRAWN crop of THIS image
                f = save_dir / "crops" / cname / (f"{stem}.jpg" if k == 0 else f"{stem}{k + 1}.jpg")
                assert f.read_bytes() == buf.getvalue(), (i, cname, k)


def test_detect_batch_size_1_and_4_write_the_same_files(dev, runs):
    a, b = _tree(runs[1][0]), _tree(runs[4][0])
    assert a.keys() == b.keys() and len(a) >= 18
    for ra, rb in zip(runs[1][2], runs[4][2]):
        assert ra["paths"] == rb["paths"]
        assert torch.equal(ra["dets"], rb["dets"]), Path(ra["paths"][0]).name
        assert np.array_equal(ra["slots"], rb["slots"]) and np.array_equal(ra["drawn"], rb["drawn"])
    for k in a:
        assert a[k] == b[k], k


def test_device_hundredths_on_the_tie_list(dev):
    """The device routine (word 5 of cft_detect_boxes) on the host test's whole list: every tie, its float32 neighbours, the values
    around x.xx and x.xx5 - equal to the restatement, which the host test pins to Python's own formatting."""
    import msod_amd  # noqa: F401
    from msod_amd import ops
    vals = detect_ref.hundredths_cases()
    n = len(vals)
    dets = np.zeros((1, n, 6), np.float32)
    dets[0, :, :4], dets[0, :, 4] = (1, 1, 5, 5), vals
    geom = np.array([[16, 16, 1, 0, 0]], np.float32)
    boxes, _, flag = ops.detect_boxes(torch.from_numpy(dets).to(dev), torch.tensor([n], dtype=torch.int32, device=dev), torch.from_numpy(geom).to(dev), 1)
    got = boxes.cpu().numpy()[0]
    want = np.array([detect_ref.hundredths(v) for v in vals], np.int32)
    assert np.array_equal(got[:, 5], want) and int(flag.item()) == 0
    assert [f"{h // 100}.{h // 10 % 10}{h % 10}" for h in got[:, 5].tolist()] == [f"{float(v):.2f}" for v in vals]
    assert np.array_equal(got[:, 7].view(np.float32), vals)


def test_detections_save_crop_print_tolist(dev, tmp_path, capsys):
    import msod_amd  # noqa: F401
    from msod_amd.models.common import Detections
    from msod_amd.utils.general import crop_rectangle
    from PIL import Image
    g = np.random.default_rng(12)
    rgb = [g.integers(0, 256, (75, 100, 3), dtype=np.uint8), g.integers(0, 256, (48, 64, 3), dtype=np.uint8)]
    ir = [g.integers(0, 256, a.shape, dtype=np.uint8) for a in rgb]
    pred = [torch.tensor([[10.4, 12.6, 60.5, 50.2, 0.9, 1], [30.0, 20.0, 90.0, 70.0, 0.6, 1], [5.0, 40.0, 25.0, 60.0, 0.3, 0]], device=dev),
            torch.zeros((0, 6), device=dev)]
    make = lambda: Detections([torch.from_numpy(a).to(dev) for a in rgb], pred, ["x.png", "y.png"], names=NAMES, shape=(2, 3, 96, 128),   # noqa: E731
                              imgs_ir=[torch.from_numpy(a).to(dev) for a in ir])
    det = make()
    det.print()
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "image 1/2: 75x100 1 person, 2 cars" and out[1] == "image 2/2: 48x64" and out[2].startswith("Speed:")
    parts = det.tolist()
    assert len(parts) == 2 and parts[0].pred is pred[0] and parts[0].imgs is det.imgs[0] and parts[1].xywhn.shape == (0, 6) and parts[0].names == NAMES
    # crop: the reference's rectangle of the UNROUNDED box, cut from the undrawn RGB original; numbered per class by increment_path
    det.crop(save_dir=str(tmp_path / "c"))
    rects = [crop_rectangle(b[:4], rgb[0].shape) for b in pred[0].tolist()]
    for f, (x1, y1, x2, y2) in zip(("car/x.jpg", "car/x2.jpg", "person/x.jpg"), rects):
        buf = io.BytesIO()
        Image.fromarray(rgb[0][y1:y2, x1:x2]).save(buf, "JPEG")
        assert (tmp_path / "c" / "crops" / f).read_bytes() == buf.getvalue()
    assert np.array_equal(det.imgs[0].cpu().numpy(), rgb[0])                        # cropping draws nothing
    # save: render() then one file per image and stream
    det.save(save_dir=str(tmp_path / "s"))
    imgs, imgs_ir = det.render()
    assert (np.array(Image.open(tmp_path / "s" / "x.png")) == imgs[0].cpu().numpy()).all() and (imgs[0].cpu().numpy() != rgb[0]).any()
    assert (np.array(Image.open(tmp_path / "s" / "x_ir.png")) == imgs_ir[0].cpu().numpy()).all()
    assert (np.array(Image.open(tmp_path / "s" / "y.png")) == rgb[1]).all()          # no detections: saved as it is
    with pytest.raises(RuntimeError, match="crop before"):
        det.crop(save_dir=str(tmp_path / "late"))
