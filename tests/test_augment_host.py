"""Host tests (no GPU) of the augmented RGB + IR training dataset of utils/datasets.py against the reference's own run recorded in
tests/golden/augment/augment_cases.pt, and of the raster restatement tests/augment_ref.py."""
import colorsys
import contextlib
import ctypes
import io
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref as AR

ROOT, CASES = AR.load_cases()
IDS = [c["name"] for c in CASES]


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def rel(p):
    return os.path.relpath(p, ROOT)


def ulp_apart(a, b):
    """Distance in float32 units in the last place."""
    ia, ib = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return np.abs(ia - ib)


def test_the_recording_covers_every_decision():
    items = [it for c in CASES for p in c["passes"] for it in p["items"]]
    assert sum(p["dropped"] for c in CASES for p in c["passes"]) > 0          # a box dropped by box_candidates
    assert any(len(it["labels_out"]) == 0 for it in items)
    assert any(it["flipud"] for it in items) and any(it["fliplr"] for it in items)
    b = next(c for c in CASES if c["name"] == "b64")
    assert {it["branch"] for it in b["passes"][0]["items"][:4]} == {"mosaic", "letterbox"}     # one batch of (b) holds both branches


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_plans_reproduce_the_recorded_pass(c):
    """Branch, row count, order and classes equal; label values within one float32 ulp (they are float32 roundings of float64 products
    that may differ in the last place between BLAS builds); shapes equal; the next draw of both generators is the recorded one."""
    ds = quiet(AR.make_dataset, ROOT, c)
    assert [rel(p) for p in ds.img_files_rgb] == c["img_files_rgb"] and len(ds) == c["n"]
    assert ds.augment is True and ds.mosaic is (not c["rect"]) and ds.mosaic_border == [-c["img_size"] // 2] * 2
    for p in c["passes"]:
        rng, np_rng = AR.generators(p["seed"])
        unequal = total = 0
        for i, want in enumerate(p["items"]):
            plan = ds.item_plan(i, rng, np_rng)
            assert ("mosaic" if plan["mosaic"] else "letterbox") == want["branch"]
            assert plan["flipud"] == want["flipud"] and plan["fliplr"] == want["fliplr"]
            got, ref = plan["labels_out"], want["labels_out"]
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape) and got.shape[1] == 6
            assert torch.equal(got[:, :2], ref[:, :2])                        # column 0 zero, the classes in order
            d = ulp_apart(got[:, 2:].numpy(), ref[:, 2:].numpy())
            assert (d <= 1).all(), f"item {i}: {d.max()} ulp"
            unequal, total = unequal + int((d != 0).sum()), total + d.size
            assert (AR_plain(plan["shapes"]) if plan["shapes"] is not None else None) == want["shapes"]
            assert tuple(plan["out"]) == tuple(want["shape"][1:])
        print(f"{c['name']} seed {p['seed']}: {unequal} of {total} label values not bit-equal")
        assert rng.random() == p["next_random"] and float(np_rng.random_sample()) == p["next_np_random"]


def AR_plain(x):
    if isinstance(x, (tuple, list)):
        return tuple(AR_plain(v) for v in x)
    return x.item() if isinstance(x, np.generic) else x


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_of_the_plans_gives_the_recorded_images(c):
    """Plans -> table -> tests/augment_ref.py (canvases, whole-image warp, whole-image HSV) against the reference's own composition of
    the same restated cv2 calls: the table carries everything the pixels need, byte for byte."""
    ds = quiet(AR.make_dataset, ROOT, c)
    p = c["passes"][0]
    rng, np_rng = AR.generators(p["seed"])
    plans = [ds.item_plan(i, rng, np_rng) for i in range(len(ds))]
    for lo in range(0, len(ds), c["batch_size"]):
        got = AR.render_plans(ds, plans[lo:lo + c["batch_size"]])
        for k, want in enumerate(p["items"][lo:lo + c["batch_size"]]):
            assert np.array_equal(got[k], want["img"].numpy()), f"item {lo + k}"


# ------------------------------------------------------------------------------ restatement self-checks
def test_integer_translation_gives_a_shifted_copy_with_a_114_border():
    g = np.random.RandomState(3)
    img = g.randint(0, 256, (20, 28, 3)).astype(np.uint8)
    assert np.array_equal(AR.warpAffine(img, np.eye(3)[:2], (28, 20)), img)
    out = AR.warpAffine(img, np.array([[1, 0, 5], [0, 1, -3.0]]), (32, 24))
    want = np.full((24, 32, 3), 114, np.uint8)
    want[0:17, 5:32] = img[3:20, 0:27]
    assert np.array_equal(out, want)


def test_luts_equal_the_reference_expressions():
    from msod_amd.utils.datasets import hsv_luts
    g = np.random.RandomState(5)
    for _ in range(4):
        r = g.uniform(-1, 1, 3) * [0.015, 0.7, 0.4] + 1
        x = np.arange(0, 256, dtype=np.int16)
        want = [((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)]
        for got in (hsv_luts(r), AR.hsv_luts(r)):
            assert got.dtype == np.uint8 and got.shape == (3, 256) and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(hsv_luts([1.0, 1.0, 1.0]), np.stack([np.arange(256) % 180, np.arange(256), np.arange(256)]).astype(np.uint8))


def test_hsv_round_trip_stays_within_the_quantisation_of_a_float_pipeline():
    """Against colorsys in float: H is quantised to 1/180 of the circle (half a step = 1/360), S and V to 1/255 (half a step = 1/510), and
    the output is rounded once (0.5).  A channel is v (1 - s f') with f' piecewise linear in 6 h of slope <= 1: an error dh in h moves it
    by at most 255 * 6 dh * s <= 255 * 6 / 360 = 4.25, an error ds by at most 255 / 510 = 0.5, an error dv by at most 0.5: 5.75 in all."""
    bound = 255 * 6 / 360 + 0.5 + 0.5 + 0.5
    g = np.random.RandomState(7)
    img = g.randint(0, 256, (48, 48, 3)).astype(np.uint8)
    img[:8] = img[:8, :, :1]                     # greys
    img[8:12] = 114
    ident = np.stack([np.arange(256) % 180, np.arange(256), np.arange(256)]).astype(np.uint8)
    out = AR.apply_hsv_rgb(img, ident)
    assert np.array_equal(out[8:12], img[8:12])  # the border grey is a fixed point
    worst = 0.0
    for (r, g_, b), got in zip(img.reshape(-1, 3), out.reshape(-1, 3)):
        want = np.array(colorsys.hsv_to_rgb(*colorsys.rgb_to_hsv(r / 255, g_ / 255, b / 255))) * 255
        worst = max(worst, np.abs(got - want).max())
    print(f"worst deviation {worst:.3f}, bound {bound:.3f}")
    assert worst <= bound


# ------------------------------------------------------------------------------ descriptors
def test_tile_rectangles_equal_hand_evaluated_values():
    """load_mosaic_RGB_IR :1504-1526 at s = 64 (canvas 128), tile 64 x 48 (w x h), evaluated by hand for a centre in each regime."""
    from msod_amd.utils.datasets import mosaic_tile_rects as R
    # centre (xc, yc) = (70, 50): every tile fits
    assert R(0, 70, 50, 64, 48, 64) == (6, 2, 70, 50, 6, 2)
    assert R(1, 70, 50, 64, 48, 64) == (70, 2, 128, 50, 70, 2)            # clipped right: 58 columns
    assert R(2, 70, 50, 64, 48, 64) == (6, 50, 70, 98, 6, 50)
    assert R(3, 70, 50, 64, 48, 64) == (70, 50, 128, 98, 70, 50)
    # centre (32, 32), the lower edge of the range: the top-left tile is cut at the canvas origin and shows its bottom-right corner
    assert R(0, 32, 32, 64, 48, 64) == (0, 0, 32, 32, -32, -16)
    assert R(1, 32, 32, 64, 48, 64) == (32, 0, 96, 32, 32, -16)
    assert R(2, 32, 32, 64, 48, 64) == (0, 32, 32, 80, -32, 32)
    assert R(3, 32, 32, 64, 48, 64) == (32, 32, 96, 80, 32, 32)
    # centre (96, 96), the upper edge: right and bottom tiles are cut at the canvas end
    assert R(0, 96, 96, 64, 48, 64) == (32, 48, 96, 96, 32, 48)
    assert R(1, 96, 96, 64, 48, 64) == (96, 48, 128, 96, 96, 48)
    assert R(2, 96, 96, 64, 48, 64) == (32, 96, 96, 128, 32, 96)
    assert R(3, 96, 96, 64, 48, 64) == (96, 96, 128, 128, 96, 96)
    # a centre on the canvas edges (outside what the reference draws, inside what the table admits): empty rectangles
    assert R(0, 0, 0, 64, 48, 64)[:4] == (0, 0, 0, 0) and R(3, 128, 128, 64, 48, 64)[:4] == (128, 128, 128, 128)


def test_table_layout_and_abi():
    from msod_amd import _lib
    from msod_amd.utils import datasets as D
    assert _lib._consts["CFT_AUG_DESC_BYTES"] == D.AUG_DESC.itemsize == 400 and _lib._consts["CFT_AUG_TILE_BYTES"] == D.AUG_TILE.itemsize == 80
    assert D.AUG_DESC.fields["inv"][1] == 32 and D.AUG_DESC.fields["tile"][1] == 80
    assert "augment.hip" in _lib.SOURCES
    restype, argtypes = _lib.SIGNATURES["cft_augment_batch_u8"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]


def test_descriptors_of_a_recorded_batch():
    from msod_amd.utils import datasets as D
    c = next(c for c in CASES if c["name"] == "b64")
    ds = quiet(AR.make_dataset, ROOT, c)
    rng, np_rng = AR.generators(c["passes"][0]["seed"])
    plans = [ds.item_plan(i, rng, np_rng) for i in range(4)]
    table, luts, HW = D.build_augment_descriptors(plans)
    assert HW == (64, 64) and table.dtype == D.AUG_DESC and luts.shape == (4, 2, 3, 256) and luts.dtype == np.uint8
    for row, lut, p in zip(table, luts, plans):
        assert row["ntiles"] == (4 if p["mosaic"] else 1) and row["warp"] == int(p["mosaic"])
        assert (row["canvas_h"], row["canvas_w"]) == ((128, 128) if p["mosaic"] else (64, 64))
        assert row["flip"] == (D.AUG_FLIPLR if p["fliplr"] else 0) | (D.AUG_FLIPUD if p["flipud"] else 0)
        assert np.array_equal(lut[0], D.hsv_luts(p["gains"][0])) and np.array_equal(lut[1], D.hsv_luts(p["gains"][1]))
        assert not np.array_equal(lut[0], lut[1])                              # the two streams draw their own gains
        if p["mosaic"]:
            M = p["M"]
            a = np.array(row["inv"]).reshape(2, 3)
            assert np.allclose(a[:, :2] @ M[:2, :2], np.eye(2), atol=1e-12) and np.allclose(a[:, :2] @ M[:2, 2] + a[:, 2], 0, atol=1e-9)
            for i, (tile, t) in enumerate(zip(row["tile"], p["tiles"])):
                want = D.mosaic_tile_rects(i, p["xc"], p["yc"], t["w"], t["h"], 64)
                assert tuple(int(tile[k]) for k in ("x1", "y1", "x2", "y2", "padw", "padh")) == want
            assert 32 <= p["xc"] <= 96 and 32 <= p["yc"] <= 96 and p["indices"][0] == p["index"] and len(p["indices"]) == 4
        assert (row["tile"]["src_rgb"] == 0).all()                             # pointers are filled where the sources are known


# ------------------------------------------------------------------------------ refusals
HYP = dict(CASES[0]["hyp"])


def _paths(root=ROOT):
    return os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images")


def test_refusals():
    from msod_amd.utils import datasets as D
    rgb, ir = _paths()
    opt = SimpleNamespace(single_cls=False)
    with pytest.raises(NotImplementedError, match="image_weights"):
        quiet(D.LoadMultiModalImagesAndLabelsAugmented, rgb, ir, 64, 4, hyp=HYP, image_weights=True)
    with pytest.raises(NotImplementedError, match="perspective"):
        quiet(D.LoadMultiModalImagesAndLabelsAugmented, rgb, ir, 64, 4, hyp=dict(HYP, perspective=0.001))
    with pytest.raises(ValueError, match="fliplr"):
        quiet(D.LoadMultiModalImagesAndLabelsAugmented, rgb, ir, 64, 4, hyp={k: v for k, v in HYP.items() if k != "fliplr"})
    with pytest.raises(ValueError, match="hyp"):
        quiet(D.LoadMultiModalImagesAndLabelsAugmented, rgb, ir, 64, 4)
    with pytest.raises(NotImplementedError, match="quad=True"):
        quiet(D.create_train_dataloader_rgb_ir, rgb, ir, 64, 4, 32, opt, HYP, quad=True)
    with pytest.raises(NotImplementedError, match="image_weights"):
        quiet(D.create_train_dataloader_rgb_ir, rgb, ir, 64, 4, 32, opt, HYP, image_weights=True)
    # the two old refusals are unchanged
    with pytest.raises(NotImplementedError, match="augment=True"):
        D.LoadMultiModalImagesAndLabels(rgb, ir, 64, 4, augment=True)
    with pytest.raises(NotImplementedError, match="quad=True"):
        D.create_dataloader_rgb_ir(rgb, ir, 64, 4, 32, opt, quad=True)


def test_a_pair_that_would_be_resized_twice_is_refused_where_the_branch_is_reachable(tmp_path):
    """load_image_rgb_ir resizes to ``int(w0 * r)`` with ``r = 64 / w0`` in floating point: for w0 = 49 that is int(63.99...) = 63, so the
    letterbox to 64 scales the 63-wide image up again.  Reachable with mosaic < 1 or rect, not with mosaic = 1."""
    from PIL import Image
    from msod_amd.utils import datasets as D
    root = str(tmp_path / "dataset")
    shutil.copytree(ROOT, root)
    w0, h0 = 49, 19
    assert int(w0 * (64 / w0)) == 63
    for stream, mode in (("rgb", "RGB"), ("ir", "L")):
        Image.new(mode, (w0, h0)).save(os.path.join(root, stream, "images", "p0_64x64.png"))
    rgb, ir = _paths(root)
    ds = quiet(D.LoadMultiModalImagesAndLabelsAugmented, rgb, ir, 64, 4, hyp=HYP)              # mosaic = 1.0: only tiles
    assert ds.mosaic and len(ds) == 8
    with pytest.raises(ValueError, match="p0_64x64.png.*second time"):
        quiet(D.LoadMultiModalImagesAndLabelsAugmented, rgb, ir, 64, 4, hyp=dict(HYP, mosaic=0.5))
    with pytest.raises(ValueError, match="second time"):
        quiet(D.LoadMultiModalImagesAndLabelsAugmented, rgb, ir, 64, 4, hyp=HYP, rect=True)


# ------------------------------------------------------------------------------ loader seeding
def _summary(plans):
    return [(p["mosaic"], p["yc"], p["xc"], tuple(p["indices"]), p["flipud"], p["fliplr"], tuple(np.concatenate(p["gains"]).tolist()),
             None if p["M"] is None else p["M"].tobytes(), p["labels_out"].numpy().tobytes()) for p in plans]


def test_batch_plans_depend_on_seed_epoch_and_batch_alone():
    from msod_amd.utils import datasets as D
    c = next(c for c in CASES if c["name"] == "b64")
    ds = quiet(AR.make_dataset, ROOT, c)

    def loader(seed=0):
        ld = D.AugmentedPairLoader.__new__(D.AugmentedPairLoader)      # planning only: no device is touched
        ld.dataset, ld.batch_size, ld.seed = ds, 4, seed
        return ld

    a, b = loader(), loader()
    first = [_summary(a.plan_batch(k, 0)) for k in (0, 1)]             # batch 1 after batch 0 ...
    assert _summary(b.plan_batch(1, 0)) == first[1]                    # ... and on its own
    assert _summary(b.plan_batch(0, 0)) == first[0]
    assert first[0] != first[1]
    assert _summary(a.plan_batch(0, 1)) != first[0] and _summary(a.plan_batch(1, 1)) != first[1]       # another epoch
    assert _summary(loader(1).plan_batch(0, 0)) != first[0]            # another seed
    seeds = {D.batch_seed(s, e, k) for s in range(4) for e in range(4) for k in range(4)}
    assert len(seeds) == 64 and all(0 <= x < 1 << 64 for x in seeds)
    import random
    state, np_state = random.getstate(), np.random.get_state()
    a.plan_batch(0, 3)
    assert random.getstate() == state and all(np.array_equal(u, v) for u, v in zip(np.random.get_state(), np_state))   # the global generators are untouched
