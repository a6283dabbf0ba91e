"""GPU tests of cft_augment_batch_u8 (csrc/augment.hip) and the augmented RGB + IR training loader of utils/datasets.py against the
reference's own run recorded in tests/golden/augment/augment_cases.pt and against the numpy restatement tests/augment_ref.py.
Every stage of the raster is integer or singly rounded, so images are compared byte for byte: there is no tie band."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref as AR
from gpu_busy import busy

pytestmark = pytest.mark.gpu

ROOT, CASES = AR.load_cases()
IDS = [c["name"] for c in CASES]
RGB_DIR, IR_DIR = os.path.join(ROOT, "rgb", "images"), os.path.join(ROOT, "ir", "images")
B64 = next(c for c in CASES if c["name"] == "b64")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ------------------------------------------------------------------------------ the recording
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_assembled_batches_equal_the_recorded_images(dev, c):
    from msod_amd.utils import datasets as D
    ds = quiet(AR.make_dataset, ROOT, c)
    for p in c["passes"]:
        rng, np_rng = AR.generators(p["seed"])
        for lo in range(0, len(ds), c["batch_size"]):
            idx = list(range(lo, min(lo + c["batch_size"], len(ds))))
            got, plans = D.assemble_augmented_batch(ds, idx, dev, rng, np_rng, return_plans=True)
            want = torch.stack([p["items"][i]["img"] for i in idx])
            assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == tuple(want.shape)
            assert torch.equal(got.cpu(), want), f"seed {p['seed']} batch {lo // c['batch_size']}: {int((got.cpu() != want).sum())} bytes differ"
            if c is B64 and lo == 0:
                assert {pl["mosaic"] for pl in plans} == {True, False}         # mosaic and letterbox rows in one launch
        assert rng.random() == p["next_random"] and float(np_rng.random_sample()) == p["next_np_random"]


# ------------------------------------------------------------------------------ the kernel against augment_ref on synthetic tables
def _image(g, h, w):
    return g.randint(0, 256, (h, w, 3)).astype(np.uint8)


def _tile(g, h0, w0, h, w, x1, y1, x2, y2, padw, padh):
    return {"rgb": _image(g, h0, w0), "ir": _image(g, h0, w0), "h0": h0, "w0": w0, "h": h, "w": w, "x1": x1, "y1": y1, "x2": x2, "y2": y2,
            "padw": padw, "padh": padh}


def _mosaic_tiles(g, xc, yc, s, sizes):
    """Four tiles around (xc, yc) in a 2s canvas; sizes: (h0, w0, h, w) per tile."""
    from msod_amd.utils.datasets import mosaic_tile_rects
    return [_tile(g, h0, w0, h, w, *mosaic_tile_rects(i, xc, yc, w, h, s)) for i, (h0, w0, h, w) in enumerate(sizes)]


def _affine(angle, scale, shear, tx, ty, canvas):
    """The inverse coefficients of a centre-rotate-shear-translate matrix, as the dataset forms them."""
    from msod_amd.utils.datasets import invert_affine
    C, R, S, T = np.eye(3), np.eye(3), np.eye(3), np.eye(3)
    C[0, 2], C[1, 2] = -canvas[1] / 2, -canvas[0] / 2
    R[:2] = AR.getRotationMatrix2D((0, 0), angle, scale)
    S[0, 1], S[1, 0] = np.tan(np.deg2rad(shear)), np.tan(np.deg2rad(-shear / 2))
    T[0, 2], T[1, 2] = tx, ty
    return invert_affine(T @ S @ R @ C)


def _luts(g, B, identity=False):
    if identity:
        return np.broadcast_to(AR.hsv_luts([1.0, 1.0, 1.0]), (B, 2, 3, 256)).copy()
    return np.stack([np.stack([AR.hsv_luts(g.uniform(-1, 1, 3) * [0.015, 0.7, 0.4] + 1) for _ in range(2)]) for _ in range(B)])


def _launch(dev, rows, luts, H, W, out=None, crop=False):
    """Build the table of python-form ``rows`` (tests/augment_ref.render_row's form), upload the sources, launch.  ``crop``: every source
    is a strided crop view of a larger device tensor."""
    from msod_amd.utils import datasets as D
    table = np.zeros(len(rows), dtype=D.AUG_DESC)
    keep = []
    for row, r in zip(table, rows):
        row["ntiles"], row["warp"], row["canvas_h"], row["canvas_w"], row["flip"] = r["ntiles"], r["warp"], r["canvas_h"], r["canvas_w"], r["flip"]
        row["inv"] = r.get("inv", (0,) * 6)
        for tile, t in zip(row["tile"], r["tiles"]):
            for k in ("h0", "w0", "h", "w", "x1", "y1", "x2", "y2", "padw", "padh"):
                tile[k] = t[k]
            for key in ("rgb", "ir"):
                src = torch.from_numpy(t[key])
                if crop:
                    big = torch.full((src.shape[0] + 5, src.shape[1] + 7, 3), 255, dtype=torch.uint8)
                    big[2:2 + src.shape[0], 3:3 + src.shape[1]] = src
                    view = big.to(dev)[2:2 + src.shape[0], 3:3 + src.shape[1]]
                    assert not view.is_contiguous()
                else:
                    view = src.to(dev)
                keep.append(view)
                tile["src_" + key], tile["stride_" + key] = view.data_ptr(), view.stride(0)
    if out is None:
        out = torch.empty((len(rows), 6, H, W), dtype=torch.uint8, device=dev)
    D.augment_batch(table, luts, out)
    torch.cuda.synchronize()
    return out, table


def _expect(rows, luts, H, W):
    return np.stack([AR.render_row(r, l, H, W) for r, l in zip(rows, luts)])


def _row(tiles, canvas, warp=0, flip=0, inv=(0,) * 6):
    return {"ntiles": len(tiles), "warp": warp, "canvas_h": canvas[0], "canvas_w": canvas[1], "flip": flip, "inv": inv, "tiles": tiles}


def test_eight_rows_with_their_own_warp_luts_and_flips(dev):
    """One launch: copy (r == 1) and resized (enlarged and reduced) tiles in one mosaic, every flip combination, rotations from none to
    one that throws output corners outside the canvas, a letterbox row; 64 x 64 outputs (4 workgroups per image)."""
    g = np.random.RandomState(11)
    s, rows = 64, []
    sizes = [(48, 64, 48, 64), (40, 50, 51, 64), (128, 96, 64, 48), (33, 47, 44, 64)]         # copy, enlarged, halved, odd sizes
    for k in range(7):
        xc, yc = g.randint(32, 97), g.randint(32, 97)
        inv = _affine(angle=(0, 5, -10, 45, 80, 170, -30)[k], scale=(1, 0.6, 1.4, 0.5, 1.2, 0.8, 1.9)[k], shear=(0, 3, -5, 0, 8, 0, 2)[k],
                      tx=32 + g.uniform(-6, 6), ty=32 + g.uniform(-6, 6), canvas=(128, 128))
        rows.append(_row(_mosaic_tiles(g, xc, yc, s, [sizes[(i + k) % 4] for i in range(4)]), (128, 128), warp=1, flip=k % 4, inv=inv))
    rows.append(_row([_tile(g, 30, 40, 48, 64, 0, 8, 64, 56, 0, 8)], (64, 64), flip=3))
    luts = _luts(g, 8)
    got, _ = _launch(dev, rows, luts, 64, 64)
    want = _expect(rows, luts, 64, 64)
    assert np.array_equal(got.cpu().numpy(), want), f"{int((got.cpu().numpy() != want).sum())} bytes differ"
    corners = want[3].reshape(6, 64, 64)[:, [0, 0, 63, 63], [0, 63, 0, 63]]
    grey = AR.apply_hsv_rgb(np.full((1, 1, 3), 114, np.uint8), luts[3][0])[0, 0]
    assert (corners[:3] == grey[:, None]).all()                                  # scale 0.5 at 45 degrees: the output corners miss the canvas


def test_strided_crop_sources_and_a_rect_output_with_partial_workgroups(dev):
    """Sources that are crop views of larger tensors (row stride > 3 w0, pointers off every alignment), a 32 x 96 output (768 groups of
    4 pixels: 3 workgroups per image) and a 20 x 12 one (60 groups: one partial workgroup)."""
    g = np.random.RandomState(12)
    for H, W in ((32, 96), (20, 12)):
        rows = [_row([_tile(g, 21, 37, H - 4, W - 4, 4, 0, W, H - 4, 4, 0)], (H, W), flip=k) for k in (0, 1)]
        rows.append(_row(_mosaic_tiles(g, 40, 50, 64, [(31, 45, 31, 45), (31, 45, 44, 64), (64, 64, 64, 64), (9, 13, 44, 64)]), (128, 128), warp=1,
                         inv=_affine(7, 1.1, 2, W / 2, H / 2, (128, 128))))
        luts = _luts(g, 3)
        got, _ = _launch(dev, rows, luts, H, W, crop=True)
        assert np.array_equal(got.cpu().numpy(), _expect(rows, luts, H, W)), (H, W)


def test_a_centre_that_leaves_a_quadrant_empty_and_pixels_that_miss_every_tile(dev):
    """Centre (0, 40) on the canvas edge: the two left tiles are empty rectangles.  With identity look-up tables a pixel whose four taps
    all miss every tile is the grey 114; with drawn tables it is the table image of that grey."""
    g = np.random.RandomState(13)
    tiles = _mosaic_tiles(g, 0, 40, 64, [(64, 64, 64, 64)] * 4)
    assert tiles[0]["x1"] == tiles[0]["x2"] and tiles[2]["x1"] == tiles[2]["x2"]
    inv = _affine(0, 1.0, 0, 64.0, 32.0, (128, 128))                             # canvas x = output x: the tiles cover canvas x in [0, 64), y in [0, 104)
    rows = [_row(tiles, (128, 128), warp=1, inv=inv)] * 2
    luts = np.concatenate([_luts(g, 1, identity=True), _luts(g, 1)])
    got, _ = _launch(dev, rows, luts, 64, 128)
    got = got.cpu().numpy()
    assert np.array_equal(got, _expect(rows, luts, 64, 128))
    sy, sx, fy, fx = AR.warp_coords(inv, 64, 128)
    miss = (sx >= 64) | (sy + 1 < 0)                                             # both columns of taps right of every tile
    assert miss.any() and (got[0][:, miss] == 114).all()
    for s in (0, 1):
        grey = AR.apply_hsv_rgb(np.full((1, 1, 3), 114, np.uint8), luts[1][s])[0, 0]
        assert (got[1][3 * s:3 * s + 3][:, miss] == grey[:, None]).all()


def test_flip_bits_are_numpy_flips_and_two_runs_are_identical(dev):
    from msod_amd.utils.datasets import AUG_FLIPLR, AUG_FLIPUD
    g = np.random.RandomState(14)
    tiles = _mosaic_tiles(g, 70, 50, 64, [(48, 64, 48, 64), (40, 50, 51, 64), (128, 96, 64, 48), (33, 47, 44, 64)])
    inv = _affine(12, 0.9, 4, 30.0, 34.0, (128, 128))
    rows = [_row(tiles, (128, 128), warp=1, flip=f, inv=inv) for f in (0, AUG_FLIPLR, AUG_FLIPUD, AUG_FLIPLR | AUG_FLIPUD)]
    luts = np.repeat(_luts(g, 1), 4, 0)
    a, _ = _launch(dev, rows, luts, 64, 64)
    b, _ = _launch(dev, rows, luts, 64, 64)
    assert torch.equal(a, b)
    a = a.cpu().numpy()
    assert np.array_equal(a[1], a[0][:, :, ::-1]) and np.array_equal(a[2], a[0][:, ::-1]) and np.array_equal(a[3], a[0][:, ::-1, ::-1])
    assert not np.array_equal(a[1], a[0])


def test_a_table_that_fails_a_guard_raises_and_leaves_out_untouched(dev):
    g = np.random.RandomState(15)
    luts = _luts(g, 1)

    def good():
        return _row(_mosaic_tiles(g, 70, 50, 64, [(48, 64, 48, 64)] * 4), (128, 128), warp=1, inv=_affine(0, 1, 0, 32, 32, (128, 128)))

    def bad(what):
        r = good()
        r["tiles"] = [dict(t) for t in r["tiles"]]
        what(r)
        return r

    cases = {
        "tiles": lambda r: r.update(ntiles=3),
        "outside the canvas": lambda r: r["tiles"][3].update(x2=129),
        "minus its pad": lambda r: r["tiles"][0].update(padw=r["tiles"][0]["padw"] + 1),
        "coefficient": lambda r: r.update(inv=(float("nan"),) + tuple(r["inv"][1:])),
        "image size": lambda r: r["tiles"][1].update(h=0),
        "overlap": lambda r: r["tiles"][1].update(x1=r["tiles"][0]["x2"] - 1, padw=r["tiles"][0]["x2"] - 1),
        "flip": lambda r: r.update(flip=4),
    }
    for match, what in cases.items():
        out = torch.full((1, 6, 64, 64), 7, dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match=match):
            _launch(dev, [bad(what)], luts, 64, 64, out=out)
        torch.cuda.synchronize()
        assert (out == 7).all(), match
    out = torch.full((1, 6, 64, 62), 7, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        _launch(dev, [good()], luts, 64, 62, out=out)
    assert (out == 7).all()


# ------------------------------------------------------------------------------ the loader
def _loader(c, **kw):
    from msod_amd.utils import datasets as D
    return quiet(D.create_train_dataloader_rgb_ir, RGB_DIR, IR_DIR, c["img_size"], c["batch_size"], c["stride"], SimpleNamespace(single_cls=False), c["hyp"],
                 rect=c["rect"], workers=4, seed=5, **kw)


@pytest.mark.parametrize("cache", [False, "device"], ids=["uncached", "cached"])
def test_loader_yields_what_the_direct_form_assembles(dev, cache):
    from msod_amd.utils import datasets as D
    loader, ds = _loader(B64, cache=cache)
    assert isinstance(loader, D.AugmentedPairLoader) and isinstance(ds, D.LoadMultiModalImagesAndLabelsAugmented) and len(loader) == 2
    epochs = []
    for e in (0, 1, 0):
        loader.set_epoch(e)
        it, batches = iter(loader), []
        for b in range(len(loader)):
            if b >= 1 or epochs:                 # the launch path after the first batch makes no host synchronisation
                torch.cuda.set_sync_debug_mode("error")
            try:
                img, targets, paths, shapes = next(it)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert img.dtype == torch.uint8 and img.is_cuda and tuple(img.shape) == (4, 6, 64, 64)
            rng, np_rng = D.batch_generators(5, e, b)
            want, plans = D.assemble_augmented_batch(ds, loader.batch_indices(b), dev, rng, np_rng, return_plans=True)
            assert torch.equal(img, want), (e, b)
            t, pth, shp = ds.plan_targets(plans)                                # the targets are the concatenated plans
            assert targets.dtype == torch.float32 and targets.device.type == "cpu" and torch.equal(targets, t) and paths == pth and shapes == shp
            assert torch.equal(targets[:, 0], torch.cat([torch.full((len(p["labels_out"]),), float(i)) for i, p in enumerate(plans)]))
            assert torch.equal(targets[:, 1:], torch.cat([p["labels_out"][:, 1:] for p in plans]))
            batches.append((img.cpu(), targets.clone()))
        assert next(it, None) is None
        epochs.append(batches)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(epochs[0], epochs[2]))          # the same epoch repeated
    assert not any(torch.equal(a[0], b[0]) for a, b in zip(epochs[0], epochs[1]))                                   # a second epoch differs
    if cache:
        assert all(t is not None and t.is_cuda for t in ds.imgs_rgb)


def test_epochs_advance_on_their_own_and_ranks_take_their_shard(dev):
    from msod_amd.distributed import shard_bounds
    loader, ds = _loader(B64)
    first = [img.cpu() for img, *_ in loader]
    second = [img.cpu() for img, *_ in loader]
    assert loader.epoch == 2 and not torch.equal(first[0], second[0])
    for rank in (0, 1):
        shard, _ = _loader(B64, rank=rank, world_size=2)
        assert list(shard.batch_range) == list(range(*shard_bounds(2, rank, 2)))
        got = [img.cpu() for img, *_ in shard]
        assert len(got) == len(shard) and all(torch.equal(g, first[b]) for g, b in zip(got, shard.batch_range))     # whichever rank assembles it


@pytest.mark.parametrize("cache", [False, "device"], ids=["uncached", "cached"])
def test_augmented_loader_reuses_a_slot_only_after_the_launch_that_read_it(dev, cache):
    """test_gpu_dataset.py's test of the same name, for this loader: one item per batch, slow work queued on the consumer stream before
    every launch, so the slot's table and look-up tables are rewritten for batch k + 2 while batch k's launch is still queued - in the
    pass that fills the device cache and in the one that reads it.  Every batch must still be its own."""
    from msod_amd.utils import datasets as D
    loader, ds = _loader(dict(B64, batch_size=1), cache=cache)
    assert len(loader) == len(ds) > 2
    torch.cuda.synchronize()
    for epoch in (0, 1):
        got, tail = [], None
        busy(dev)
        for img, _, _, _ in loader:
            got.append(img.clone())
            tail = busy(dev)
        pending = not torch.cuda.current_stream().query()                  # the host got here with consumer work still queued
        torch.cuda.synchronize()
        print(f"epoch {epoch}: consumer stream still busy when the host finished: {pending}")
        assert len(got) == len(loader) and tail is not None
        for b, g in enumerate(got):
            want = D.assemble_augmented_batch(ds, loader.batch_indices(b), dev, *D.batch_generators(5, epoch, b))
            assert torch.equal(g, want), f"epoch {epoch}: batch {b}"
    assert all((t is not None) == bool(cache) for t in ds.imgs_rgb)


# ------------------------------------------------------------------------------ closed loop
def test_an_augmented_batch_trains_a_two_stream_model(dev):
    """One augmented batch through a small two-stream Model in train() mode and ComputeLoss: the loss is finite and check() passes, so
    no label is out of range."""
    from msod_amd import ops
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils import datasets as D
    from msod_amd.utils import loss as L
    from msod_amd.utils.seeded import seeded_state_dict
    c = torch.load(os.path.join(os.path.dirname(ROOT), "s_x3_train_96.pt"), weights_only=False)["case"]
    model = Model(named_config(c["cfg"]))
    model.load_state_dict(seeded_state_dict(model.state_dict(), c["seed"]))
    model = model.to(dev).set_compute_dtype(torch.float32)
    model.hyp, model.gr = dict(box=0.05, obj=1.0, cls=0.5, cls_pw=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0), 1.0
    model.train()
    loader, ds = quiet(D.create_train_dataloader_rgb_ir, RGB_DIR, IR_DIR, 128, 4, 32, SimpleNamespace(single_cls=True), B64["hyp"], workers=4, seed=1)
    img, targets, paths, shapes = next(iter(loader))
    assert tuple(img.shape) == (4, 6, 128, 128) and len(targets) > 0
    assert (targets[:, 2:] >= 0).all() and (targets[:, 2:] <= 1).all()
    x = img.float() / 255
    with torch.no_grad():
        ops.manual_dropout_seed(3)
        out = model(x[:, :3].contiguous(), x[:, 3:].contiguous())
    cl = L.ComputeLoss(model)
    loss, items = cl([t.detach().clone().requires_grad_(True) for t in out], targets.to(dev))
    assert torch.isfinite(loss).all() and torch.isfinite(items).all()
    cl.check()
