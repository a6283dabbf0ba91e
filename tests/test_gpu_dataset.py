"""GPU tests of cft_pair_batch_u8 (csrc/dataset.hip) and the RGB + IR loader of utils/datasets.py against the reference's own run
recorded in tests/golden/dataset/dataset_cases.pt, oracle/letterbox_oracle.py (INTER_LINEAR) and tests/dataset_ref.py (INTER_AREA)."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dataset_ref as DR
from gpu_busy import busy as _busy
from oracle import letterbox_oracle as LO

pytestmark = pytest.mark.gpu

ROOT, CASES, BLOCKS = DR.load_cases()
IDS = [DR.case_id(c) for c in CASES]
RGB_DIR, IR_DIR = os.path.join(ROOT, "rgb", "images"), os.path.join(ROOT, "ir", "images")
VAL = next(c for c in CASES if c["img_size"] == 64 and c["rect"] and c["pad"] == 0.5 and c["batch_size"] == 4 and not c["single_cls"])   # test.py's form


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def expected_block(rgb, ir, h, w, top, left, mode, H, W):
    """(block uint8 [6, H, W], may_differ bool [6, H, W]) of one pair from HWC RGB originals, by the CPU restatements."""
    from msod_amd.utils import datasets as D
    block, mark = np.full((6, H, W), 114, np.uint8), np.zeros((6, H, W), bool)
    for s, img in enumerate((rgb, ir)):
        if mode == D.PAIR_COPY:
            res = img
        elif mode == D.PAIR_LINEAR:
            res = LO.resize(img, (w, h))
        else:
            res = DR.resize_area(img, (w, h))
            mark[3 * s:3 * s + 3, top:top + h, left:left + w] = DR.near_tie(img, (w, h)).transpose(2, 0, 1)
        block[3 * s:3 * s + 3, top:top + h, left:left + w] = res.transpose(2, 0, 1)
    return block, mark


def assert_block(got, want, mark, what):
    """Byte for byte outside ``mark``; at most 1 LSB inside it."""
    got, want = got.astype(np.int16), np.asarray(want).astype(np.int16)
    diff = np.abs(got - want)
    print(f"{what}: {int((diff > 0).sum())} bytes differ, all among the {int(mark.sum())} within 2^-10 of a tie; max diff {int(diff.max())}")
    assert not (diff[~mark] > 0).any(), what
    assert diff.max() <= 1, what


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_recorded_batches(dev, c):
    """copy, linear and integer-scale area pairs equal the reference's batch byte for byte, border and plane order included;
    fractional-area pairs may be 1 LSB off only where the float64 restatement is within 2^-10 of a tie."""
    from msod_amd.utils import datasets as D
    ds = quiet(DR.make_dataset, ROOT, c)
    bs = min(c["batch_size"], len(ds))
    seen = set()
    for b, want in enumerate(c["batches"]):
        idx = list(range(b * bs, min((b + 1) * bs, len(ds))))
        got = D.assemble_batch(ds, idx, dev).cpu().numpy()
        desc, (H, W) = ds.build_descriptors(idx)
        assert got.shape == (len(idx), 6, H, W)
        for k, (i, row) in enumerate(zip(idx, desc)):
            recorded = BLOCKS[want["blocks"][k]].numpy()
            mode, exact = int(row["mode"]), True
            mark = np.zeros(recorded.shape, bool)
            if mode == D.PAIR_AREA and not DR.is_integer_scale((row["h0"], row["w0"]), (row["h"], row["w"])):
                exact = False
                _, mark = expected_block(*ds.load_pair(i), row["h"], row["w"], row["top"], row["left"], mode, H, W)
            seen.add((D.PAIR_MODE_NAMES[mode], exact))
            assert_block(got[k], recorded, mark, f"{want['paths'][k]} {D.PAIR_MODE_NAMES[mode]}{'' if exact else ' (fractional)'}")
    assert {("linear", True), ("area", True), ("area", False)} <= seen and (("copy", True) in seen) == (c["img_size"] == 64)


def _sources(dev):
    """Four synthetic pairs, one per path of the kernel, two of them crop views of larger images (row strides 3 * 91 and 3 * 131)."""
    from msod_amd.utils import datasets as D
    g = np.random.RandomState(5)
    big = [g.randint(0, 256, (80, 91, 3)).astype(np.uint8), g.randint(0, 256, (80, 91, 3)).astype(np.uint8),
           g.randint(0, 256, (90, 131, 3)).astype(np.uint8), g.randint(0, 256, (90, 131, 3)).astype(np.uint8)]
    big_d = [torch.from_numpy(a).to(dev) for a in big]
    host = [(big[0][7:71, 13:77], big[1][9:73, 5:69]),                                                 # 64x64 copy, crop views
            (g.randint(0, 256, (5, 7, 3)).astype(np.uint8), g.randint(0, 256, (5, 7, 3)).astype(np.uint8)),      # 7x5 -> 64x45 linear
            (big[2][3:78, 11:111], big[3][10:85, 30:130]),                                             # 100x75 -> 64x48 area, crop views
            (g.randint(0, 256, (96, 128, 3)).astype(np.uint8), g.randint(0, 256, (96, 128, 3)).astype(np.uint8))]  # 128x96 -> 64x48 integer area
    device = [(big_d[0][7:71, 13:77], big_d[1][9:73, 5:69]), tuple(torch.from_numpy(a).to(dev) for a in host[1]),
              (big_d[2][3:78, 11:111], big_d[3][10:85, 30:130]), tuple(torch.from_numpy(a).to(dev) for a in host[3])]
    geometry = [(64, 64, 0, 0, D.PAIR_COPY), (45, 64, 9, 0, D.PAIR_LINEAR), (48, 64, 8, 0, D.PAIR_AREA), (48, 64, 3, 0, D.PAIR_AREA)]
    return host, device, geometry


def _table(device, geometry, rows, flip=0):
    from msod_amd.utils import datasets as D
    desc = np.zeros(len(rows), D.PAIR_DESC)
    for r, k in zip(desc, rows):
        h, w, top, left, mode = geometry[k]
        r["h0"], r["w0"], r["h"], r["w"], r["top"], r["left"], r["mode"], r["flip"] = *device[k][0].shape[:2], h, w, top, left, mode, flip
    D._fill_sources(desc, [device[k] for k in rows])
    return desc


def test_mixed_batch_strides_single_pair_and_guard_band(dev):
    from msod_amd.utils import datasets as D
    host, device, geometry = _sources(dev)
    assert device[0][0].stride(0) == 3 * 91 and device[2][1].stride(0) == 3 * 131 and not device[0][0].is_contiguous()
    H = W = 64
    want = [expected_block(*host[k], *geometry[k], H, W) for k in range(4)]
    # one launch, every mode, four source sizes, strided sources
    got = D.pair_batch(_table(device, geometry, range(4)), torch.empty((4, 6, H, W), dtype=torch.uint8, device=dev)).cpu().numpy()
    for k in range(4):
        assert_block(got[k], *want[k], f"mixed batch pair {k}")
    assert not want[0][1].any() and not want[1][1].any() and not want[3][1].any()          # only the fractional pair has a tie band
    # BGR sources with the flip flag: the same planes
    bgr = [tuple(t.flip(2).contiguous() for t in pair) for pair in device]
    flipped = D.pair_batch(_table(bgr, geometry, range(4), flip=1), torch.empty((4, 6, H, W), dtype=torch.uint8, device=dev)).cpu().numpy()
    assert np.array_equal(flipped, got)
    # B = 1, each pair alone
    for k in range(4):
        one = D.pair_batch(_table(device, geometry, [k]), torch.empty((1, 6, H, W), dtype=torch.uint8, device=dev)).cpu().numpy()
        assert np.array_equal(one[0], got[k])
    # a pre-filled buffer between two guard bands: every byte of the batch is written, none outside it
    G, n = 4096, 4 * 6 * H * W
    for fill in (0xAA, 0x55):
        buf = torch.full((G + n + G,), fill, dtype=torch.uint8, device=dev)
        D.pair_batch(_table(device, geometry, range(4)), buf[G:G + n].view(4, 6, H, W))
        out = buf.cpu().numpy()
        assert (out[:G] == fill).all() and (out[G + n:] == fill).all()
        assert np.array_equal(out[G:G + n].reshape(4, 6, H, W), got)


def test_a_letterbox_wider_than_one_tile_and_a_4x_reduction(dev):
    """640 x 512 from 1280 x 1024 (integer) and 1279 x 1023 (fractional): several 256-wide tiles per row, a span that needs the narrow
    tile; and the largest reduction the guard admits."""
    from msod_amd.utils import datasets as D
    g = np.random.RandomState(9)
    cases = [((1024, 1280), (512, 640), (512, 640)), ((1023, 1279), (511, 639), (512, 640)), ((128, 256), (32, 64), (32, 64)), ((127, 255), (32, 64), (32, 64))]
    for (h0, w0), (h, w), (H, W) in cases:
        rgb, ir = (g.randint(0, 256, (h0, w0, 3)).astype(np.uint8) for _ in range(2))
        top, left = (H - h) // 2, (W - w) // 2
        device = [tuple(torch.from_numpy(a).to(dev) for a in (rgb, ir))]
        got = D.pair_batch(_table(device, [(h, w, top, left, D.PAIR_AREA)], [0]), torch.empty((1, 6, H, W), dtype=torch.uint8, device=dev)).cpu().numpy()
        assert_block(got[0], *expected_block(rgb, ir, h, w, top, left, D.PAIR_AREA, H, W), f"{w0}x{h0} -> {w}x{h}")


def test_guards_return_a_status_and_launch_nothing(dev):
    from msod_amd.utils import datasets as D
    host, device, geometry = _sources(dev)
    out = torch.full((1, 6, 64, 64), 7, dtype=torch.uint8, device=dev)

    def bad(k, **change):
        desc = _table(device, geometry, [k])
        for name, v in change.items():
            desc[0][name] = v
        return desc

    for desc, why in [(bad(0, top=1), "does not fit"), (bad(0, left=-1), "does not fit"), (bad(0, mode=3), "unknown resize mode"),
                      (bad(0, h=63), "copy mode"), (bad(1, h=4), "enlarging"), (bad(2, h=4, top=0), "4x"), (bad(2, stride_rgb=299), "row stride"),
                      (bad(3, src_ir=0), "null source"), (bad(0, flip=2), "channel-order")]:
        with pytest.raises(RuntimeError, match=why):
            D.pair_batch(desc, out)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        D.pair_batch(_table(device, [(64, 62, 0, 0, D.PAIR_COPY)], [0]), torch.empty((1, 6, 64, 62), dtype=torch.uint8, device=dev))
    assert (out == 7).all()


@pytest.mark.parametrize("c", [VAL, next(c for c in CASES if c["img_size"] == 32 and c["rect"] and c["batch_size"] == 1 and c["pad"] == 0.5)],
                         ids=["val-bs4", "s32-bs1"])
def test_loader_end_to_end(dev, c):
    from msod_amd.utils import datasets as D
    opt = SimpleNamespace(single_cls=False)
    kw = dict(pad=c["pad"], rect=c["rect"], workers=4)
    loader, ds = quiet(D.create_dataloader_rgb_ir, RGB_DIR, IR_DIR, c["img_size"], c["batch_size"], c["stride"], opt, cache='device', **kw)
    plain_loader, plain_ds = quiet(D.create_dataloader_rgb_ir, RGB_DIR, IR_DIR, c["img_size"], c["batch_size"], c["stride"], opt, **kw)
    assert len(loader) == len(c["batches"]) and not hasattr(loader, "sampler")
    first = [(img.clone(), t, p, s) for img, t, p, s in loader]
    assert all(t is not None and t.is_cuda and t.dtype == torch.uint8 for t in ds.imgs_rgb + ds.imgs_ir)
    second = [(img.clone(), t, p, s) for img, t, p, s in loader]
    uncached = [(img.clone(), t, p, s) for img, t, p, s in plain_loader]
    assert all(t is None for t in plain_ds.imgs_rgb)
    assert len(first) == len(second) == len(uncached) == len(c["batches"])
    for b, (one, two, three, want) in enumerate(zip(first, second, uncached, c["batches"])):
        direct = D.assemble_batch(plain_ds, loader.batch_indices(b), dev)           # no prefetch, no staging buffers
        for img, targets, paths, shapes in (one, two, three):
            assert img.is_cuda and img.dtype == torch.uint8 and torch.equal(img, direct)
            assert targets.device.type == "cpu" and torch.equal(targets, want["targets"])
            assert [os.path.relpath(p, ROOT) for p in paths] == want["paths"] and DR.plain(shapes) == want["shapes"]


def test_loader_reuses_a_slot_only_after_the_launch_that_read_it(dev):
    """The host runs ahead of the consumer stream: slow work is queued there before every batch's launch, the loop body waits for
    nothing, and with one pair per batch the slot's table is rewritten for batch k + 2 while batch k's launch is still queued - in
    the pass that fills the device cache, in the passes that read it, and without a cache.  Every batch must still be its own."""
    from msod_amd.utils import datasets as D
    c = next(c for c in CASES if c["img_size"] == 64 and c["rect"] and c["batch_size"] == 1 and c["pad"] == 0.5)
    opt = SimpleNamespace(single_cls=False)
    kw = dict(pad=c["pad"], rect=True, workers=4)
    cached, ds = quiet(D.create_dataloader_rgb_ir, RGB_DIR, IR_DIR, 64, 1, c["stride"], opt, cache='device', **kw)
    plain_loader, _ = quiet(D.create_dataloader_rgb_ir, RGB_DIR, IR_DIR, 64, 1, c["stride"], opt, **kw)
    direct = [D.assemble_batch(ds, cached.batch_indices(b), dev) for b in range(len(cached))]
    assert len({tuple(d.shape) for d in direct}) > 1                       # consecutive batches differ in shape and in source sizes
    torch.cuda.synchronize()
    for what, loader in (("cache-filling pass", cached), ("cached pass", cached), ("cached pass 2", cached), ("uncached", plain_loader)):
        got, tail = [], None
        _busy(dev)
        for img, _, _, _ in loader:
            got.append(img.clone())
            tail = _busy(dev)
        pending = not torch.cuda.current_stream().query()                  # the host got here with consumer work still queued
        torch.cuda.synchronize()
        print(f"{what}: consumer stream still busy when the host finished: {pending}")
        assert len(got) == len(direct) and tail is not None
        for b, (g, d) in enumerate(zip(got, direct)):
            assert torch.equal(g, d), f"{what}: batch {b}"


def test_a_letterbox_that_resizes_again_takes_the_letterbox_pair_path(dev, tmp_path):
    """Not reachable through the class's own shapes: the batch shape is forced below the resized images.  The batch is then the
    load_image_rgb_ir resize followed by the letterbox's own INTER_LINEAR resize and border, as the reference composes them; the
    pairs picked take the bit-exact modes (copy, linear, integer-scale area), so the result is byte for byte."""
    from msod_amd.utils import datasets as D
    names = ["p0_64x64.png", "p1_128x96.png", "p2_96x128.png", "p6_40x32.png"]
    for stream in ("rgb", "ir"):
        with open(tmp_path / (stream + ".txt"), "w") as f:
            f.writelines(os.path.join(ROOT, stream, "images", n) + "\n" for n in names)
    loader, ds = quiet(D.create_dataloader_rgb_ir, str(tmp_path / "rgb.txt"), str(tmp_path / "ir.txt"), 64, 4, 32, SimpleNamespace(single_cls=False),
                       rect=True, cache='device')
    assert len(ds) == 4 and len(loader) == 1
    ds.batch_shapes_rgb = np.array([[32, 48]])
    H, W = 32, 48
    want = np.full((4, 6, H, W), 114, np.uint8)
    modes = set()
    for k in range(4):
        h0, w0, h, w, top, left, mode, hw, ratio, _ = ds.pair_geometry(k)
        assert hw == (H, W) and ratio[0] < 1 and not (mode == D.PAIR_AREA and not DR.is_integer_scale((h0, w0), (h, w)))
        modes.add(mode)
        nh, nw = int(round(h * ratio[0])), int(round(w * ratio[0]))
        for s, img in enumerate(ds.load_pair(k)):
            first = img if mode == D.PAIR_COPY else LO.resize(img, (w, h)) if mode == D.PAIR_LINEAR else DR.resize_area(img, (w, h))
            want[k, 3 * s:3 * s + 3, top:top + nh, left:left + nw] = LO.resize(np.ascontiguousarray(first), (nw, nh)).transpose(2, 0, 1)
    assert modes == {D.PAIR_COPY, D.PAIR_LINEAR, D.PAIR_AREA}
    for what in ("first pass", "cached pass"):
        (img, targets, paths, shapes), = list(loader)
        assert tuple(img.shape) == (4, 6, H, W) and np.array_equal(img.cpu().numpy(), want), what
        t, p, s = ds.batch_targets([0, 1, 2, 3])
        assert torch.equal(targets, t) and paths == p and shapes == s
    assert np.array_equal(D.assemble_batch(ds, [0, 1, 2, 3], dev).cpu().numpy(), want)


def _small_model(dev):
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_state_dict
    model = Model(named_config("cfg2"))
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    return model.to(dev)


def test_evaluate_over_the_loader_equals_evaluate_over_its_batches(dev):
    from msod_amd.evaluate import evaluate
    from msod_amd.utils import datasets as D
    model = _small_model(dev)
    nc = model.model[-1].nc
    loader, _ = quiet(D.create_dataloader_rgb_ir, RGB_DIR, IR_DIR, 64, 4, 32, SimpleNamespace(single_cls=False), pad=0.5, rect=True)
    got = evaluate(model, loader, nc)
    batches = [(img.clone(), t.clone(), p, s) for img, t, p, s in loader]
    want = evaluate(model, batches, nc)
    np.testing.assert_equal(got[0], want[0])
    np.testing.assert_equal(np.asarray(got[1]), np.asarray(want[1]))


def test_autoanchor_takes_the_dataset_object(dev):
    from msod_amd.utils import autoanchor as aa
    ds = quiet(DR.make_dataset, ROOT, VAL)
    twin = SimpleNamespace(shapes=ds.shapes.copy(), labels=[l.copy() for l in ds.labels])
    results = []
    for d in (ds, twin):
        np.random.seed(3)
        k = quiet(aa.kmean_anchors, d, n=9, img_size=64, gen=10, verbose=False)
        model = _small_model(dev)
        np.random.seed(3)
        quiet(aa.check_anchors_rgb_ir, d, model, thr=4.0, imgsz=64)
        results.append((k, model.model[-1].anchors.cpu().clone(), model.model[-1].anchor_grid.cpu().clone()))
    assert results[0][0].shape == (9, 2) and np.array_equal(results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1]) and torch.equal(results[0][2], results[1][2])
