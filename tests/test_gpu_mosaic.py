"""GPU tests of the batch mosaics: cft_mosaic_compose / _slots / _finish / _area, the two render flags they use and
``plot_images`` / ``evaluate(plots=True)`` against the numpy restatement in tests/mosaic_ref.py.  Every comparison is for equality
(integers, uint8, chains of single roundings); only the fractional area reduction may differ, by one, where the real value lies
within 2^-10 of a tie (``mosaic_ref.assert_area_equal``, the bound of csrc/dataset.hip)."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dataset_ref
import detect_ref
import mosaic_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "dataset")
NAMES = ["person", "car", "bicycle"]


def _plots():
    import msod_amd  # noqa: F401
    from msod_amd.utils import plots
    return plots


def _ops():
    import msod_amd  # noqa: F401
    from msod_amd import ops
    return ops


@pytest.fixture(scope="module")
def atlas():
    """A synthetic 7 x 5 atlas: seeded noise, the space left empty."""
    a = np.random.default_rng(3).integers(0, 256, (96, 7, 5), dtype=np.uint8)
    a[0] = 0
    return a


def batch(B, C, H, W, dtype, seed=0, hi=255.0):
    g = np.random.default_rng(seed)
    if dtype == np.uint8:
        return g.integers(0, 256, (B, C, H, W), dtype=np.uint8)
    return g.uniform(0, hi, (B, C, H, W)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- compose
def gpu_compose(dev, images, c0=0, max_size=640, max_subplots=16):
    """images: a numpy batch or a (possibly strided) CUDA tensor."""
    t = torch.from_numpy(images).to(dev) if isinstance(images, np.ndarray) else images
    g = _plots().mosaic_geometry(t.shape[0], t.shape[2], t.shape[3], max_size, max_subplots)
    out = torch.empty((g.ns * g.h, g.ns * g.w, 3), dtype=torch.uint8, device=dev)
    _ops().mosaic_compose(t, c0, g.bs, g.ns, g.h, g.w, g.resize, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
@pytest.mark.parametrize("B", [5, 17])
def test_compose_grid(dev, dtype, B):
    """7 x 5 images: B = 5 gives ns 3 with four white cells, B = 17 is cut at max_subplots = 16; column-major placement."""
    images = batch(B, 3, 7, 5, dtype, seed=B)
    got = gpu_compose(dev, images)
    ns = 3 if B == 5 else 4
    assert got.shape == (ns * 7, ns * 5, 3) and np.array_equal(got, mosaic_ref.compose_ref(images))
    assert np.array_equal(got[7:14, 0:5], mosaic_ref.to_u8(images[1].astype(np.float32).transpose(1, 2, 0)))          # image 1 sits BELOW image 0
    if B == 5:
        assert (got[14:, 5:] == 255).all() and (got[:, 10:] == 255).all()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_compose_unit_range_is_decided_by_image_0(dev, dtype):
    unit = batch(3, 3, 9, 6, dtype, seed=1, hi=1.0)
    got = gpu_compose(dev, unit)
    assert np.array_equal(got, mosaic_ref.compose_ref(unit)) and got[:9, :6].max() > 200           # x 255
    mixed = unit.copy()
    mixed[0, 1, 4, 2] = 1.5                                                                         # image 0 exceeds 1, image 1 does not: no factor
    got = gpu_compose(dev, mixed)
    assert np.array_equal(got, mosaic_ref.compose_ref(mixed)) and got[:, :6].max() <= 1
    late = unit.copy()
    late[1, 0, 0, 0] = 200.0                                                                        # only image 0 is looked at
    assert np.array_equal(gpu_compose(dev, late), mosaic_ref.compose_ref(late))
    odd = batch(2, 3, 4, 4, np.float32, seed=2, hi=300.0) - 20                                     # below 0 and above 255: clamped; a NaN gives 0
    odd[1, 2, 1, 1] = np.nan
    assert np.array_equal(gpu_compose(dev, odd.astype(dtype)), mosaic_ref.compose_ref(odd.astype(dtype)))


def test_compose_second_stream_of_a_six_channel_batch(dev):
    images = batch(5, 6, 7, 5, np.uint8, seed=4)
    t = torch.from_numpy(images).to(dev)
    want = mosaic_ref.compose_ref(images, 3)
    assert np.array_equal(gpu_compose(dev, t, c0=3), want)
    view = t[:, 3:]
    assert not view.is_contiguous() and np.array_equal(gpu_compose(dev, view), want)                 # the strided view as the input
    unit = batch(2, 6, 6, 4, np.float32, seed=5, hi=1.0)
    unit[0, 0, 0, 0] = 7.0                                                                          # the maximum is over all six channels of image 0
    assert np.array_equal(gpu_compose(dev, unit, c0=3), mosaic_ref.compose_ref(unit, 3))


@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
@pytest.mark.parametrize("H,W,hw", [(75, 100, (48, 64)), (50, 70, (46, 64))])
def test_compose_resize(dev, dtype, H, W, hw):
    images = batch(5, 3, H, W, dtype, seed=H)
    got = gpu_compose(dev, images, max_size=64)
    assert got.shape == (3 * hw[0], 3 * hw[1], 3)
    assert np.array_equal(got, mosaic_ref.compose_ref(images, 0, 64))
    unit = batch(2, 3, H, W, np.float32, seed=W, hi=1.0).astype(dtype) if dtype != np.uint8 else None
    if unit is not None:
        assert np.array_equal(gpu_compose(dev, unit, max_size=64), mosaic_ref.compose_ref(unit, 0, 64))


# ---------------------------------------------------------------------------------------------------------------- slots
def gpu_slots(dev, targets, bs, cap, nc, h, w, sf):
    if isinstance(targets, tuple):
        t = (torch.from_numpy(targets[0]).to(dev), torch.from_numpy(targets[1]).to(dev))
    else:
        t = torch.from_numpy(targets).to(dev)
    slots, flag = _ops().mosaic_slots(t, bs, cap, nc, h, w, sf)
    return slots.cpu().numpy(), int(flag.item())


def slot_rows(dtype, conf):
    """bs = 5 cells of 48 x 64, sf = 0.64: image 0 normalised, 1 in pixels, 2 without targets, 3 normalised with a box leaving the cell,
    4 in pixels with boxes beyond the cell; rows of images 5, 7, -1 and 0.5 are ignored.  Mixed order, > 256 rows for the chunked scan."""
    g = np.random.default_rng(7)
    rows = []
    for _ in range(300):
        i = int(g.choice([0, 1, 3, 4, 5, 7, -1]))
        if i in (0, 3):
            box = [g.uniform(0.1, 0.8), g.uniform(0.1, 0.8), g.uniform(0, 0.4), g.uniform(0, 0.4)]
        else:
            box = [g.uniform(0, 100), g.uniform(0, 75), g.uniform(0, 60), g.uniform(0, 50)]
        rows.append([i, int(g.integers(0, 3))] + box + [g.uniform(0, 1)])
    rows.append([0.5, 1, 0.5, 0.5, 0.1, 0.1, 0.9])
    rows.append([3, 2, 0.05, 0.02, 0.3, 0.2, 0.77])                  # x1, y1 negative
    rows.append([4, 0, 90, 70, 40, 30, 0.5])                          # x2, y2 beyond the cell after * sf
    return np.array(rows, dtype)[:, :7 if conf else 6]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("conf", [False, True])
def test_slots_equal_restatement(dev, dtype, conf):
    rows = slot_rows(dtype, conf)
    got, flag = gpu_slots(dev, rows, 5, 128, 3, 48, 64, 0.64)
    want, wflag = mosaic_ref.slots_ref(rows, 5, 128, 3, 48, 64, 0.64)
    assert flag == wflag == 0 and np.array_equal(got, want)
    assert got[2, :, 6].sum() == 0 and got[0, :, 6].sum() > 10 and (got[3, :, :2] < 0).any()
    # the decision is per image: image 0 was multiplied by (w, h), image 1 by sf
    first0 = rows[rows[:, 0] == 0][0]
    n0 = int(got[0, :, 6].sum())
    if not conf:
        assert got[0, n0 - 1, 0] == int(dtype(first0[2] - first0[4] / dtype(2)) * dtype(64))       # reverse order: the first target in the last used slot
    # without a resize (sf >= 1) pixel boxes are taken as they are
    got, _ = gpu_slots(dev, rows, 5, 128, 3, 75, 100, 1.5)
    assert np.array_equal(got, mosaic_ref.slots_ref(rows, 5, 128, 3, 75, 100, 1.5)[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_slots_normalised_threshold(dev, dtype):
    """A box maximum just below 1.01 (multiplied by w, h) and just above (multiplied by sf), each at least 4 ulps clear of the constant."""
    lo, hi = dtype(1.009999), dtype(1.010001)
    rows = np.array([[0, 0, 0.5, 0.5, 0, 0], [1, 0, 0.5, 0.5, 0, 0]], dtype)
    rows[0, 4], rows[1, 4] = (lo - dtype(0.5)) * dtype(2), (hi - dtype(0.5)) * dtype(2)
    for r, side in ((rows[0], -1), (rows[1], 1)):
        m = r[2] + r[4] / dtype(2)
        assert side * (m - dtype(1.01)) >= 4 * np.spacing(dtype(1.01))
    got, flag = gpu_slots(dev, rows, 2, 1, 1, 48, 64, 0.64)
    want, _ = mosaic_ref.slots_ref(rows, 2, 1, 1, 48, 64, 0.64)
    assert flag == 0 and np.array_equal(got, want)
    assert got[0, 0, 2] == 64 and got[0, 0, 1] == 24 and got[1, 0, 2] == 0 and got[1, 0, 1] == 0


def test_slots_confidence_threshold_tenths_and_reverse_order(dev):
    above = np.nextafter(np.float32(0.25), np.float32(1))
    rows = np.array([[0, 0, 10, 10, 4, 4, 0.25], [0, 1, 20, 20, 4, 4, above], [0, 2, 30, 30, 4, 4, 0.96], [0, 1, 40, 40, 4, 4, 0.75],
                     [0, 0, 5, 5, 2, 2, 0.05], [0, 2, 50, 50, 4, 4, 1.0]], np.float32)
    got, flag = gpu_slots(dev, rows, 1, 6, 3, 100, 100, 1.0)
    assert flag == 0 and np.array_equal(got, mosaic_ref.slots_ref(rows, 1, 6, 3, 100, 100, 1.0)[0])
    assert got[0, :, 6].tolist() == [1, 1, 1, 1, 0, 0]                                             # 0.25 and 0.05 are not drawn
    assert got[0, :4, 4].tolist() == [2, 1, 2, 1] and got[0, :4, 5].tolist() == [10, 8, 10, 3]     # last target first; 0.75 -> 0.8, 0.96 -> 1.0
    assert got[0, 3, :4].tolist() == [18, 18, 22, 22]
    got64, _ = gpu_slots(dev, rows.astype(np.float64), 1, 6, 3, 100, 100, 1.0)
    assert np.array_equal(got64, got)


def test_slots_bad_class_and_overflow_set_their_bits(dev, tmp_path):
    rows = np.array([[0, 0, 10, 10, 4, 4], [0, 3, 20, 20, 4, 4], [0, 1, 30, 30, 4, 4], [0, -1, 5, 5, 2, 2], [0, np.nan, 5, 5, 2, 2], [0, 2, 40, 40, 4, 4]], np.float32)
    got, flag = gpu_slots(dev, rows, 1, 4, 3, 100, 100, 1.0)
    want, wflag = mosaic_ref.slots_ref(rows, 1, 4, 3, 100, 100, 1.0)
    assert flag == wflag == mosaic_ref.BAD_CLASS and np.array_equal(got, want) and got[0, :, 6].tolist() == [1, 1, 1, 0]
    got, flag = gpu_slots(dev, rows, 1, 2, 3, 100, 100, 1.0)                                       # three drawn, two slots
    want, wflag = mosaic_ref.slots_ref(rows, 1, 2, 3, 100, 100, 1.0)
    assert flag == wflag == (mosaic_ref.BAD_CLASS | mosaic_ref.OVERFLOW) and np.array_equal(got, want)
    images = torch.zeros((1, 3, 100, 100), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="class"):
        _plots().plot_images(images, rows, fname=str(tmp_path / "bad.png"), names=NAMES)
    assert not (tmp_path / "bad.png").exists()
    assert _plots().plot_images(images, rows[:1], fname=str(tmp_path / "good.png"), names=NAMES).shape == (100, 100, 3)


def padded_dets(seed=0, B=4, max_det=20):
    g = np.random.default_rng(seed)
    dets = np.zeros((B, max_det, 6), np.float32)
    x1, y1 = g.uniform(-5, 80, (B, max_det)), g.uniform(-5, 50, (B, max_det))
    dets[..., 0], dets[..., 1] = x1, y1
    dets[..., 2], dets[..., 3] = x1 + g.uniform(0, 40, (B, max_det)), y1 + g.uniform(0, 30, (B, max_det))
    dets[..., 4] = g.uniform(0, 1, (B, max_det))
    dets[..., 5] = g.integers(0, 3, (B, max_det))
    dets[0, 0, 4], dets[0, 1, 4] = 0.25, np.nextafter(np.float32(0.25), np.float32(1))
    return dets, np.array(([max_det, 0, 1, 7] * B)[:B], np.int32)


def test_slots_padded_form_equals_output_to_target_rows(dev):
    dets, counts = padded_dets()
    got, flag = gpu_slots(dev, (dets, counts), 4, 20, 3, 48, 64, 0.64)
    rows = mosaic_ref.output_to_target(dets, counts)
    want, _ = mosaic_ref.slots_ref(rows, 4, 20, 3, 48, 64, 0.64)
    assert flag == 0 and rows.dtype == np.float64 and np.array_equal(got, want)
    assert got[:, :, 6].sum(1)[1] == 0 and got[2, :, 6].sum() <= 1 and got[0, :, 6].sum() > 5
    # the same through this package's output_to_target on the device and the float64 row kernel
    out = [torch.from_numpy(dets[i, :counts[i]]).to(dev) for i in range(4)]
    dev_rows = _plots().output_to_target(out)
    assert dev_rows.is_cuda and np.array_equal(dev_rows.cpu().numpy().astype(np.float64), rows)
    slots, _ = _ops().mosaic_slots(dev_rows.double().contiguous(), 4, 20, 3, 48, 64, 0.64)
    assert np.array_equal(slots.cpu().numpy(), got)
    # bs below B: the images beyond are not read
    got2, _ = gpu_slots(dev, (dets, counts), 3, 20, 3, 48, 64, 0.64)
    assert np.array_equal(got2, got[:3])


# ---------------------------------------------------------------------------------------------------------------- render flags
def render_cell(dev, img, slots, has_conf, atlas, signed=True):
    """One HWC uint8 image and its int32 [n, 16] slots through cft_detect_render as plot_images calls it."""
    P = _plots()
    r = P.BoxRenderer(NAMES, dev, 3, hide_conf=not has_conf, atlas=atlas, color_table=mosaic_ref.PALETTE[:3], text_color=mosaic_ref.TEXT_COLOR)
    r.flags |= (P.RENDER_SIGNED if signed else 0) | (P.RENDER_CONF1 if has_conf else 0)
    t = torch.from_numpy(img).to(dev)
    r(torch.from_numpy(slots[None].copy()).to(dev), [t])
    return t.cpu().numpy()


def test_render_tenths_labels(dev, atlas):
    g = np.random.default_rng(1)
    img = g.integers(0, 256, (90, 130, 3), dtype=np.uint8)
    slots = np.zeros((3, 16), np.int32)
    for r, (tn, c) in enumerate(((0, 0), (3, 1), (10, 2))):
        slots[r, :7] = [10 + 5 * r, 25 + 22 * r, 100, 80, c, tn, 1]
    got = render_cell(dev, img, slots, True, atlas)
    want = img.copy()
    mosaic_ref.draw_cell([want], slots, NAMES, True, atlas)
    assert np.array_equal(got, want) and not np.array_equal(got, img)
    # ' d.d' is one character shorter than ' d.dd': the background of slot 0 ends at x1 + (6 + 4) * 5
    assert (got[25 - 5, 10 + 50] == mosaic_ref.PALETTE[0]).all() or (got[25 - 5, 10 + 50] == mosaic_ref.TEXT_COLOR).all()
    assert (got[25 - 5, 10 + 51] == img[25 - 5, 10 + 51]).all()


def test_render_signed_coordinates(dev, atlas):
    g = np.random.default_rng(2)
    img = g.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    slots = np.zeros((4, 16), np.int32)
    slots[0, :7] = [-20, 10, 30, 40, 0, 7, 1]            # starts left of the cell: the label starts at x = -20, only its tail is inside
    slots[1, :7] = [20, -9, 90, 20, 1, 5, 1]             # starts above, ends right of the cell
    slots[2, :7] = [-5, -5, 70, 55, 2, 10, 1]            # surrounds the cell: nothing of its outline is inside
    slots[3, :7] = [-40, -40, -10, -10, 0, 1, 1]         # wholly outside
    for conf in (False, True):
        got = render_cell(dev, img, slots, conf, atlas)
        want = img.copy()
        mosaic_ref.draw_cell([want], slots, NAMES, conf, atlas)
        assert np.array_equal(got, want) and not np.array_equal(got, img)
    assert (got[15, 0] == img[15, 0]).all() and (got[10, 0] == mosaic_ref.PALETTE[0]).all()        # no left edge pulled to the border; the top edge is there
    unsigned = render_cell(dev, img, slots, True, atlas, signed=False)                              # the old clamp pulls the edges to 0
    assert (unsigned[15, 0] == mosaic_ref.PALETTE[0]).all()


def test_render_without_the_new_flags_is_unchanged(dev, atlas):
    """The detect tests' scene (coordinates >= 0) with and without CFT_RENDER_SIGNED: both equal detect_ref.render_ref."""
    import test_gpu_detect as TD
    P = _plots()
    scene = TD.render_scene()
    boxes = torch.from_numpy(detect_ref.pack_slots(scene)).to(dev)
    for extra in (0, P.RENDER_SIGNED):
        host, device, _ = TD.make_images(dev, seed=9)
        r = P.BoxRenderer(TD.NAMES, dev, 3, hide_conf=False, atlas=atlas, color_table=TD.COLORS, text_color=TD.TEXT)
        r.flags |= extra
        r(boxes, [p[0] for p in device], [p[1] for p in device])
        for b in range(3):
            detect_ref.render_ref(host[b], scene, b, TD.COLORS, TD.TEXT, 3, True, True, TD.NAMES, atlas)
            for s in range(2):
                assert np.array_equal(device[b][s].cpu().numpy(), host[b][s]), (extra, b, s)


# ---------------------------------------------------------------------------------------------------------------- finish
def gpu_finish(dev, mosaics, bs, ns, h, w, paths, atlas):
    P = _plots()
    t = [torch.from_numpy(m).to(dev) for m in mosaics]
    codes = lens = at = None
    if paths:
        codes, lens = P._path_codes(paths, bs, dev)
        at = torch.from_numpy(atlas).to(dev)
    _ops().mosaic_finish(t[0], t[1] if len(t) == 2 else None, bs, ns, h, w, codes, lens, at)
    return [x.cpu().numpy() for x in t]


PATHS = ["/data/set/a.png", "dir/0123456789abcdefghijklmnopqrstuvwxyz01234.jpg", "café 中.png", "x", "/deep/er/IMG_0042.jpeg"]


@pytest.mark.parametrize("h,w", [(7, 5), (48, 64), (3, 2)])
@pytest.mark.parametrize("streams", [1, 2])
def test_finish_names_and_borders(dev, atlas, h, w, streams):
    """Five cells of a 3 x 3 grid: text clipped at a 7 x 5 cell, a 45-character name cut at 40, non-ASCII characters as spaces, the
    borders of a partly filled grid (free cells keep none), twice with the same bytes."""
    g = np.random.default_rng(h)
    base = [g.integers(0, 200, (3 * h, 3 * w, 3), dtype=np.uint8) for _ in range(streams)]
    assert len(os.path.basename(PATHS[1])) == 45
    got = gpu_finish(dev, base, 5, 3, h, w, PATHS, atlas)
    want = [m.copy() for m in base]
    mosaic_ref.finish_ref(want, 5, 3, h, w, PATHS, atlas)
    for s in range(streams):
        assert np.array_equal(got[s], want[s]), s
    again = gpu_finish(dev, base, 5, 3, h, w, PATHS, atlas)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    if (h, w) == (48, 64):
        assert (got[0] == 220).all(2).any() and np.array_equal(got[0][2 * h + 2:, 2 * w + 2:], base[0][2 * h + 2:, 2 * w + 2:])      # a free cell's inside is untouched
        assert (got[0][h, :2 * w] == 255).all() and (got[0][:, 2 * w + 1] == 255)[:2 * h].all()
    plain = gpu_finish(dev, base, 5, 3, h, w, None, atlas)
    want = [m.copy() for m in base]
    mosaic_ref.finish_ref(want, 5, 3, h, w, None, None)
    assert all(np.array_equal(a, b) for a, b in zip(plain, want))


# ---------------------------------------------------------------------------------------------------------------- area
@pytest.mark.parametrize("src,dst", [((48, 64), (24, 32)), ((37, 53), (13, 20)), ((40, 40), (10, 10)), ((144, 192), (144, 192))])
def test_area(dev, src, dst):
    img = np.random.default_rng(src[0]).integers(0, 256, (src[0], src[1] + 3, 3), dtype=np.uint8)
    t = torch.from_numpy(img).to(dev)[:, :src[1]]                                                  # a padded row stride
    got = _ops().mosaic_area(t, *dst).cpu().numpy()
    view = np.ascontiguousarray(img[:, :src[1]])
    mosaic_ref.assert_area_equal(got, dataset_ref.resize_area(view, (dst[1], dst[0])), dataset_ref.near_tie(view, (dst[1], dst[0])))
    if src[0] % dst[0] == 0 and src[1] % dst[1] == 0:
        assert np.array_equal(got, dataset_ref.resize_area(view, (dst[1], dst[0])))


def test_area_refuses_more_than_4x(dev):
    t = torch.zeros((41, 41, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="4x"):
        _ops().mosaic_area(t, 10, 10)
    with pytest.raises(ValueError):
        _ops().mosaic_area(t, 42, 41)
    lib = _ops()._lib.load()
    out = torch.zeros((10, 10, 3), dtype=torch.uint8, device=dev)
    assert lib.cft_mosaic_area(t.data_ptr(), t.stride(0), 41, 41, out.data_ptr(), out.stride(0), 10, 10, None) == -1       # CFT_EINVAL from C too
    torch.cuda.synchronize()
    assert int(out.sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- end to end
def label_rows(B, seed, n=40, nc=3):
    g = np.random.default_rng(seed)
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0] = g.integers(0, B, n)
    rows[:, 1] = g.integers(0, nc, n)
    rows[:, 2:4] = g.uniform(0.1, 0.9, (n, 2))
    rows[:, 4:6] = g.uniform(0.05, 0.5, (n, 2))
    return rows


def compare(got, want, marks):
    got = [got] if torch.is_tensor(got) else list(got)
    assert len(got) == len(want)
    for s, (a, b) in enumerate(zip(got, want)):
        a = a.cpu().numpy()
        if marks is None:
            assert np.array_equal(a, b), s
        else:
            mosaic_ref.assert_area_equal(a, b, marks[s])


def test_plot_images_fractional_final_reduction(dev, tmp_path):
    """16 images of 324 x 322: a 1296 x 1288 mosaic saved at int(1296 r) x int(1288 r), r = 1280 / 324 / 4."""
    P = _plots()
    images = batch(16, 3, 324, 322, np.uint8, seed=8)
    rows = label_rows(16, 8)
    paths = [f"/set/img_{i:03d}.png" for i in range(16)]
    got = P.plot_images(torch.from_numpy(images).to(dev), rows, paths, str(tmp_path / "m.png"), NAMES)
    full = P.plot_images(torch.from_numpy(images).to(dev), rows, paths, None, NAMES)               # fname None: the unreduced mosaic
    want_full, _, flag = mosaic_ref.plot_images_ref(images, rows, paths, NAMES, atlas=P.glyph_atlas(), reduce=False)
    compare(full, want_full, None)
    g = P.mosaic_geometry(16, 324, 322)
    assert flag == 0 and tuple(got.shape) == (g.out_h, g.out_w, 3) and g.out_h < 1296 == full.shape[0]
    want, mark = mosaic_ref.area_ref(want_full[0], g.out_h, g.out_w)
    compare(got, [want], [mark])
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m.png")), got.cpu().numpy())


@pytest.mark.parametrize("kind", ["labels", "pred", "empty", "numbers"])
def test_plot_images_two_streams(dev, tmp_path, kind):
    """[5, 6, 64, 96] with labels, with predictions (the padded NMS form) and with paths: both streams equal the restatement, the saved
    files decode to the returned tensors."""
    from PIL import Image
    P = _plots()
    images = batch(5, 6, 64, 96, np.uint8, seed=6)
    t = torch.from_numpy(images).to(dev)
    paths = PATHS
    names = None if kind == "numbers" else NAMES
    if kind == "pred":
        dets, counts = padded_dets(seed=3, B=5)[0], np.array([20, 0, 1, 7, 12], np.int32)
        targets, ref_targets, cap = (torch.from_numpy(dets).to(dev), torch.from_numpy(counts).to(dev)), (dets, counts), 20
    elif kind == "empty":
        targets, ref_targets, cap = np.zeros((0, 6), np.float32), np.zeros((0, 6), np.float32), None
    else:
        targets, ref_targets, cap = label_rows(5, 5), label_rows(5, 5), None
    got = P.plot_images(t, targets, paths, str(tmp_path / "m.png"), names)
    want, marks, flag = mosaic_ref.plot_images_ref(images, ref_targets, paths, names, atlas=P.glyph_atlas(), cap=cap)
    assert isinstance(got, tuple) and len(got) == 2 and marks is None and flag == 0 and tuple(got[0].shape) == (192, 288, 3)
    compare(got, want, None)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m.png")), got[0].cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m_ir.png")), got[1].cpu().numpy())
    if kind in ("labels", "pred"):
        drawn = (want[0] != mosaic_ref.plot_images_ref(images, np.zeros((0, 6), np.float32), paths, names, atlas=P.glyph_atlas())[0][0]).any(2)
        assert drawn.any() and np.array_equal(want[0][drawn], want[1][drawn])                      # the same boxes in both streams
    if kind == "labels":
        P.plot_images(t, torch.from_numpy(targets).to(dev), paths, str(tmp_path / "d.jpg"), names)   # device rows; a JPEG name
        assert (tmp_path / "d.jpg").stat().st_size > 0 and (tmp_path / "d_ir.jpg").stat().st_size > 0
        assert Image.open(tmp_path / "d.jpg").size == (288, 192)
        one = P.plot_images(t[:, :3], targets, paths, None, names)                                   # three channels: one tensor
        assert torch.is_tensor(one) and torch.equal(one, got[0])


def test_plot_images_device_stage_does_not_synchronise(dev):
    P = _plots()
    t = torch.from_numpy(batch(5, 6, 64, 96, np.uint8, seed=6)).to(dev)
    rows = label_rows(5, 5)
    rows_dev = torch.from_numpy(rows).to(dev)
    dets, counts = padded_dets(seed=3, B=5)
    pair = (torch.from_numpy(dets).to(dev), torch.from_numpy(counts).to(dev))
    P.plot_images(t, rows, PATHS, None, NAMES)                  # tables and the atlas are built on first use
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = P.plot_images(t, rows, PATHS, None, NAMES)
        b = P.plot_images(t, rows_dev, PATHS, None, NAMES)
        c = P.plot_images(t, pair, PATHS, None, NAMES)
        d = P.plot_images(t.half(), np.zeros((0, 6)), None, None, None, max_size=48)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and c[0].shape == a[0].shape and tuple(d[0].shape) == (96, 144, 3)


# ---------------------------------------------------------------------------------------------------------------- evaluate(plots=True)
def test_evaluate_plots(dev, tmp_path):
    """The ten pairs of tests/golden/dataset (the loader keeps eight: one is too small, one has duplicate labels) in batches of two,
    so four batches of which the first three are plotted, the seeded tiny model: twelve files, the label mosaics equal plot_images
    called by hand, the metrics equal those of a run without plots."""
    from PIL import Image
    from msod_amd.evaluate import evaluate
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils import datasets as D
    from msod_amd.utils.seeded import seeded_state_dict
    P = _plots()
    model = Model(named_config("cfg2"))
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    model = model.to(dev)
    with contextlib.redirect_stdout(io.StringIO()):
        loader, _ = D.create_dataloader_rgb_ir(os.path.join(DATA, "rgb", "images"), os.path.join(DATA, "ir", "images"), 64, 2, 32,
                                               SimpleNamespace(single_cls=True), pad=0.5, rect=True)
    batches = [(img.clone(), t.clone(), p, s) for img, t, p, s in loader]
    assert len(batches) == 4
    plain = evaluate(model, batches, 1, single_cls=True)
    got = evaluate(model, batches, 1, single_cls=True, plots=True, save_dir=str(tmp_path / "run"), names=["object"])
    np.testing.assert_equal(got[0], plain[0])
    np.testing.assert_equal(np.asarray(got[1]), np.asarray(plain[1]))
    files = sorted(f.name for f in (tmp_path / "run").iterdir())
    assert files == sorted(f"test_batch{i}_{k}{s}.jpg" for i in range(3) for k in ("labels", "pred") for s in ("", "_ir"))
    for i, (img, targets, paths, _) in enumerate(batches[:3]):
        P.plot_images(img.to(dev), targets, paths, str(tmp_path / f"hand{i}.jpg"), ["object"])
        for s in ("", "_ir"):
            a, b = Image.open(tmp_path / "run" / f"test_batch{i}_labels{s}.jpg"), Image.open(tmp_path / f"hand{i}{s}.jpg")
            assert a.size == b.size and np.array_equal(np.asarray(a), np.asarray(b)), (i, s)
            assert Image.open(tmp_path / "run" / f"test_batch{i}_pred{s}.jpg").size == a.size
