"""Host tests of the batch mosaics (no GPU): the grid and final-size formulas of ``plot_images`` against hand-evaluated values of the
reference's (utils/plots.py:142-152, :199-200), the tenths routine against Python's '%.1f', ``output_to_target`` against the
reference's loop, the ``_ir`` file name, the refusals that come before any device work, the ABI of the four new entry points and the
two new render flags, and a few direct looks at the restatement in tests/mosaic_ref.py."""
import ctypes
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

import mosaic_ref

import msod_amd  # noqa: F401
from msod_amd import _lib
from msod_amd.utils import plots


@pytest.mark.parametrize("B,H,W,max_size,want", [(5, 75, 100, 64, (5, 3, 48, 64)),        # sf = 0.64: ceil(48.0), ceil(64.0)
                                                 (5, 50, 70, 64, (5, 3, 46, 64)),         # sf = 64 / 70: ceil(45.71), 64
                                                 (1, 700, 700, 640, (1, 1, 640, 640)),
                                                 (2, 1024, 1280, 640, (2, 2, 512, 640)),
                                                 (4, 64, 96, 640, (4, 2, 64, 96)),        # sf > 1: never enlarged
                                                 (17, 7, 5, 640, (16, 4, 7, 5))])         # max_subplots = 16
def test_grid_geometry(B, H, W, max_size, want):
    g = plots.mosaic_geometry(B, H, W, max_size)
    assert (g.bs, g.ns, g.h, g.w) == want
    assert g.resize == (max_size / max(H, W) < 1)
    assert mosaic_ref.geometry(B, H, W, max_size)[:2] + mosaic_ref.geometry(B, H, W, max_size)[3:5] == want


def test_final_size():
    g = plots.mosaic_geometry(5, 75, 100, 64)
    assert (g.ns, g.h, g.w, g.out_h, g.out_w, g.r) == (3, 48, 64, 144, 192, 1.0)
    g = plots.mosaic_geometry(16, 640, 640)
    assert (g.ns, g.out_h, g.out_w) == (4, 1280, 1280) and g.r == 0.5
    g = plots.mosaic_geometry(64, 640, 640, max_subplots=64)               # 5120 -> 1280: exactly the kernel's 4x
    assert (g.ns, g.out_h, g.out_w, g.r) == (8, 1280, 1280, 0.25)
    g = plots.mosaic_geometry(16, 324, 322)                                 # a fractional reduction: r = 1280 / 324 / 4
    assert (g.ns, g.h, g.w) == (4, 324, 322) and (g.out_h, g.out_w) == (int(4 * 324 * g.r), int(4 * 322 * g.r)) and g.r < 1
    assert mosaic_ref.geometry(16, 324, 322)[5:] == (g.out_h, g.out_w)


def test_reduction_beyond_4x_is_refused_before_any_device_work():
    with pytest.raises(ValueError, match="smaller per axis"):
        plots.mosaic_geometry(64, 2000, 2000, max_size=2000, max_subplots=64)
    # plot_images computes the geometry before it touches the device: a tensor without storage is enough to meet the refusal
    with pytest.raises(ValueError, match="smaller per axis"):
        plots.plot_images(torch.empty((64, 3, 2000, 2000), dtype=torch.uint8, device="meta"), np.zeros((0, 6)), max_size=2000, max_subplots=64)


def _neighbours(x):
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return [struct.unpack("<f", struct.pack("<I", v))[0] for v in (u - 1, u, u + 1)]


def test_tenths_equal_python_formatting():
    vals = []
    for k in range(1, 21):                               # every tie k / 20 (0.05, 0.15, ..., 0.25, 0.75, 0.95) and every x.x, with float32 neighbours
        vals += _neighbours(float(np.float32(k / 20)))
    g = np.random.default_rng(11)
    vals += g.uniform(0, 1, 3000).astype(np.float32).tolist()
    doubles = [0.25, 0.75, 0.05, 0.15, 0.35, 0.45, 0.95, 0.9499999999999999, 0.9500000000000001, 0.25000000000000006, 0.24999999999999997, 1e-12,
               2.0 ** -1074, 0.0, 1.0] + g.uniform(0, 1, 2000).tolist()
    for v in vals + doubles:
        t = mosaic_ref.tenths(v)
        assert '%.1f' % v == f"{t // 10}.{t % 10}", v
    assert mosaic_ref.tenths(0.25) == 2 and mosaic_ref.tenths(0.75) == 8             # exact binary ties go to even
    assert mosaic_ref.tenths(np.float32(0.25) + np.float32(2.0 ** -25)) == 3
    assert [mosaic_ref.tenths(v) for v in (-0.3, float("nan"), float("inf"), 1.04, 7.0)] == [0, 0, 10, 10, 10]


def test_header_constants_and_signatures():
    c = _lib._consts
    assert (c["CFT_RENDER_LABELS"], c["CFT_RENDER_CONF"], c["CFT_RENDER_CONF1"], c["CFT_RENDER_SIGNED"]) == (1, 2, 4, 8)
    assert (plots.RENDER_CONF1, plots.RENDER_SIGNED) == (4, 8)
    assert (c["CFT_MOSAIC_U8"], c["CFT_MOSAIC_F16"], c["CFT_MOSAIC_F32"], c["CFT_MOSAIC_BAD_CLASS"], c["CFT_MOSAIC_OVERFLOW"]) == (0, 1, 2, 1, 2)
    assert c["CFT_MOSAIC_NAME_CHARS"] == 40
    i, l, v = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert _lib.SIGNATURES["cft_mosaic_compose"] == (i, [v, i, i, i, i, i, l, l, l, l, i, i, i, i, i, i, v, l, v, v])
    assert _lib.SIGNATURES["cft_mosaic_slots"] == (i, [v, i, i, i, v, v, i, i, i, i, i, i, i, v, v, v, v])
    assert _lib.SIGNATURES["cft_mosaic_finish"] == (i, [v, v, l, l, i, i, i, i, v, v, v, i, i, v])
    assert _lib.SIGNATURES["cft_mosaic_area"] == (i, [v, l, i, i, v, l, i, i, v])
    assert len(_lib.SIGNATURES["cft_detect_render"][1]) == 17                # unchanged
    assert "mosaic.hip" in _lib.SOURCES


def test_evaluate_plots_needs_a_save_dir():
    from msod_amd.evaluate import evaluate
    with pytest.raises(ValueError, match="save_dir"):
        evaluate(None, [], 1, plots=True)


def test_output_to_target_equals_reference_loop():
    g = torch.Generator().manual_seed(3)
    output = [torch.rand((n, 6), generator=g) * torch.tensor([640, 512, 640, 512, 1, 5.]) for n in (3, 0, 7, 1)]
    got = plots.output_to_target(output)
    assert got.dtype == torch.float32 and tuple(got.shape) == (11, 7) and got.device == output[0].device
    max_det = 7
    dets, counts = np.zeros((4, max_det, 6), np.float32), np.array([3, 0, 7, 1])
    for i, o in enumerate(output):
        dets[i, :len(o)] = o.numpy()
    want = mosaic_ref.output_to_target(dets, counts)                          # float64, box values computed in float32
    assert want.dtype == np.float64 and np.array_equal(got.numpy().astype(np.float64), want)
    assert want[3, 0] == 2 and want[0, 2] == (np.float32(dets[0, 0, 0]) + np.float32(dets[0, 0, 2])) / np.float32(2)
    assert tuple(plots.output_to_target([]).shape) == (0, 7)


def test_ir_file_name():
    assert plots.ir_name("runs/val/test_batch0_pred.jpg") == Path("runs/val/test_batch0_pred_ir.jpg")
    assert plots.ir_name(Path("images.png")) == Path("images_ir.png")
    assert plots.ir_name("a.b/mosaic") == Path("a.b/mosaic_ir")
    assert plots.mosaic_file_names("x.jpg", 1) == [Path("x.jpg")] and plots.mosaic_file_names("x.jpg", 2) == [Path("x.jpg"), Path("x_ir.jpg")]


# ------------------------------------------------------------------------------------------------ the restatement, looked at directly
def test_restatement_compose_places_cells_column_major():
    imgs = np.zeros((5, 3, 2, 3), np.uint8)
    for i in range(5):
        imgs[i] = 10 * (i + 1)
    m = mosaic_ref.compose_ref(imgs)
    assert m.shape == (6, 9, 3)
    assert [int(m[y, x, 0]) for (y, x) in ((0, 0), (2, 0), (4, 0), (0, 3), (2, 3))] == [10, 20, 30, 40, 50]       # down the first column, then the second
    assert (m[4:, 3:] == 255).all() and (m[:, 6:] == 255).all()
    unit = np.full((1, 3, 2, 2), 0.5, np.float32)
    assert (mosaic_ref.compose_ref(unit) == 127).all()                      # <= 1: x 255, truncated
    unit[0, 0, 0, 0] = 1.5
    assert sorted(set(mosaic_ref.compose_ref(unit).ravel().tolist())) == [0, 1]


def test_restatement_resize_is_a_convex_blend():
    g = np.random.default_rng(0)
    img = g.uniform(0, 255, (50, 70, 3)).astype(np.float32)
    out = mosaic_ref.resize_float(img, 64, 46)
    assert out.shape == (46, 64, 3) and out.min() >= img.min() - 1e-3 and out.max() <= img.max() + 1e-3
    flat = np.full((75, 100, 3), 77, np.float32)
    assert np.abs(mosaic_ref.resize_float(flat, 64, 48) - 77).max() < 1e-4
    s0, s1, a0, a1 = mosaic_ref.float_taps(64, 100)
    assert s0[0] == 0 and s1[-1] == 99 and np.all(a0 == np.float32(1) - a1) and a1[0] == np.float32(0.28125)          # 0.5 * 1.5625 - 0.5


def test_restatement_slots_rules():
    sf = 0.5
    rows = np.array([[0, 1, 0.5, 0.5, 0.2, 0.2],          # image 0: normalised (max 0.6)
                     [1, 2, 50, 40, 20, 10],              # image 1: pixels, scaled by sf
                     [0, 0, 0.25, 0.25, 0.5, 0.5],
                     [5, 0, 0.5, 0.5, 0.1, 0.1],          # image index >= bs: ignored
                     [1, 9, 10, 10, 4, 4]], np.float32)   # class outside nc = 3
    slots, flag = mosaic_ref.slots_ref(rows, 2, 4, 3, 100, 200, sf)
    assert flag == mosaic_ref.BAD_CLASS
    assert slots[0, 0, :7].tolist() == [0, 0, 100, 50, 0, 0, 1]           # the later target sits in the lower slot
    assert slots[0, 1, :7].tolist() == [int(np.float32(0.4) * 200), 40, 120, 60, 1, 0, 1]
    assert slots[1, 0, :7].tolist() == [20, 17, 30, 22, 2, 0, 1] and slots[1, 1, 6] == 0
    conf = np.array([[0, 0, 10, 10, 4, 4, 0.25], [0, 1, 10, 10, 4, 4, np.nextafter(np.float32(0.25), np.float32(1))], [0, 2, 10, 10, 4, 4, 0.96]], np.float32)
    slots, flag = mosaic_ref.slots_ref(conf, 1, 1, 3, 100, 200, 2.0)
    assert flag == mosaic_ref.OVERFLOW and slots[0, 0, :7].tolist() == [8, 8, 12, 12, 2, 10, 1]


def test_restatement_borders():
    m = [np.zeros((8, 12, 3), np.uint8)]
    mosaic_ref.finish_ref(m, 1, 2, 4, 6, None, None)        # one occupied cell of 4 x 6 at the origin in a 2 x 2 grid
    want = np.zeros((8, 12), bool)
    want[0:6, 0:8] = True                                    # [bx - 1, bx + w + 1] x [by - 1, by + h + 1], clipped
    want[2:3, 2:5] = False                                   # inside [bx + 2, bx + w - 2] x [by + 2, by + h - 2]
    assert np.array_equal(m[0][..., 0] == 255, want) and np.array_equal(m[0][..., 0], m[0][..., 2])
