"""Numpy restatement of the raster of cft_augment_batch_u8 (include/cft_hip.h).  TEST INFRASTRUCTURE ONLY.

Written as the other algorithm: where the kernel gathers every output pixel through flips, inverse affine, tile lookup and on-the-fly
resize, this builds the resized pairs and the canvases, warps whole images, converts whole images and flips at the end.  The cv2
calls of the reference's augmented ``__getitem__`` (``warpAffine``, ``cvtColor``, ``getRotationMatrix2D``, ``split``, ``merge``,
``LUT``) are restated here from OpenCV's published 8-bit paths; cv2 itself is absent, so "parity with cv2 unpinned".  INTER_LINEAR is
``oracle.letterbox_oracle.resize``.  tests/golden/make_augment_golden.py binds the reference's cv2 names to these functions."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import letterbox_oracle as LO  # noqa: E402

COLOR_BGR2HSV, COLOR_HSV2BGR = 40, 54
BORDER = 114
FLIPLR, FLIPUD = 1, 2

_i = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate(([0], np.rint((255 << 12) / _i))).astype(np.int64)
HDIV = np.concatenate(([0], np.rint((180 << 12) / (6.0 * _i)))).astype(np.int64)


def getRotationMatrix2D(center=(0, 0), angle=0.0, scale=1.0):
    """cv2's closed form: angle in degrees, positive = counter-clockwise."""
    a = angle * np.pi / 180
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def invert_affine(M):
    """The inverse of a 2x3 affine in double by warpAffine's closed form: (a00, a01, a02, a10, a11, a12)."""
    m00, m01, m02, m10, m11, m12 = (float(v) for v in np.asarray(M, dtype=np.float64)[:2].reshape(-1))
    D = m00 * m11 - m01 * m10
    D = 1.0 / D if D != 0 else 0.0
    a00, a11 = m11 * D, m00 * D
    a01, a10 = m01 * -D, m10 * -D
    a02 = -a00 * m02 - a01 * m12
    a12 = -a10 * m02 - a11 * m12
    return a00, a01, a02, a10, a11, a12


def warp_coords(inv, H, W):
    """(sy, sx, fy, fx) int64 [H, W]: integer part and 1/32 fraction of the canvas coordinate of every output pixel."""
    a00, a01, a02, a10, a11, a12 = inv
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    X = (np.rint(a00 * x * 1024.0).astype(np.int64) + np.rint((a01 * y + a02) * 1024.0).astype(np.int64) + 16) >> 5
    Y = (np.rint(a10 * x * 1024.0).astype(np.int64) + np.rint((a11 * y + a12) * 1024.0).astype(np.int64) + 16) >> 5
    return Y >> 5, X >> 5, Y & 31, X & 31


def _bilinear(img, sy, sx, fy, fx, border):
    """The four-tap blend with weights in 1/1024; a tap outside the image is ``border``, each tap tested on its own."""
    h, w, c = img.shape
    src = img.astype(np.int64)
    border = np.broadcast_to(np.asarray(border, dtype=np.int64).reshape(-1)[:c], (c,))

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(inside[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], border[None, None, :])

    acc = (tap(sy, sx) * ((32 - fx) * (32 - fy))[..., None] + tap(sy, sx + 1) * (fx * (32 - fy))[..., None]
           + tap(sy + 1, sx) * ((32 - fx) * fy)[..., None] + tap(sy + 1, sx + 1) * (fx * fy)[..., None])
    return ((acc + 512) >> 10).astype(np.uint8)


def warpAffine(img, M, dsize, borderValue=(BORDER, BORDER, BORDER)):
    """cv2.warpAffine for uint8 HWC images, INTER_LINEAR, BORDER_CONSTANT.  dsize = (width, height)."""
    assert img.dtype == np.uint8 and img.ndim == 3
    W, H = dsize
    return _bilinear(img, *warp_coords(invert_affine(M), H, W), borderValue)


def rgb_to_hsv8(r, g, b):
    """8-bit HSV (H in 0..179) of integer planes r, g, b."""
    r, g, b = (np.asarray(p).astype(np.int64) for p in (r, g, b))
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * SDIV[v] + 2048) >> 12
    hh = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (hh * HDIV[diff] + 2048) >> 12
    h = h + np.where(h < 0, 180, 0)
    return h, s, v


def hsv8_to_rgb(h, s, v):
    """The six-sector formula in float32, one rounding per operation; returns integer planes r, g, b."""
    f32 = np.float32
    sf, vf, hf = np.asarray(s).astype(f32) / f32(255), np.asarray(v).astype(f32) / f32(255), np.asarray(h).astype(f32) / f32(30)
    kf = np.floor(hf)
    f = hf - kf
    k = kf.astype(np.int64) % 6
    one = f32(1)
    t = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))])
    assert t.dtype == np.float32
    sector = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # (b, g, r) per sector
    pick = lambda c: np.take_along_axis(t, sector[k, c][None], 0)[0]  # noqa: E731
    out = [np.clip(np.rint(f32(255) * pick(c)), 0, 255).astype(np.int64) for c in (2, 1, 0)]
    return out[0], out[1], out[2]


def cvtColor(img, code, dst=None):
    assert img.dtype == np.uint8
    if code == COLOR_BGR2HSV:
        out = np.stack(rgb_to_hsv8(img[..., 2], img[..., 1], img[..., 0]), -1).astype(np.uint8)
    elif code == COLOR_HSV2BGR:
        r, g, b = hsv8_to_rgb(img[..., 0], img[..., 1], img[..., 2])
        out = np.stack((b, g, r), -1).astype(np.uint8)
    else:
        raise ValueError(f"cvtColor: code {code} is not restated")
    if dst is not None:
        dst[...] = out
        return dst
    return out


def split(img):
    return tuple(np.ascontiguousarray(img[..., c]) for c in range(img.shape[2]))


def merge(planes):
    return np.stack(planes, -1)


def LUT(plane, lut):
    return np.asarray(lut)[plane]


def hsv_luts(r):
    """The three look-up tables of augment_hsv for gains ``r`` (already ``uniform * [h, s, v] + 1``): uint8 [3, 256]."""
    x = np.arange(0, 256, dtype=np.int16)
    return np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)])


def apply_hsv_rgb(img, luts):
    """augment_hsv on an HWC image in RGB order with the three tables ``luts`` [3, 256]."""
    h, s, v = rgb_to_hsv8(img[..., 0], img[..., 1], img[..., 2])
    r, g, b = hsv8_to_rgb(luts[0][h], luts[1][s], luts[2][v])
    return np.stack((r, g, b), -1).astype(np.uint8)


def render_row(row, luts, H, W):
    """One output image [6, H, W] from a row in python form: dict(ntiles, warp, canvas_h, canvas_w, flip, inv, tiles) with every tile
    a dict(rgb, ir (HWC uint8 arrays in RGB order), h, w, x1, y1, x2, y2, padw, padh); ``luts`` uint8 [2, 3, 256]."""
    planes = []
    for s, key in enumerate(("rgb", "ir")):
        canvas = np.full((row["canvas_h"], row["canvas_w"], 3), BORDER, dtype=np.uint8)
        for t in row["tiles"][:row["ntiles"]]:
            src = np.ascontiguousarray(t[key])
            small = src if src.shape[:2] == (t["h"], t["w"]) else LO.resize(src, (t["w"], t["h"]))
            canvas[t["y1"]:t["y2"], t["x1"]:t["x2"]] = small[t["y1"] - t["padh"]:t["y2"] - t["padh"], t["x1"] - t["padw"]:t["x2"] - t["padw"]]
        if row["warp"]:
            img = _bilinear(canvas, *warp_coords(row["inv"], H, W), BORDER)
        else:
            assert canvas.shape[:2] == (H, W)
            img = canvas
        img = apply_hsv_rgb(img, luts[s])
        if row["flip"] & FLIPUD:
            img = np.flipud(img)
        if row["flip"] & FLIPLR:
            img = np.fliplr(img)
        planes.append(np.ascontiguousarray(img.transpose(2, 0, 1)))
    return np.concatenate(planes, 0)


# ---- the recording tests/golden/augment/augment_cases.pt and this package's side of it ----
def load_cases():
    """``(fixture root, cases)`` of the recording; every item's image is inflated to a uint8 [6, H, W] tensor under ``"img"``."""
    import zlib
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    rec = torch.load(os.path.join(here, "golden", "augment", "augment_cases.pt"), weights_only=False)
    for c in rec["cases"]:
        for p in c["passes"]:
            for it in p["items"]:
                it["img"] = torch.frombuffer(bytearray(zlib.decompress(it["zlib"])), dtype=torch.uint8).reshape(it["shape"])
    return os.path.join(here, "golden", "dataset"), rec["cases"]


def make_dataset(root, c, **kw):
    """This package's augmented dataset for one recorded case."""
    from msod_amd.utils.datasets import LoadMultiModalImagesAndLabelsAugmented
    return LoadMultiModalImagesAndLabelsAugmented(os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), c["img_size"], c["batch_size"],
                                                  hyp=c["hyp"], rect=c["rect"], stride=c["stride"], **kw)


def generators(seed):
    """The generators in the state ``random.seed(seed); np.random.seed(seed)`` leaves the global ones in."""
    import random
    return random.Random(seed), np.random.RandomState(seed)


def rows_from_table(table, luts, plans, sources):
    """The rows of a built table in the python form ``render_row`` takes; ``sources``: {pair index: (rgb, ir) HWC RGB uint8 arrays}."""
    rows = []
    for row, p in zip(table, plans):
        tiles = []
        for tile, t in zip(row["tile"][:int(row["ntiles"])], p["tiles"]):
            d = {k: int(tile[k]) for k in ("h", "w", "x1", "y1", "x2", "y2", "padw", "padh")}
            d["rgb"], d["ir"] = sources[t["index"]]
            tiles.append(d)
        rows.append({"ntiles": int(row["ntiles"]), "warp": int(row["warp"]), "canvas_h": int(row["canvas_h"]), "canvas_w": int(row["canvas_w"]),
                     "flip": int(row["flip"]), "inv": tuple(float(v) for v in row["inv"]), "tiles": tiles})
    return rows


def render_plans(ds, plans):
    """uint8 [B, 6, H, W]: what cft_augment_batch_u8 must write for ``plans``, through this file alone."""
    from msod_amd.utils.datasets import build_augment_descriptors
    table, luts, (H, W) = build_augment_descriptors(plans)
    sources = {k: ds.load_pair(k) for k in sorted({t["index"] for p in plans for t in p["tiles"]})}
    return np.stack([render_row(r, l, H, W) for r, l in zip(rows_from_table(table, luts, plans, sources), luts)])
