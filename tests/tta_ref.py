"""Restatement of cft_tta_view and cft_tta_merge (include/cft_hip.h) as whole-array numpy: the other algorithm - index and weight
vectors per axis and fancy indexing instead of a thread per pixel group, slices instead of a thread per element.  Every float32
array operation of numpy rounds once, like the kernels' contract(off) arithmetic, so the two agree bit for bit."""
import math

import numpy as np

F = np.float32
PAD = F(0.447)


def normalised(img):
    """[B, 3, H, W] uint8 / float16 / float32 array -> float32, uint8 divided by 255 (IEEE division)."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(F) / F(255)
    return img.astype(F)


def sizes(H, W, ratio, gs):
    """((hs, ws), (Ho, Wo)): the scaled and the padded size, in Python's doubles."""
    return (int(H * ratio), int(W * ratio)), tuple(math.ceil(x * ratio / gs) * gs for x in (H, W))


def taps(out, inn):
    """Per output index of one axis: (i0, i1, w0, w1) of torch's align_corners=False bilinear resize in float32."""
    scale = F(inn) / F(out)
    src = scale * (np.arange(out, dtype=F) + F(0.5)) - F(0.5)
    src = np.maximum(src, F(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), inn - 1)
    lam = np.clip(src - i0.astype(F), F(0), F(1))
    return i0, np.minimum(i0 + 1, inn - 1), F(1) - lam, lam


def view(img, ratio, gs, flip=False):
    x = normalised(img)
    if flip:
        x = x[..., ::-1]
    B, C, H, W = x.shape
    (hs, ws), (Ho, Wo) = sizes(H, W, ratio, gs)
    y0, y1, wy0, wy1 = taps(hs, H)
    x0, x1, wx0, wx1 = taps(ws, W)
    top, bot = x[:, :, y0], x[:, :, y1]
    h0 = top[..., x0] * wx0 + top[..., x1] * wx1
    h1 = bot[..., x0] * wx0 + bot[..., x1] * wx1
    out = np.full((B, C, Ho, Wo), PAD, dtype=F)
    out[:, :, :hs, :ws] = h0 * wy0[:, None] + h1 * wy1[:, None]
    return out


def merge(preds, scales, flips, img_w):
    parts = []
    for p, s, f in zip(preds, scales, flips):
        y = np.array(p, dtype=F, copy=True)
        y[..., :4] = y[..., :4] / F(s)
        if f:
            y[..., 0] = F(img_w) - y[..., 0]
        parts.append(y)
    return np.concatenate(parts, 1)
