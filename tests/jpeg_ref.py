"""numpy restatement of the pixel half of the JPEG decoder (the definition in include/cft_hip.h), written plane by plane from the
quantised coefficients to RGB - whole-plane array operations, where the kernels of csrc/jpeg.hip work per block and per pixel - and the
generator of the test files.  TEST INFRASTRUCTURE ONLY."""
import io
import os
import sys

import numpy as np

from jpeg_enc_ref import content  # noqa: F401  (the encoder's generator of [h, w, 3] uint8 test images; CONTENTS below are three of its kinds)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(1, 1), (2, 2), (8, 8), (16, 16), (17, 13), (5, 7), (6, 5), (3, 8), (4, 9), (33, 47), (64, 64)]      # (h, w)
CONTENTS = ("gradient", "noise", "mixed")
LAYOUTS = ("444", "422", "420", "gray")
OPTIONS = ({}, {"restart_marker_blocks": 1}, {"optimize": True})
QUALITIES = (30, 75, 95, 100)


def encode(arr, layout, quality, **options):
    """The bytes of ``arr`` ([h, w, 3] uint8) as a JPEG written by PIL's encoder."""
    from PIL import Image
    buf = io.BytesIO()
    if layout == "gray":
        Image.fromarray(arr).convert("L").save(buf, format="JPEG", quality=quality, **options)
    else:
        Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[layout], **options)
    return buf.getvalue()


def pil_decode(blob):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.array(im.convert("RGB"))


_MATRIX = None


def matrix():
    """The test matrix, built once and shared: a list of (name, bytes, PIL's decode [h, w, 3] uint8)."""
    global _MATRIX
    if _MATRIX is None:
        cases = []
        for si, (h, w) in enumerate(SIZES):
            for ci, kind in enumerate(CONTENTS):
                arr = content(kind, h, w, 1000 * si + ci)
                for layout in LAYOUTS:
                    for oi, opt in enumerate(OPTIONS):
                        for q in QUALITIES:
                            blob = encode(arr, layout, q, **opt)
                            cases.append((f"{h}x{w}-{kind}-{layout}-opt{oi}-q{q}", blob, pil_decode(blob)))
        _MATRIX = cases
    return _MATRIX


def entropy(blob):
    """(info, coef int16 [ncoef], qtab uint16 [3, 64]) of a supported file through the library's host half; None when unsupported."""
    from msod_amd.utils import jpeg as J
    info = J.jpeg_info(blob)
    if info is None:
        return None
    coef = np.empty(int(info["ncoef"]), dtype=np.int16)
    qtab = np.empty(192, dtype=np.uint16)
    if not J.jpeg_entropy(blob, info, coef, qtab):
        return None
    return info, coef, qtab.reshape(3, 64)


def _idct_1d(v, shift):
    """jpeg_idct_islow's butterfly on the eight int32 arrays v[0..7], descaled by ``shift``."""
    i32 = np.int32
    z1 = (v[2] + v[6]) * i32(4433)
    e2 = z1 + v[6] * i32(-15137)
    e3 = z1 + v[2] * i32(6270)
    e0 = (v[0] + v[4]) << 13
    e1 = (v[0] - v[4]) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * i32(9633)
    t0, t1, t2, t3 = t0 * i32(2446), t1 * i32(16819), t2 * i32(25172), t3 * i32(12299)
    z1, z2, z3, z4 = z1 * i32(-7373), z2 * i32(-20995), z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = i32(1 << (shift - 1))
    return [(a + r) >> shift for a in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)]


def planes(info, coef, qtab):
    """The component planes after dequantisation and IDCT: uint8 [8 bh, 8 bw] each, padding samples included."""
    out, base = [], 0
    for c in range(int(info["ncomp"])):
        bh, bw = int(info["bh"][c]), int(info["bw"][c])
        n = 64 * bh * bw
        blocks = coef[base:base + n].reshape(bh, bw, 8, 8).astype(np.int32) * qtab[c].reshape(8, 8).astype(np.int32)
        base += n
        with np.errstate(over="ignore"):
            cols = np.stack(_idct_1d([blocks[:, :, k, :] for k in range(8)], 11), axis=2)          # pass 1 runs down the columns
            rows = np.stack(_idct_1d([cols[:, :, :, k] for k in range(8)], 18), axis=3)            # pass 2 along the rows
        out.append(np.clip(rows + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw))
    return out


def _shift(a, axis, step):
    """``a`` moved by one along ``axis`` with the edge sample repeated: element i becomes a[i - step]."""
    idx = np.clip(np.arange(a.shape[axis]) - step, 0, a.shape[axis] - 1)
    return np.take(a, idx, axis=axis)


def upsample(plane, info, c):
    """Component ``c`` at full size [height, width] int32: fancy (triangle) upsampling over the downsampled size only."""
    H, W = int(info["height"]), int(info["width"])
    ch, cw = int(info["ch"][c]), int(info["cw"][c])
    a = plane[:ch, :cw].astype(np.int32)
    hr, vr = int(info["hmax"]) // int(info["hs"][c]), int(info["vmax"]) // int(info["vs"][c])
    if hr == 1 and vr == 1:
        return a[:H, :W]
    if vr == 1:
        even, odd = (3 * a + _shift(a, 1, 1) + 1) >> 2, (3 * a + _shift(a, 1, -1) + 2) >> 2
    else:
        s = np.empty((2 * ch, cw), dtype=np.int32)
        s[0::2] = 3 * a + _shift(a, 0, 1)             # even output rows lean on the row above
        s[1::2] = 3 * a + _shift(a, 0, -1)            # odd ones on the row below
        even, odd = (3 * s + _shift(s, 1, 1) + 8) >> 4, (3 * s + _shift(s, 1, -1) + 7) >> 4
    out = np.empty((even.shape[0], 2 * cw), dtype=np.int32)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out[:H, :W]


def to_rgb(info, comp_planes):
    H, W = int(info["height"]), int(info["width"])
    if int(info["ncomp"]) == 1:
        return np.repeat(comp_planes[0][:H, :W, None], 3, axis=2)
    y, cb, cr = (upsample(p, info, c) for c, p in enumerate(comp_planes))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(blob):
    """[h, w, 3] uint8 by the library's entropy decoder and this file's pixel half; None when the file is unsupported."""
    e = entropy(blob)
    if e is None:
        return None
    info, coef, qtab = e
    return to_rgb(info, planes(info, coef, qtab))
