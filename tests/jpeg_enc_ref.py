"""numpy restatement of the pixel half of the JPEG encoder (the definition in include/cft_hip.h): from an image to the quantised
coefficients in the layout cft_jpeg_entropy writes - whole-plane array operations (pad the planes, filter them, cut them into blocks,
transform all blocks at once in int64), where the kernel of csrc/jpeg_encode.hip gathers per block row with clamped indices in
int32 - and the generator of the test matrix with PIL's file for every case.  TEST INFRASTRUCTURE ONLY."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (40, 24), (36, 20), (9, 50), (41, 3), (64, 48)]      # (width, height)
CONTENTS = ("noise", "gradient", "mixed", "primaries")
LAYOUTS = ("gray", "444", "422", "420")
QUALITIES = (1, 30, 75, 95, 100)
SAMPLING = {"gray": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}                       # ncomp, hmax, vmax
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def content(kind, h, w, seed):
    """An [h, w, 3] uint8 test image; "primaries" holds only 0 and 255 in 3 x 2 patches of saturated colours."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], -1).astype(np.uint8)
    noise = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "gradient":
        return grad
    if kind == "noise":
        return noise
    if kind == "primaries":
        cells = rng.randint(0, 2, (h // 2 + 1, w // 3 + 1, 3)).astype(np.uint8) * 255
        return np.ascontiguousarray(cells[yy // 2, xx // 3])
    return np.where(((xx // 4 + yy // 4) % 2 == 0)[..., None], grad, noise).astype(np.uint8)


def source(arr, layout):
    """What the encoder is given for a layout: the RGB array, or its grey version [h, w]."""
    from PIL import Image
    return np.array(Image.fromarray(arr).convert("L")) if layout == "gray" else arr


def pil_file(src, layout, quality):
    """The yardstick: PIL's file of ``src`` ([h, w, 3] or [h, w] uint8), optimize off."""
    from PIL import Image
    buf = io.BytesIO()
    if layout == "gray":
        Image.fromarray(src).save(buf, "JPEG", quality=quality)
    else:
        Image.fromarray(src).save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[layout])
    return buf.getvalue()


_MATRIX = None


def matrix():
    """The test matrix, built once and shared and never modified: a list of (name, source array, layout, quality, PIL's bytes)."""
    global _MATRIX
    if _MATRIX is None:
        cases = []
        for si, (w, h) in enumerate(SIZES):
            for ci, kind in enumerate(CONTENTS):
                arr = content(kind, h, w, 2000 * si + ci)
                for layout in LAYOUTS:
                    src = source(arr, layout)
                    src.setflags(write=False)
                    for q in QUALITIES:
                        cases.append((f"{w}x{h}-{kind}-{layout}-q{q}", src, layout, q, pil_file(src, layout, q)))
        _MATRIX = cases
    return _MATRIX


def real_block_mask(info):
    """bool [blocks]: which blocks of the coefficient layout lie inside their component's real grid."""
    parts = []
    for c in range(int(info["ncomp"])):
        bh, bw = int(info["bh"][c]), int(info["bw"][c])
        m = np.zeros((bh, bw), dtype=bool)
        m[:-(-int(info["ch"][c]) // 8), :-(-int(info["cw"][c]) // 8)] = True
        parts.append(m.reshape(-1))
    return np.concatenate(parts)


# ---- tables (ITU T.81 Annex K.1 / K.2, natural order)
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def quality_tables(quality):
    """uint16 [3, 64]: luminance, chrominance, chrominance."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    rows = [np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA, BASE_CHROMA)]
    return np.stack(rows).astype(np.uint16)


# ---- pixels to coefficients
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(a, first):
    """jpeg_fdct_islow's butterfly on the eight int64 arrays a[0..7]; ``first``: the row pass, which scales up by PASS1_BITS."""
    t0, t7, t1, t6 = a[0] + a[7], a[0] - a[7], a[1] + a[6], a[1] - a[6]
    t2, t5, t3, t4 = a[2] + a[5], a[2] - a[5], a[3] + a[4], a[3] - a[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4], n = (t10 + t11) << 2, (t10 - t11) << 2, 11
    else:
        o[0], o[4], n = _descale(t10 + t11, 2), _descale(t10 - t11, 2), 15
    z1 = (t12 + t13) * 4433
    o[2], o[6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return o


def _edge(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def component_planes(src, ncomp, hmax, vmax):
    """The int64 sample planes [8 bh, 8 bw] of every component, edge rules applied."""
    H, W = src.shape[:2]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    if ncomp == 1:
        return [_edge(src.astype(np.int64), 8 * my, 8 * mx)]
    R, G, B = (src[..., k].astype(np.int64) for k in range(3))
    full = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
            (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
            (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16]
    out = [_edge(full[0], 8 * my * vmax, 8 * mx * hmax)]
    for p in full[1:]:
        p = _edge(p, -(-H // vmax) * vmax, 8 * mx * hmax)          # every column of the MCU grid, rows only up to a multiple of vmax
        if hmax == 2 and vmax == 2:
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)[None, :]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif hmax == 2:
            bias = (np.arange(p.shape[1] // 2) & 1)[None, :]
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        out.append(_edge(p, 8 * my, 8 * mx))                        # the rest of the rows repeat the last downsampled row
    return out


def coefficients(src, quality, layout):
    """int16 [ncoef]: component after component, blocks in raster order of the padded grid, natural order; dummy blocks zero."""
    ncomp, hmax, vmax = SAMPLING[layout]
    H, W = src.shape[:2]
    qtab = quality_tables(quality).astype(np.int64)
    out = []
    for c, p in enumerate(component_planes(src, ncomp, hmax, vmax)):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = (p - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)                            # [bh, bw, row, column]
        rows = np.stack(_fdct_1d([blocks[..., k] for k in range(8)], True), axis=-1)              # along each row
        cols = np.stack(_fdct_1d([rows[:, :, k, :] for k in range(8)], False), axis=2)            # down each column
        d = qtab[c].reshape(8, 8) << 3
        q = np.sign(cols) * ((np.abs(cols) + (d >> 1)) // d)
        fh, fv = (1, 1) if c == 0 else (hmax, vmax)
        real_bw, real_bh = -(-(-(-W // fh)) // 8), -(-(-(-H // fv)) // 8)
        q[real_bh:] = 0
        q[:, real_bw:] = 0
        out.append(q.reshape(-1))
    return np.concatenate(out).astype(np.int16)
