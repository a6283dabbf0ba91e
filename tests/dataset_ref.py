"""float64 numpy restatement of cv2.resize(INTER_AREA) for 8-bit images, the arithmetic that ``cft_pair_batch_u8`` is tested
against (csrc/dataset.hip).  TEST INFRASTRUCTURE ONLY.

The reference's ``load_image_rgb_ir`` (utils/datasets.py:1361-1367) shrinks with ``cv2.resize(..., interpolation=cv2.INTER_AREA)``.
cv2 is absent here and unpinned by the reference, so, as oracle/letterbox_oracle.py does for INTER_LINEAR, OpenCV's published
algorithm (modules/imgproc/src/resize.cpp) is restated:

* ``computeResizeAreaTab``: output cell ``d`` covers ``[d * scale, (d + 1) * scale)`` of the source with ``scale = ssize / dsize``
  from the integer sizes; whole source cells weigh ``1 / cellWidth``, the first and the last weigh their covered fraction, and a
  covered fraction of at most 1e-3 is dropped;
* ``ResizeArea_``: the weighted columns of a source row, then the weighted rows; the result is rounded to nearest
  (``saturate_cast<uchar>``);
* ``ResizeAreaFast_`` when both scales are integers: the block sum over ``scale_y x scale_x`` pixels divided by the block size,
  halves rounded up (the 2x2 fast path's ``(a + b + c + d + 2) >> 2``, applied to every integer scale).

"Parity unpinned": this is the definition of the result here, not a measurement of any cv2 build."""
import numpy as np

INTER_AREA = 3
TIE_BAND = 2.0 ** -10


def area_tab(ssize, dsize):
    """``[dsize, ssize]`` float64 weights of one axis (computeResizeAreaTab)."""
    scale = float(ssize) / float(dsize)
    tab = np.zeros((dsize, ssize), dtype=np.float64)
    for d in range(dsize):
        fsx1 = d * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            tab[d, sx1 - 1] = (sx1 - fsx1) / cell
        for sx in range(sx1, sx2):
            tab[d, sx] = 1.0 / cell
        if fsx2 - sx2 > 1e-3:
            tab[d, sx2] = min(min(fsx2 - sx2, 1.0), cell) / cell
    return tab


def is_integer_scale(src_hw, dst_hw):
    return src_hw[0] % dst_hw[0] == 0 and src_hw[1] % dst_hw[1] == 0


def resize_area_real(img, dsize):
    """The value before rounding, float64 ``[h, w, c]``; dsize = (width, height).  Integer scales: the exact block mean."""
    assert img.dtype == np.uint8 and img.ndim == 3
    h0, w0 = img.shape[:2]
    w, h = dsize
    assert 0 < w <= w0 and 0 < h <= h0
    src = img.astype(np.float64)
    if is_integer_scale((h0, w0), (h, w)):
        iy, ix = h0 // h, w0 // w
        return src.reshape(h, iy, w, ix, -1).sum(axis=(1, 3)) / (iy * ix)
    ty, tx = area_tab(h0, h), area_tab(w0, w)
    rows = np.einsum("dx,yxc->ydc", tx, src)          # columns of every source row
    return np.einsum("ey,ydc->edc", ty, rows)         # then the rows


def resize_area(img, dsize, interpolation=INTER_AREA):
    """cv2.resize(img, dsize, interpolation=cv2.INTER_AREA) for uint8 HWC images."""
    assert interpolation == INTER_AREA
    v = resize_area_real(img, dsize)
    if is_integer_scale(img.shape[:2], (dsize[1], dsize[0])):
        out = np.floor(v + 0.5)                       # halves up; v is a multiple of 1 / (iy * ix), exact in float64 at these sizes
    else:
        out = np.rint(v)
    return np.clip(out, 0, 255).astype(np.uint8)


def near_tie(img, dsize):
    """bool ``[h, w, c]``: pixels whose real value lies within 2^-10 of a .5 tie - the only ones where an fp32 accumulation may
    round the other way.  All False for integer scales (that path is exact)."""
    v = resize_area_real(img, dsize)
    if is_integer_scale(img.shape[:2], (dsize[1], dsize[0])):
        return np.zeros(v.shape, dtype=bool)
    return np.abs(v - np.floor(v) - 0.5) < TIE_BAND


def box_filter_supersampled(img, dsize, ss=16):
    """Brute force: every source pixel split into ss x ss samples, every output pixel the plain mean of the samples whose centres
    fall into its box.  float64 ``[h, w, c]``, for cross-checking ``resize_area_real``."""
    h0, w0 = img.shape[:2]
    w, h = dsize
    big = np.repeat(np.repeat(img.astype(np.float64), ss, axis=0), ss, axis=1)
    ys = ((np.arange(h0 * ss) + 0.5) / ss * h / h0).astype(np.int64).clip(0, h - 1)
    xs = ((np.arange(w0 * ss) + 0.5) / ss * w / w0).astype(np.int64).clip(0, w - 1)
    out = np.zeros((h, w, img.shape[2]))
    cnt = np.zeros((h, w, 1))
    np.add.at(out, (ys[:, None], xs[None, :]), big)
    np.add.at(cnt, (ys[:, None], xs[None, :]), 1.0)
    return out / cnt


# ------------------------------------------------------------------------------ the recording (tests/golden/make_dataset_golden.py)
def load_cases():
    """``(fixture root, cases, blocks)``: blocks are the distinct recorded uint8 [6, H, W] pair blocks, inflated."""
    import os
    import zlib
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset")
    rec = torch.load(os.path.join(root, "dataset_cases.pt"), weights_only=False)
    blocks = [torch.frombuffer(bytearray(zlib.decompress(b["zlib"])), dtype=torch.uint8).reshape(b["shape"]) for b in rec["blocks"]]
    return root, rec["cases"], blocks


def case_id(c):
    return f"s{c['img_size']}-{'rect' if c['rect'] else 'square'}-pad{c['pad']}-bs{c['batch_size']}" + ("-single" if c["single_cls"] else "")


def make_dataset(root, c, **kw):
    """This package's dataset for one recorded case."""
    import os
    from msod_amd.utils.datasets import LoadMultiModalImagesAndLabels
    return LoadMultiModalImagesAndLabels(os.path.join(root, "rgb", "images"), os.path.join(root, "ir", "images"), c["img_size"], c["batch_size"],
                                         rect=c["rect"], pad=c["pad"], stride=c["stride"], single_cls=c["single_cls"], **kw)


def plain(x):
    """Nested tuples of numpy / python scalars -> python floats and ints, as the recording holds ``shapes``."""
    if isinstance(x, (tuple, list)):
        return tuple(plain(v) for v in x)
    return x.item() if isinstance(x, np.generic) else x
