"""Host restatement of the batch mosaics (csrc/mosaic.hip, utils/plots.py ``plot_images``), numpy on the CPU.  TEST INFRASTRUCTURE ONLY.

Written from the rules stated at ``cft_mosaic_*`` in include/cft_hip.h, which follow the reference's utils/plots.py:128-203 line by
line (the line numbers below are the reference's); cv2 is absent, so its float resize is restated from OpenCV's published coordinate
convention and its lines and font are this project's raster (``detect_ref.render_ref``).

* ``geometry``          :142-152 and :199-200 in Python doubles;
* ``compose_ref``       :137-138, :152-164: x 255 when image 0 is <= 1, float32 bilinear resize, clamp, truncate, column-major cells;
* ``tenths``            the digits of '%.1f' in integers on the double's bits;
* ``output_to_target``  :119-125, the float64 array the reference builds from float32 boxes;
* ``slots_ref``         :166-186 in the rows' dtype, one numpy operation per reference operation, reverse slot order;
* ``finish_ref``        file names and borders by ordered overdraw;
* ``plot_images_ref``   the whole function: compose, every cell's slots drawn by ``detect_ref.render_ref`` on a view of the cell (ordered
                        overdraw - the other algorithm from the kernel's per-pixel search), finish, ``area_ref``;
* ``area_ref``          ``dataset_ref.resize_area`` and ``near_tie`` for a whole mosaic, from one evaluation of the real value.
"""
import math
import struct
from pathlib import Path

import numpy as np

import dataset_ref
import detect_ref

BAD_CLASS, OVERFLOW = 1, 2
TEXT_COLOR = (225, 255, 255)          # :81
NAME_COLOR = (220, 220, 220)          # :192
PALETTE = [(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127),
           (188, 189, 34), (23, 190, 207)]      # matplotlib's Tableau colours, '#1f77b4' ... as RGB (:29-41)


def geometry(B, H, W, max_size=640, max_subplots=16):
    """``(bs, ns, sf, h, w, out_h, out_w)``."""
    bs = min(B, max_subplots)
    ns = int(np.ceil(bs ** 0.5))
    sf = max_size / max(H, W)
    h, w = H, W
    if sf < 1:
        h, w = math.ceil(sf * h), math.ceil(sf * w)
    r = min(1280. / max(h, w) / ns, 1.0)
    return bs, ns, sf, h, w, int(ns * h * r), int(ns * w * r)


def float_taps(dsize, ssize):
    """One axis of the float32 bilinear resize: indices s0, s1 (clamped) and weights a0, a1 (float32; the fraction is kept)."""
    scale = 1.0 / (dsize / ssize)
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    a1 = f - s
    a0 = np.float32(1) - a1
    s = s.astype(np.int64)
    assert a0.dtype == a1.dtype == np.float32
    return np.clip(s, 0, ssize - 1), np.clip(s + 1, 0, ssize - 1), a0, a1


def resize_float(img, w, h):
    """float32 HWC -> [h, w, C]: horizontal pass a0 * p0 + a1 * p1, then vertical, every operation one float32 rounding."""
    assert img.dtype == np.float32
    x0, x1, a0, a1 = float_taps(w, img.shape[1])
    y0, y1, b0, b1 = float_taps(h, img.shape[0])
    rows = a0[None, :, None] * img[:, x0] + a1[None, :, None] * img[:, x1]
    out = b0[:, None, None] * rows[y0] + b1[:, None, None] * rows[y1]
    assert out.dtype == np.float32
    return out


def to_u8(v):
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, 0, 255).astype(np.int64).astype(np.uint8)          # clamp, then truncation toward zero


def compose_ref(images, c0=0, max_size=640, max_subplots=16):
    """images: numpy [B, C, H, W] of any of the kernel's dtypes; channels [c0, c0 + 3) -> the HWC uint8 mosaic."""
    B, C, H, W = images.shape
    bs, ns, sf, h, w, _, _ = geometry(B, H, W, max_size, max_subplots)
    factor = np.float32(255 if np.max(images[0].astype(np.float32)) <= 1 else 1)          # a NaN maximum compares False
    mosaic = np.full((ns * h, ns * w, 3), 255, np.uint8)
    for i in range(bs):
        bx, by = w * (i // ns), h * (i % ns)
        img = images[i, c0:c0 + 3].astype(np.float32).transpose(1, 2, 0) * factor
        if sf < 1:
            img = resize_float(np.ascontiguousarray(img), w, h)
        mosaic[by:by + h, bx:bx + w] = to_u8(img)
    return mosaic


def tenths(x):
    """round(x * 10) of the double's exact value, ties to even, saturating at 0 and 10; NaN -> 0: the digits of '%.1f' % x."""
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    if u >> 63:
        return 0
    ex, frac = u >> 52, u & ((1 << 52) - 1)
    if ex == 2047:
        return 0 if frac else 10
    m = (frac | (1 << 52)) if ex else frac
    e = (ex if ex else 1) - 1075              # value = m * 2^e
    p = 10 * m
    if e >= 0:
        q = p << e
    else:
        q, rem = p >> -e, p & ((1 << -e) - 1)
        half = 1 << (-e - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
    return min(q, 10)


def output_to_target(dets, counts):
    """:119-125 on the padded NMS output: np.array of [i, cls, *xyxy2xywh(float32 box), conf] rows - a float64 array whose box values
    were computed in float32."""
    rows = []
    for i in range(len(counts)):
        for x1, y1, x2, y2, conf, cls in np.asarray(dets[i][:max(0, min(int(counts[i]), dets.shape[1]))], np.float32):
            rows.append([i, cls, (x1 + x2) / np.float32(2), (y1 + y2) / np.float32(2), x2 - x1, y2 - y1, conf])
    return np.array(rows, np.float64).reshape(-1, 7)


def _trunc(v):
    v = float(v)
    if v != v:
        return 0
    return int(max(-2.0 ** 30, min(2.0 ** 30, v)))


def slots_ref(targets, bs, cap, nc, h, w, sf):
    """targets: numpy float32 / float64 [nt, 6 or 7] -> (slots int32 [bs, cap, 16], flag), :166-186 in the array's dtype."""
    t = np.asarray(targets)
    assert t.dtype in (np.float32, np.float64)
    T = t.dtype.type
    slots, flag = np.zeros((bs, cap, 16), np.int32), 0
    if t.size == 0:
        return slots, flag
    labels = t.shape[1] == 6
    for i in range(bs):
        it = t[t[:, 0] == i]                                              # :166
        x, y, ww, hh = it[:, 2], it[:, 3], it[:, 4], it[:, 5]
        boxes = np.stack([x - ww / T(2), y - hh / T(2), x + ww / T(2), y + hh / T(2)])      # :167 xywh2xyxy, .T
        assert boxes.dtype == t.dtype
        if boxes.shape[1]:
            if boxes.max() <= T(1.01):                                    # :173
                boxes[[0, 2]] *= T(w)
                boxes[[1, 3]] *= T(h)
            elif sf < 1:                                                  # :176
                boxes *= T(sf)
        drawn = []
        for j, box in enumerate(boxes.T):
            c = float(it[j, 1])
            c = int(c) if (c == c and abs(c) < 2.0 ** 30) else -1         # :168 .astype('int')
            if not 0 <= c < nc:
                flag |= BAD_CLASS
                continue
            if labels or it[j, 6] > T(0.25):                              # :184
                drawn.append(([_trunc(v) for v in box], c, 0 if labels else tenths(it[j, 6])))      # :70 int(), '%.1f'
        D = len(drawn)
        if D > cap:
            flag |= OVERFLOW
        for k, (b, c, tn) in enumerate(drawn):
            s = D - 1 - k                                                 # the last drawn target ends on top: the lowest slot
            if s < cap:
                slots[i, s, :7] = b + [c, tn, 1]
    return slots, flag


def draw_cell(views, slots_i, names, has_conf, atlas):
    """One cell's slots into the views of that cell (one per stream), through ``detect_ref.render_ref``.  Every slot gets a class of
    its own whose name is the slot's whole label, so the ' d.d' suffix needs nothing of render_ref's ' d.dd'."""
    n = slots_i.shape[0]
    s = detect_ref.unpack_slots(slots_i[None].copy())
    texts, cols = [], []
    for r in range(n):
        c, tn = int(slots_i[r, 4]), int(slots_i[r, 5])
        name = names[c] if names else str(c)
        texts.append(f"{name} {tn // 10}.{tn % 10}" if has_conf else name)
        cols.append(PALETTE[c % 10])
        s["cls"][0, r] = r
    detect_ref.render_ref(views, s, 0, cols, TEXT_COLOR, 3, True, False, texts, atlas)


def finish_ref(mosaics, bs, ns, h, w, paths, atlas):
    """Ordered overdraw: every file name, then every border (the border wins)."""
    MH, MW = mosaics[0].shape[:2]
    gh, gw = atlas.shape[1:] if atlas is not None else (1, 1)
    for i in range(bs):
        bx, by = w * (i // ns), h * (i % ns)
        if paths:
            label = Path(paths[i]).name[:40]                              # :190
            for k, ch in enumerate(label):
                code = ord(ch)
                on = atlas[code - 32 if 32 <= code <= 127 else 0] >= 128
                ys, xs = np.nonzero(on)
                ys, xs = ys + by + 5, xs + bx + 5 + k * gw
                ok = (xs < bx + w) & (ys < by + h)                        # clipped to the cell
                for m in mosaics:
                    m[ys[ok], xs[ok]] = NAME_COLOR
    for i in range(bs):
        bx, by = w * (i // ns), h * (i % ns)
        for (X0, Y0, X1, Y1) in ((bx - 1, by - 1, bx + 1, by + h + 1), (bx + w - 1, by - 1, bx + w + 1, by + h + 1),
                                 (bx - 1, by - 1, bx + w + 1, by + 1), (bx - 1, by + h - 1, bx + w + 1, by + h + 1)):      # the four thick lines
            xa, xb, ya, yb = max(X0, 0), min(X1, MW - 1) + 1, max(Y0, 0), min(Y1, MH - 1) + 1
            for m in mosaics:
                m[ya:yb, xa:xb] = 255


def plot_images_ref(images, targets, paths=None, names=None, max_size=640, max_subplots=16, atlas=None, reduce=True, cap=None):
    """images numpy [B, 3 or 6, H, W]; targets numpy rows or ``(dets, counts)``.  Returns ``(mosaics, near_tie masks or None, flag)``."""
    B, C, H, W = images.shape
    bs, ns, sf, h, w, out_h, out_w = geometry(B, H, W, max_size, max_subplots)
    mosaics = [compose_ref(images, 3 * s, max_size, max_subplots) for s in range(C // 3)]
    if isinstance(targets, tuple):
        targets = output_to_target(*targets)
    targets = np.asarray(targets)
    flag = 0
    if targets.size:
        nc = len(names) if names else 1000
        cap = cap or max(1, max(int((targets[:, 0] == i).sum()) for i in range(bs)))
        slots, flag = slots_ref(targets, bs, cap, nc, h, w, sf)
        for i in range(bs):
            bx, by = w * (i // ns), h * (i % ns)
            draw_cell([m[by:by + h, bx:bx + w] for m in mosaics], slots[i], names, targets.shape[1] == 7, atlas)
    finish_ref(mosaics, bs, ns, h, w, paths, atlas)
    marks = None
    if reduce and (out_h, out_w) != (ns * h, ns * w):
        pairs = [area_ref(m, out_h, out_w) for m in mosaics]
        mosaics, marks = [p[0] for p in pairs], [p[1] for p in pairs]
    return mosaics, marks, flag


def area_ref(img, out_h, out_w):
    """``(dataset_ref.resize_area(img), dataset_ref.near_tie(img))`` for the sizes of a whole mosaic: the same tables and the same
    float64 real value, evaluated once and as two matrix products (a summation order of its own: float64's error is ten orders below
    the 2^-10 band that decides anything here)."""
    sh, sw = img.shape[:2]
    if dataset_ref.is_integer_scale((sh, sw), (out_h, out_w)):
        return dataset_ref.resize_area(img, (out_w, out_h)), np.zeros((out_h, out_w, img.shape[2]), bool)
    ty, tx = dataset_ref.area_tab(sh, out_h), dataset_ref.area_tab(sw, out_w)
    rows = np.tensordot(img.astype(np.float64), tx, axes=([1], [1]))          # [y, c, d]: the columns of every source row
    v = np.tensordot(ty, rows, axes=([1], [0])).transpose(0, 2, 1)           # [e, d, c]: then the rows
    return np.clip(np.rint(v), 0, 255).astype(np.uint8), np.abs(v - np.floor(v) - 0.5) < dataset_ref.TIE_BAND


def assert_area_equal(got, want, mark):
    """Equal everywhere except where the real value lies within 2^-10 of a tie (dataset_ref.near_tie): there the kernel's fp32 sum may
    round the other way, by one (the bound is derived in csrc/dataset.hip)."""
    got, want = got.astype(np.int64), want.astype(np.int64)
    assert got.shape == want.shape
    assert np.array_equal(got[~mark], want[~mark])
    assert (np.abs(got - want)[mark] <= 1).all()
