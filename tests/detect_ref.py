"""Host restatement of the detect stage (csrc/detect.hip), numpy / torch on the CPU.

* ``boxes_ref``   the box arithmetic of detect_twostream.py:129-153 op for op in float32 (torch on the CPU rounds each operation
                  once, as ATen does for the reference);
* ``hundredths``  f'{conf:.2f}' as an integer 0..100, in integer arithmetic on the float32's bits;
* ``render_ref``  the raster of include/cft_hip.h by plain ordered overdraw in the reference's loop order (reversed(det); outline,
                  background, text) - deliberately the other algorithm from the kernel's per-pixel search;
* ``label_lines`` / ``class_string`` / ``label_text``  the strings the host writes from the box buffer.
"""
import struct

import numpy as np
import torch

BOX_WORDS = 16


def hundredths(x):
    """round(x * 100) of the float32's exact value, ties to even, saturating at 0 and 100; NaN -> 0."""
    u = struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]
    if u >> 31:
        return 0
    ex, frac = u >> 23, u & 0x7fffff
    if ex == 255:
        return 0 if frac else 100
    m = (frac | 0x800000) if ex else frac
    e = (ex if ex else 1) - 150                 # value = m * 2^e
    p = 100 * m
    if e >= 0:
        q = p << e
    else:
        q, rem = p >> -e, p & ((1 << -e) - 1)
        half = 1 << (-e - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
    return min(q, 100)


def boxes_ref(dets, counts, geom, nc, gain=1.02, pad=10, square=False):
    """dets [B, max_det, 6] float32, counts [B], geom [B, 5] float32 (h0, w0, gain, padw, padh) -> dict of arrays shaped like the
    kernel's slots: xyxy int32 [B, max_det, 4], cls, conf100, valid int32 [B, max_det], conf float32, crop int32 [.., 4],
    xywhn float32 [.., 4], hist int32 [B, nc], flag int."""
    dets = torch.as_tensor(np.asarray(dets), dtype=torch.float32)
    geom = torch.as_tensor(np.asarray(geom), dtype=torch.float32)
    B, max_det = dets.shape[:2]
    out = {"xyxy": np.zeros((B, max_det, 4), np.int32), "cls": np.zeros((B, max_det), np.int32), "conf100": np.zeros((B, max_det), np.int32),
           "valid": np.zeros((B, max_det), np.int32), "conf": np.zeros((B, max_det), np.float32), "crop": np.zeros((B, max_det, 4), np.int32),
           "xywhn": np.zeros((B, max_det, 4), np.float32), "hist": np.zeros((B, nc), np.int32), "flag": 0}
    for b in range(B):
        n = max(0, min(int(counts[b]), max_det))
        if n == 0:
            continue
        h0, w0, g, pw, ph = (geom[b, i] for i in range(5))        # 0-dim float32 tensors: every op below is a float32 op
        d = dets[b, :n].clone()
        c = d[:, :4]
        c[:, [0, 2]] -= pw                                      # scale_coords
        c[:, [1, 3]] -= ph
        c[:, :4] /= g
        c[:, 0] = torch.minimum(torch.maximum(c[:, 0], torch.zeros(())), w0)      # clip_coords
        c[:, 1] = torch.minimum(torch.maximum(c[:, 1], torch.zeros(())), h0)
        c[:, 2] = torch.minimum(torch.maximum(c[:, 2], torch.zeros(())), w0)
        c[:, 3] = torch.minimum(torch.maximum(c[:, 3], torch.zeros(())), h0)
        c = c.round()                                           # half to even
        cx, cy = (c[:, 0] + c[:, 2]) / 2, (c[:, 1] + c[:, 3]) / 2                 # xyxy2xywh
        w, h = c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
        out["xyxy"][b, :n] = c.to(torch.int32).numpy()
        out["xywhn"][b, :n] = torch.stack((cx / w0, cy / h0, w / w0, h / h0), 1).numpy()
        cw, ch = (torch.maximum(w, h),) * 2 if square else (w, h)                 # save_one_box
        cw = cw * torch.tensor(gain, dtype=torch.float32) + torch.tensor(pad, dtype=torch.float32)
        ch = ch * torch.tensor(gain, dtype=torch.float32) + torch.tensor(pad, dtype=torch.float32)
        crop = torch.stack((cx - cw / 2, cy - ch / 2, cx + cw / 2, cy + ch / 2), 1).long()
        crop[:, [0, 2]] = crop[:, [0, 2]].clamp(0, int(w0))
        crop[:, [1, 3]] = crop[:, [1, 3]].clamp(0, int(h0))
        out["crop"][b, :n] = crop.to(torch.int32).numpy()
        cls = d[:, 5].to(torch.int32).numpy()                    # truncation toward zero
        out["cls"][b, :n] = cls
        out["conf"][b, :n] = d[:, 4].numpy()
        out["conf100"][b, :n] = [hundredths(v) for v in d[:, 4].numpy()]
        out["valid"][b, :n] = 1
        for k in cls:
            if 0 <= k < nc:
                out["hist"][b, k] += 1
            else:
                out["flag"] |= 1
    return out


def pack_slots(ref):
    """The dict of ``boxes_ref`` as the kernel's int32 [B, max_det, 16] buffer."""
    B, max_det = ref["cls"].shape
    buf = np.zeros((B, max_det, BOX_WORDS), np.int32)
    buf[..., 0:4] = ref["xyxy"]
    buf[..., 4], buf[..., 5], buf[..., 6] = ref["cls"], ref["conf100"], ref["valid"]
    buf[..., 7] = ref["conf"].view(np.int32)
    buf[..., 8:12] = ref["crop"]
    buf[..., 12:16] = ref["xywhn"].view(np.int32)
    return buf


def unpack_slots(buf):
    """The kernel's buffer (numpy int32 [B, max_det, 16]) as the dict of ``boxes_ref`` (without hist / flag)."""
    buf = np.ascontiguousarray(buf)
    return {"xyxy": buf[..., 0:4].copy(), "cls": buf[..., 4].copy(), "conf100": buf[..., 5].copy(), "valid": buf[..., 6].copy(),
            "conf": buf[..., 7].copy().view(np.float32), "crop": buf[..., 8:12].copy(), "xywhn": buf[..., 12:16].copy().view(np.float32)}


def label_lines(slots, b, save_conf):
    """The lines of labels/<stem>.txt for image b (detect_twostream.py:139-144): reversed(det), '%g' of class, xywh (, conf)."""
    n = int(slots["valid"][b].sum())
    lines = []
    for r in reversed(range(n)):
        line = (float(slots["cls"][b, r]), *(float(v) for v in slots["xywhn"][b, r]))
        if save_conf:
            line += (float(slots["conf"][b, r]),)
        lines.append(('%g ' * len(line)).rstrip() % line + '\n')
    return lines


def class_string(hist_row, names):
    """'3 persons, 1 car, ' (detect_twostream.py:134-136): classes ascending, an s for more than one."""
    return "".join(f"{int(n)} {names[c]}{'s' * (int(n) > 1)}, " for c, n in enumerate(hist_row) if n > 0)


def label_text(name, conf100, conf):
    return f"{name} {conf100 // 100}.{conf100 // 10 % 10}{conf100 % 10}" if conf else name


def render_ref(images, slots, b, colors, text_color, t, labels, conf, names, atlas):
    """Draw image b's slots into every HWC uint8 array of ``images`` (in place), by ordered overdraw."""
    h0, w0 = images[0].shape[:2]
    n_slots = slots["valid"].shape[1]
    a = t // 2
    m = max(1, (t + 1) // 3)
    gh, gw = (atlas.shape[1], atlas.shape[2]) if atlas is not None else (1, 1)

    def fill(X0, Y0, X1, Y1, color, hole=None):      # inclusive rectangle, clipped
        xa, xb, ya, yb = max(X0, 0), min(X1, w0 - 1) + 1, max(Y0, 0), min(Y1, h0 - 1) + 1
        if xa >= xb or ya >= yb:
            return
        ys, xs = np.mgrid[ya:yb, xa:xb]
        keep = np.ones(ys.shape, bool)
        if hole is not None:
            keep &= ~((xs >= hole[0]) & (xs <= hole[2]) & (ys >= hole[1]) & (ys <= hole[3]))
        for im in images:
            im[ys[keep], xs[keep]] = color

    for r in reversed(range(n_slots)):
        c = int(slots["cls"][b, r])
        if not slots["valid"][b, r] or not 0 <= c < len(colors):
            continue
        x1, y1, x2, y2 = (int(v) for v in slots["xyxy"][b, r])
        col = tuple(int(v) for v in colors[c])
        fill(x1 - a, y1 - a, x2 + a, y2 + a, col, hole=(x1 + t - a, y1 + t - a, x2 - t + a, y2 - t + a))
        text = label_text(names[c], int(slots["conf100"][b, r]), conf) if labels else ""
        if not text:
            continue
        fill(x1, y1 - gh * m - 3, x1 + len(text) * gw * m, y1, col)
        top = y1 - 1 - gh * m
        for k, ch in enumerate(text):
            code = ord(ch)
            on = np.repeat(np.repeat(atlas[code - 32 if 32 <= code <= 127 else 0] >= 128, m, 0), m, 1)      # nearest-neighbour magnification
            ys, xs = np.nonzero(on)
            ys, xs = ys + top, xs + x1 + k * gw * m
            ok = (xs >= 0) & (xs < w0) & (ys >= 0) & (ys < h0)
            for im in images:
                im[ys[ok], xs[ok]] = text_color


def case_inputs(case, max_det=None):
    """One fixture case as the kernel's inputs: dets [1, max_det, 6], counts [1], geom [1, 5]."""
    import msod_amd  # noqa: F401
    from msod_amd.utils.metrics import geometry
    d = case["dets"].numpy()
    n = len(d)
    max_det = max_det or max(1, n)
    dets = np.zeros((1, max_det, 6), np.float32)
    dets[0, :n] = d
    return dets, np.array([n], np.int32), geometry([(case["im0_shape"], None)], case["img_shape"]).numpy()


def check_case(case, slots, hist):
    """Every recorded result of one fixture case against slots (dict of arrays, image 0) and its class counts."""
    n = len(case["dets"])
    assert int(slots["valid"][0].sum()) == n
    assert np.array_equal(slots["xyxy"][0, :n], case["rounded"].numpy().astype(np.int32).reshape(n, 4))
    assert label_lines(slots, 0, False) == case["lines"]
    assert label_lines(slots, 0, True) == case["lines_conf"]
    assert class_string(hist[0], case["names"]) == case["s"]
    order = list(reversed(range(n)))
    assert [label_text(case["names"][slots["cls"][0, r]], int(slots["conf100"][0, r]), True) for r in order] == case["labels_conf"]
    for r, (y1, x1, hh, ww) in zip(order, case["crops"]):
        cx1, cy1, cx2, cy2 = (int(v) for v in slots["crop"][0, r])
        assert (max(cy2 - cy1, 0), max(cx2 - cx1, 0)) == (hh, ww)
        if hh and ww:
            assert (cy1, cx1) == (y1, x1)


def _neighbours(x):
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return [struct.unpack("<f", struct.pack("<I", v))[0] for v in (u - 1, u, u + 1)]


def hundredths_cases():
    """float32 values in [0, 1] for the hundredths routine: the ties of binary fractions and decimal x.xx5 with their float32
    neighbours, values around every x.xx, a few thousand seeded ones, 0 and 1."""
    vals = []
    for x in (0.125, 0.375, 0.005, 0.015, 0.995, 0.999999, 1.0, 0.5, 0.625, 0.875, 0.0049999, 2.0 ** -20, 0.01, 0.045, 0.555):
        vals += _neighbours(float(np.float32(x)))
    g = np.random.default_rng(5)
    vals += g.uniform(0, 1, 3000).astype(np.float32).tolist()
    vals += (g.integers(0, 101, 1000) / 100 + g.choice([-1, 0, 1], 1000) * 2.0 ** -24).clip(0, 1).astype(np.float32).tolist()      # around x.xx
    vals += ((2 * g.integers(0, 100, 1000) + 1) / 200).astype(np.float32).tolist()                                                  # around x.xx5
    vals += [0.0]
    return np.array(vals, np.float32)
