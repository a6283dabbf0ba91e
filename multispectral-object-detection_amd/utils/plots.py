"""Box drawing of the reference's ``utils/plots.py`` (``colors``, ``plot_one_box``) on the GPU: one launch of ``cft_detect_render``
draws every box of a batch into the device copies of the original images, both streams, in place (csrc/detect.hip); and its batch
mosaics (``plot_images``, ``output_to_target``), built on the device by the ``cft_mosaic_*`` kernels (csrc/mosaic.hip).

cv2 is not used: its anti-aliased thick lines and Hershey font are not reproduced ("parity with cv2 unpinned").  The raster is this
project's own definition, stated at ``cft_detect_render`` in include/cft_hip.h: hard-edged outlines of thickness ``t`` centred on the
box, a filled label background above the top-left corner and text from a bitmap glyph atlas magnified by ``max(1, (t + 1) // 3)``.
The reference's painter's order holds: it draws ``reversed(det)``, so the most confident box ends on top.
"""
import math
from collections import namedtuple
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from .. import ops
from ..ops import _require_cuda, detect_render
from .jpeg import encode_jpeg_start, is_jpeg_name

RENDER_LABELS, RENDER_CONF = _lib._consts["CFT_RENDER_LABELS"], _lib._consts["CFT_RENDER_CONF"]
RENDER_CONF1, RENDER_SIGNED = _lib._consts["CFT_RENDER_CONF1"], _lib._consts["CFT_RENDER_SIGNED"]
MOSAIC_BAD_CLASS, MOSAIC_OVERFLOW = _lib._consts["CFT_MOSAIC_BAD_CLASS"], _lib._consts["CFT_MOSAIC_OVERFLOW"]
NAME_CHARS = _lib._consts["CFT_MOSAIC_NAME_CHARS"]
MAX_REDUCTION = _lib._consts["CFT_PAIR_MAX_REDUCTION"]
MAX_NAME = _lib._consts["CFT_RENDER_MAX_NAME"]
RENDER_DESC = np.dtype([("img_rgb", "<u8"), ("img_ir", "<u8"), ("stride_rgb", "<i8"), ("stride_ir", "<i8"), ("h0", "<i4"), ("w0", "<i4"),
                        ("pad0", "<i4"), ("pad1", "<i4")])
assert RENDER_DESC.itemsize == _lib._consts["CFT_RENDER_DESC_BYTES"]
TEXT_COLOR_BGR = (225, 255, 255)          # utils/plots.py:81, in the channel order of the cv2 image it draws into


class Colors:
    """The reference's palette (utils/plots.py:29-41): matplotlib's ten Tableau colours, written out so matplotlib is not needed."""

    def __init__(self):
        hexes = ('#1f77b4', '#ff7f0e', '#2ca02c', '#d62728', '#9467bd', '#8c564b', '#e377c2', '#7f7f7f', '#bcbd22', '#17becf')
        self.palette = [self.hex2rgb(c) for c in hexes]
        self.n = len(self.palette)

    def __call__(self, i, bgr=False):
        c = self.palette[int(i) % self.n]
        return (c[2], c[1], c[0]) if bgr else c

    @staticmethod
    def hex2rgb(h):  # rgb order (PIL)
        return tuple(int(h[1 + i:1 + i + 2], 16) for i in (0, 2, 4))


colors = Colors()  # create instance for 'from utils.plots import colors'

_atlas_cache = {}


def glyph_atlas(font=None):
    """uint8 [96, gh, gw] bitmaps of ASCII 32..127, rasterised with PIL (``font`` None: PIL's default font, rasterised once and kept).
    A pixel is ink where the value is >= 128.  The cell is the largest glyph box of the set; every glyph is drawn from the cell's
    top-left corner."""
    if font is None and None in _atlas_cache:
        return _atlas_cache[None]
    from PIL import Image, ImageDraw, ImageFont
    f = font if font is not None else ImageFont.load_default()
    boxes = [f.getbbox(chr(c)) for c in range(32, 128)]
    gw, gh = max(1, max(b[2] for b in boxes)), max(1, max(b[3] for b in boxes))
    if gw > 64 or gh > 64:
        raise ValueError(f"glyph_atlas: a {gw}x{gh} glyph cell is larger than the kernel's 64x64")
    atlas = np.zeros((96, gh, gw), np.uint8)
    for c in range(32, 128):
        im = Image.new('L', (gw, gh), 0)
        ImageDraw.Draw(im).text((0, 0), chr(c), fill=255, font=f)
        atlas[c - 32] = np.asarray(im)
    if font is None:
        _atlas_cache[None] = atlas
    return atlas


def _upload(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


class BoxRenderer:
    """The device tables ``cft_detect_render`` reads, built once: class colours, class names as character codes, the glyph atlas.
    ``bgr`` is the channel order of the images drawn into (the reference draws into cv2's BGR images; PIL-decoded originals are RGB)."""

    def __init__(self, names, device, line_thickness=3, hide_labels=False, hide_conf=True, bgr=False, atlas=None, color_table=None,
                 text_color=None):
        names = [str(n) for n in names]
        nc = len(names)
        if nc < 1:
            raise ValueError("BoxRenderer: at least one class name")
        self.device = torch.device(device)
        self.thickness = int(line_thickness)
        if self.thickness < 1:
            raise ValueError("BoxRenderer: line_thickness must be >= 1")
        self.flags = 0 if hide_labels else (RENDER_LABELS | (0 if hide_conf else RENDER_CONF))
        table = np.array([colors(c, bgr) for c in range(nc)] if color_table is None else color_table, np.uint8).reshape(nc, 3)
        self.text_color = tuple(text_color) if text_color is not None else (TEXT_COLOR_BGR if bgr else TEXT_COLOR_BGR[::-1])
        self.colors = _upload(table, self.device)
        self.names = self.name_len = self.atlas = None
        if self.flags:
            L = max(1, max(len(n) for n in names))
            if L > MAX_NAME:
                raise ValueError(f"BoxRenderer: a class name longer than {MAX_NAME} characters")
            codes = np.zeros((nc, L), np.uint8)
            for i, n in enumerate(names):
                b = n.encode('ascii', 'replace')
                codes[i, :len(b)] = np.frombuffer(b, np.uint8)
            self.names = _upload(codes, self.device)
            self.name_len = _upload(np.array([len(n) for n in names], np.int32), self.device)
            self.atlas = _upload(glyph_atlas() if atlas is None else np.asarray(atlas, np.uint8), self.device)

    def __call__(self, boxes, images, images_ir=None):
        """Draw the slots of ``boxes`` (int32 [B, max_det, 16], ``ops.detect_boxes``) into ``images`` (B HWC uint8 CUDA tensors) and, when
        given, the same boxes into ``images_ir`` (same sizes).  In place, one launch, no synchronisation."""
        B = boxes.shape[0]
        if len(images) != B or (images_ir is not None and len(images_ir) != B):
            raise ValueError(f"plot_boxes: {B} images expected")
        desc = np.zeros(B, RENDER_DESC)
        for b, row in enumerate(desc):
            pair = (images[b],) if images_ir is None else (images[b], images_ir[b])
            for t in pair:
                _require_cuda(t, "plot_boxes")
                if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.stride(2) != 1 or t.stride(1) != 3:
                    raise ValueError("plot_boxes: images must be HWC uint8 CUDA tensors with contiguous pixels")
                if tuple(t.shape) != tuple(pair[0].shape):
                    raise ValueError(f"plot_boxes: the two images of pair {b} differ in size")
            row["img_rgb"], row["stride_rgb"], row["h0"], row["w0"] = pair[0].data_ptr(), pair[0].stride(0), pair[0].shape[0], pair[0].shape[1]
            if images_ir is not None:
                row["img_ir"], row["stride_ir"] = pair[1].data_ptr(), pair[1].stride(0)
        host = torch.from_numpy(desc.view(np.uint8).reshape(B, -1)).pin_memory()
        dev = host.to(self.device, non_blocking=True)
        detect_render(dev, host, boxes, self.colors, self.text_color, self.thickness, self.flags, self.names, self.name_len, self.atlas)
        return images if images_ir is None else (images, images_ir)


def plot_boxes(boxes, images, images_ir=None, names=None, line_thickness=3, hide_labels=False, hide_conf=True, bgr=False, atlas=None,
               color_table=None, text_color=None):
    """The batched ``plot_one_box``: every valid slot of ``boxes`` into its image (and its IR twin), in place.  ``names`` None draws no labels."""
    if names is None:
        names, hide_labels = [""] * (len(color_table) if color_table is not None else colors.n), True
    r = BoxRenderer(names, boxes.device, line_thickness, hide_labels, hide_conf, bgr, atlas, color_table, text_color)
    return r(boxes, images, images_ir)


def plot_one_box(x, im, color=None, label=None, line_thickness=3, atlas=None, bgr=False):
    """The reference's ``plot_one_box`` (utils/plots.py:67-81) on an HWC uint8 CUDA tensor, in place: one box ``x`` = (x1, y1, x2, y2),
    truncated with ``int()`` as there, through the same kernel.  ``color`` is in the image's channel order (None: a random colour, as
    the reference); ``bgr`` says which order that is, for the text colour: the reference's [225, 255, 255] belongs to a BGR image and is
    reversed for an RGB one, as ``BoxRenderer`` does.  Every call builds and uploads the renderer's tables (colour, label, atlas): for
    more than a few boxes use ``plot_boxes`` / ``BoxRenderer``, which draw a whole batch with one launch and no per-box host work."""
    import random
    _require_cuda(im, "plot_one_box")
    tl = line_thickness or round(0.002 * (im.shape[0] + im.shape[1]) / 2) + 1
    color = color or [random.randint(0, 255) for _ in range(3)]
    slot = np.zeros((1, 1, 16), np.int32)
    slot[0, 0, :4] = [int(v) for v in x]
    slot[0, 0, 6] = 1
    boxes = _upload(slot, im.device)
    r = BoxRenderer([label or ""], im.device, tl, not label, True, bgr=bgr, atlas=atlas, color_table=[color])
    r(boxes, [im])
    return im


# ---------------------------------------------------------------------------------------------------------------- batch mosaics
MosaicGeometry = namedtuple("MosaicGeometry", "bs ns sf h w resize r out_h out_w")
NUMBERED_CLASSES = 1000          # names=None draws the class number: the table holds '0' .. '999'
_renderers = {}


def mosaic_geometry(B, H, W, max_size=640, max_subplots=16):
    """The reference's grid (utils/plots.py:142-152) and final size (:199-200), in Python doubles as there: ``bs`` images in an ``ns x ns``
    grid of ``h x w`` cells (resized when ``sf < 1``), saved at ``out_h x out_w`` (``r`` < 1: the INTER_AREA reduction).  A reduction beyond
    4x per axis raises ValueError: the area kernel does not do it."""
    if B < 1 or H < 1 or W < 1 or max_subplots < 1 or not max_size > 0:
        raise ValueError(f"plot_images: bad sizes (B {B}, {H}x{W}, max_size {max_size}, max_subplots {max_subplots})")
    bs = min(B, max_subplots)
    ns = math.ceil(bs ** 0.5)
    sf = max_size / max(H, W)
    h, w = (math.ceil(sf * H), math.ceil(sf * W)) if sf < 1 else (H, W)
    r = min(1280. / max(h, w) / ns, 1.0)
    out_h, out_w = int(ns * h * r), int(ns * w * r)
    if out_h < 1 or out_w < 1 or ns * h > MAX_REDUCTION * out_h or ns * w > MAX_REDUCTION * out_w:
        raise ValueError(f"plot_images: a {ns * h}x{ns * w} mosaic would be saved at {out_h}x{out_w}, more than {MAX_REDUCTION}x smaller per axis; "
                         "lower max_size or max_subplots")
    return MosaicGeometry(bs, ns, sf, h, w, sf < 1, r, out_h, out_w)


def ir_name(fname):
    """``<stem>_ir<suffix>`` next to ``fname``: where the IR mosaic of a six-channel batch is saved."""
    p = Path(fname)
    return p.with_name(p.stem + '_ir' + p.suffix)


def output_to_target(output):
    """The reference's ``output_to_target`` (utils/plots.py:119-125): a list of per-image ``[n_i, 6]`` tensors (xyxy, conf, cls) ->
    ``[n, 7]`` float32 rows ``image, class, x, y, w, h, conf`` on the inputs' device.  torch operations only, no synchronisation."""
    rows = []
    for i, o in enumerate(output):
        o = o.float()
        x1, y1, x2, y2 = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
        rows.append(torch.stack((torch.full_like(x1, float(i)), o[:, 5], (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, o[:, 4]), 1))     # xyxy2xywh
    if not rows:
        return torch.zeros((0, 7), dtype=torch.float32)
    return torch.cat(rows, 0)


def _class_names(names):
    if not names:
        return None
    if isinstance(names, dict):
        return tuple(str(names[k]) for k in range(len(names)))
    return tuple(str(n) for n in names)


def _mosaic_renderer(names, device):
    """The colour / name / atlas tables of one class list on one device, built once and kept."""
    key = (names, str(device))
    if key not in _renderers:
        table = names if names is not None else tuple(str(c) for c in range(NUMBERED_CLASSES))
        _renderers[key] = BoxRenderer(table, device, line_thickness=3, hide_conf=False, text_color=TEXT_COLOR_BGR)   # :81's literal, in the mosaic's own order
    return _renderers[key]


def _mosaic_targets(targets, bs, device):
    """``(device targets or None, cap, has_conf)``: rows as a contiguous float32 / float64 CUDA tensor, or the ``(dets, counts)`` pair.
    ``cap`` (slots per cell) comes from the host alone: the exact per-image maximum for CPU targets, nt for device rows, max_det for the pair."""
    if isinstance(targets, (tuple, list)) and len(targets) == 2 and torch.is_tensor(targets[0]) and targets[0].dim() == 3:
        dets, counts = targets
        _require_cuda(dets, "plot_images")
        if dets.shape[1] == 0:
            return None, 0, True
        return (dets.float().contiguous(), counts.to(torch.int32).contiguous()), dets.shape[1], True
    if isinstance(targets, np.ndarray):
        targets = torch.from_numpy(np.ascontiguousarray(targets))
    elif not torch.is_tensor(targets):
        targets = torch.as_tensor(np.asarray(targets))
    if targets.numel() == 0 or targets.shape[0] == 0:
        return None, 0, False
    if targets.dim() != 2 or targets.shape[1] not in (6, 7):
        raise ValueError(f"plot_images: targets must be [nt, 6] (labels) or [nt, 7] (with confidence), got {tuple(targets.shape)}")
    if targets.dtype not in (torch.float32, torch.float64):
        targets = targets.float()
    has_conf = targets.shape[1] == 7
    if targets.is_cuda:
        return targets.contiguous(), targets.shape[0], has_conf
    idx = targets[:, 0].numpy()
    cap = max(1, max(int((idx == i).sum()) for i in range(bs)))
    return targets.contiguous().pin_memory().to(device, non_blocking=True), cap, has_conf


def _path_codes(paths, bs, device):
    """The first 40 characters of each base name as codes (a character outside 32..127 becomes 0 and draws as a space)."""
    codes, lens = np.zeros((bs, NAME_CHARS), np.uint8), np.zeros(bs, np.int32)
    for i in range(min(bs, len(paths))):
        label = Path(paths[i]).name[:NAME_CHARS]           # :190
        lens[i] = len(label)
        codes[i, :len(label)] = [ord(ch) if 32 <= ord(ch) <= 127 else 0 for ch in label]
    return _upload(codes, device), _upload(lens, device)


def cell_descriptors(mosaics, g):
    """The ``cft_render_desc_t`` table that makes every occupied cell one "image" of ``cft_detect_render``: the pointer is the cell's
    origin in the mosaic, the stride the mosaic's, the size the cell's, so drawing is clipped to the cell.  ``(device, host)`` tensors."""
    desc = np.zeros(g.bs, RENDER_DESC)
    for i, row in enumerate(desc):
        off = g.h * (i % g.ns) * mosaics[0].stride(0) + g.w * (i // g.ns) * 3
        row["img_rgb"], row["stride_rgb"], row["h0"], row["w0"] = mosaics[0].data_ptr() + off, mosaics[0].stride(0), g.h, g.w
        if len(mosaics) == 2:
            row["img_ir"], row["stride_ir"] = mosaics[1].data_ptr() + off, mosaics[1].stride(0)
    host = torch.from_numpy(desc.view(np.uint8).reshape(g.bs, -1)).pin_memory()
    return host.to(mosaics[0].device, non_blocking=True), host


def mosaic_render_flags(has_conf):
    return RENDER_LABELS | RENDER_SIGNED | ((RENDER_CONF | RENDER_CONF1) if has_conf else 0)


def plot_images_device(images, targets, paths=None, names=None, max_size=640, max_subplots=16, reduce=True):
    """The device stage of ``plot_images``: ``(mosaics, flag, geometry)`` with one HWC uint8 CUDA mosaic per stream (after the area
    reduction when ``reduce``) and the int32 [1] flag word (None without targets).  Nothing here synchronises."""
    if not torch.is_tensor(images):
        raise TypeError("plot_images: images must be a CUDA tensor (the mosaic is built on the device)")
    if images.dim() != 4 or images.shape[1] not in (3, 6) or images.shape[0] == 0:
        raise ValueError(f"plot_images: images must be [B, 3 or 6, H, W], got {tuple(images.shape)}")
    B, C, H, W = images.shape
    g = mosaic_geometry(B, H, W, max_size, max_subplots)          # refusals come before any device work
    _require_cuda(images, "plot_images")
    if images.dtype not in (torch.uint8, torch.float16, torch.float32):
        images = images.float()
    device = images.device
    names = _class_names(names)
    tg, cap, has_conf = _mosaic_targets(targets, g.bs, device)
    mosaics = [torch.empty((g.ns * g.h, g.ns * g.w, 3), dtype=torch.uint8, device=device) for _ in range(C // 3)]
    maxkey = torch.empty((1,), dtype=torch.int32, device=device)
    for s, m in enumerate(mosaics):
        ops.mosaic_compose(images, 3 * s, g.bs, g.ns, g.h, g.w, g.resize, m, maxkey)
    flag = None
    rnd = _mosaic_renderer(names, device) if (tg is not None or paths) else None
    if tg is not None:
        slots, flag = ops.mosaic_slots(tg, g.bs, cap, len(rnd.colors), g.h, g.w, g.sf)
        desc_dev, desc_host = cell_descriptors(mosaics, g)
        detect_render(desc_dev, desc_host, slots, rnd.colors, rnd.text_color, 3, mosaic_render_flags(has_conf), rnd.names, rnd.name_len, rnd.atlas)
    codes = lens = None
    if paths:
        codes, lens = _path_codes(paths, g.bs, device)
    ops.mosaic_finish(mosaics[0], mosaics[1] if len(mosaics) == 2 else None, g.bs, g.ns, g.h, g.w, codes, lens, None if codes is None else rnd.atlas)
    if reduce and (g.out_h, g.out_w) != (g.ns * g.h, g.ns * g.w):
        mosaics = [ops.mosaic_area(m, g.out_h, g.out_w) for m in mosaics]
    return mosaics, flag, g


def check_mosaic_flag(word):
    """Raise for the flag word of ``cft_mosaic_slots`` (a host int)."""
    if word & MOSAIC_BAD_CLASS:
        raise ValueError("plot_images: a target's class is outside the names table")
    if word & MOSAIC_OVERFLOW:
        raise ValueError("plot_images: more drawn targets in one image than slots")


def mosaic_file_names(fname, n):
    return [Path(fname)] if n == 1 else [Path(fname), ir_name(fname)]


def save_mosaic(array, fname):
    from PIL import Image
    Image.fromarray(array).save(fname)          # :202


def plot_images(images, targets, paths=None, fname='images.jpg', names=None, max_size=640, max_subplots=16, device_jpeg=False):
    """The reference's ``plot_images`` (utils/plots.py:128-203) on the GPU: the first ``max_subplots`` images of a batch in a square
    grid (column-major, as there), the targets drawn in, file names and cell borders on top, reduced to at most 1280 pixels a side and
    saved when ``fname`` is given.

    ``images``: a ``[B, 3 or 6, H, W]`` CUDA tensor (uint8, or float in 0..1 or 0..255: multiplied by 255 when the maximum of image 0
    is <= 1, decided on the device).  ``targets``: a tensor / ndarray ``[nt, 6]`` (image, class, x, y, w, h: labels) or ``[nt, 7]`` (with
    confidence; drawn above 0.25) on either device, normalised or in pixels (decided per image, as there); the ``(dets, counts)`` pair of
    ``batched_nms`` (``output_to_target`` is fused into the kernel); or an empty array.  ``names`` None draws the class number
    (classes below 1000).

    Returns the HWC uint8 CUDA mosaic, after the area reduction when ``fname`` is given, as the reference returns it.  A six-channel
    batch has no precedent (the reference's thread dies on it, test.py:223): here it gives the pair ``(rgb, ir)`` with the same boxes in
    both, saved as ``fname`` and ``<stem>_ir<suffix>``.

    Everything stays on the device and nothing synchronises until the bytes are needed: saving is one device-to-host copy per mosaic
    and a PIL save, and there the kernel's flag word is read: a class outside the table or more drawn targets than slots raise ValueError.
    ``device_jpeg`` with a .jpg / .jpeg name: the file is written by ``utils.jpeg.encode_jpeg_start`` instead (the DCT on the device, the
    quantised coefficients copied, Huffman coding on the host) and holds the same bytes.

    The raster is this project's own (cv2 is absent: "parity unpinned"), defined in include/cft_hip.h: float32 bilinear resize in
    OpenCV's published coordinate convention, the hard-edged boxes and atlas text of ``plot_one_box``, ``' d.d'`` confidences.
    Deliberate differences: every cell is drawn as one image, so boxes and labels are clipped to their cell (the reference lets a label
    spill into the neighbouring cell); coordinates are truncated relative to the cell; the file name is drawn with its top-left at
    (block_x + 5, block_y + 5)."""
    mosaics, flag, _ = plot_images_device(images, targets, paths, names, max_size, max_subplots, reduce=bool(fname))
    if fname and device_jpeg and is_jpeg_name(fname):
        job = encode_jpeg_start(list(mosaics))
        if flag is not None:
            check_mosaic_flag(int(flag.item()))
        for k, f in enumerate(mosaic_file_names(fname, len(job))):
            job.save(k, f)
    elif fname:
        host = [m.cpu() for m in mosaics]
        if flag is not None:
            check_mosaic_flag(int(flag.item()))
        for a, f in zip(host, mosaic_file_names(fname, len(host))):
            save_mosaic(a.numpy(), f)
    return mosaics[0] if len(mosaics) == 1 else tuple(mosaics)
