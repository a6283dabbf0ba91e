"""Box drawing of the reference's ``utils/plots.py`` (``colors``, ``plot_one_box``) on the GPU: one launch of ``cft_detect_render``
draws every box of a batch into the device copies of the original images, both streams, in place (csrc/detect.hip).

cv2 is not used: its anti-aliased thick lines and Hershey font are not reproduced ("parity with cv2 unpinned").  The raster is this
project's own definition, stated at ``cft_detect_render`` in include/cft_hip.h: hard-edged outlines of thickness ``t`` centred on the
box, a filled label background above the top-left corner and text from a bitmap glyph atlas magnified by ``max(1, (t + 1) // 3)``.
The reference's painter's order holds: it draws ``reversed(det)``, so the most confident box ends on top.
"""
import numpy as np
import torch

from .. import _lib
from ..ops import _require_cuda, detect_render

RENDER_LABELS, RENDER_CONF = _lib._consts["CFT_RENDER_LABELS"], _lib._consts["CFT_RENDER_CONF"]
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
