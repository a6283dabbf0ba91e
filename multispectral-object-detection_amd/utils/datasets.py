"""Input pre-processing that sits directly in front of the forward in every reference caller:
``letterbox`` of the reference's ``utils/datasets.py:1698-1728`` - resize to a stride-friendly shape keeping the
aspect ratio, pad with grey - on the device, one kernel per image (``cft_letterbox_u8``), and the pair packer that
builds the uint8 ``[B,6,H,W]`` batch the model consumes (``utils/datasets.py:1274-1281``: BGR->RGB, HWC->CHW); below them the paired
RGB + IR dataset and its loaders, validation form (one cft_pair_batch_u8 launch per batch) and augmented training form (one
cft_augment_batch_u8 launch per batch), and the inference loaders of the detect driver.  The three batched loaders share one prefetch
pipeline (``_Prefetch``, described where it is defined) and one decode-and-upload (``_upload``); each states only its table and launch."""
import glob
import os
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from ..ops import _require_cuda, _stream

def letterbox_geometry(shape, new_shape=(640, 640), auto=True, scaleFill=False, scaleup=True, stride=32):
    """The arithmetic of reference utils/datasets.py:1700-1726, verbatim in meaning: returns
    (new_unpad (w, h), ratio (w, h), (dw, dh) per side, (top, bottom, left, right))."""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)
    elif scaleFill:
        dw, dh = 0.0, 0.0
        new_unpad = (new_shape[1], new_shape[0])
        ratio = new_shape[1] / shape[1], new_shape[0] / shape[0]
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return new_unpad, ratio, (dw, dh), (top, bottom, left, right)


def letterbox(img, new_shape=(640, 640), color=(114, 114, 114), auto=True, scaleFill=False, scaleup=True, stride=32, out=None,
              chw_rgb=False):
    """Same signature and return value as the reference's ``letterbox``: ``img`` is an HWC uint8 image (cv2 order, BGR)
    as a CUDA tensor; returns ``(img, ratio, (dw, dh))`` with ``img`` the letterboxed HWC uint8 CUDA tensor.
    ``chw_rgb=True`` (or ``out=`` a [3,H,W] view) writes the CHW RGB plane instead - the layout the callers build next
    (``img[:, :, ::-1].transpose(2, 0, 1)``), e.g. straight into a slice of the [B,6,H,W] pair batch."""
    _require_cuda(img, "letterbox")
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or img.stride(2) != 1 or img.stride(1) != 3:
        raise ValueError("letterbox: expected an HWC uint8 image with contiguous pixels")
    sh, sw = int(img.shape[0]), int(img.shape[1])
    new_unpad, ratio, (dw, dh), (top, bottom, left, right) = letterbox_geometry((sh, sw), new_shape, auto, scaleFill, scaleup, stride)
    rw, rh = new_unpad
    H, W = rh + top + bottom, rw + left + right
    if out is None:
        out = torch.empty((3, H, W) if chw_rgb else (H, W, 3), dtype=torch.uint8, device=img.device)
    if tuple(out.shape) == (3, H, W):
        sy, sx, sc, flip = out.stride(1), out.stride(2), out.stride(0), 1
    elif tuple(out.shape) == (H, W, 3):
        sy, sx, sc, flip = out.stride(0), out.stride(1), out.stride(2), 0
    else:
        raise ValueError(f"letterbox: out has shape {tuple(out.shape)}, expected {(H, W, 3)} or {(3, H, W)}")
    st = _lib.load().cft_letterbox_u8(img.data_ptr(), sh, sw, img.stride(0), out.data_ptr(), H, W, sy, sx, sc, flip,
                                      rh, rw, top, left, int(color[0]), int(color[1]), int(color[2]), _stream())
    _lib.check(st, "cft_letterbox_u8")
    return out, ratio, (dw, dh)


def letterbox_pair(img_rgb, img_ir, new_shape=640, stride=32, auto=False, scaleup=False, out=None):
    """One RGB + one IR image (HWC BGR uint8, the pair of utils/datasets.py:1206-1207) -> the uint8 [6,H,W] block of the
    batch (RGB plane 0-2, IR plane 3-5), both letterboxed to the same shape, BGR->RGB and HWC->CHW fused into the kernel."""
    new_unpad, _, _, (top, bottom, left, right) = letterbox_geometry(tuple(img_rgb.shape[:2]), new_shape, auto, False, scaleup, stride)
    H, W = new_unpad[1] + top + bottom, new_unpad[0] + left + right
    if out is None:
        out = torch.empty((6, H, W), dtype=torch.uint8, device=img_rgb.device)
    _, ratio, pad = letterbox(img_rgb, new_shape, auto=auto, scaleup=scaleup, stride=stride, out=out[:3])
    letterbox(img_ir, new_shape, auto=auto, scaleup=scaleup, stride=stride, out=out[3:])
    return out, ratio, pad


# ------------------------------------------------------------------------------ paired RGB + IR dataset, validation form
# The non-augmented (validation / rect) form of the reference's LoadMultiModalImagesAndLabels and create_dataloader_rgb_ir
# (utils/datasets.py:820-1288, :223-257).  The host keeps the reference's bookkeeping - file lists, label checks, the rect sort and
# batch shapes, targets and shapes - and decodes the files; everything between the decoded originals and the uint8 [B,6,H,W] batch
# is ONE launch of cft_pair_batch_u8 per batch (csrc/dataset.hip).
img_formats = ['bmp', 'jpg', 'jpeg', 'png', 'tif', 'tiff', 'dng', 'webp', 'mpo']  # acceptable image suffixes (reference :33)
PAIR_COPY, PAIR_LINEAR, PAIR_AREA = (_lib._consts[k] for k in ("CFT_PAIR_COPY", "CFT_PAIR_LINEAR", "CFT_PAIR_AREA"))
PAIR_MODE_NAMES = {PAIR_COPY: "copy", PAIR_LINEAR: "linear", PAIR_AREA: "area"}
# one row of the table cft_pair_batch_u8 reads: cft_pair_desc_t of include/cft_hip.h
PAIR_DESC = np.dtype([("src_rgb", "<u8"), ("src_ir", "<u8"), ("stride_rgb", "<i8"), ("stride_ir", "<i8"), ("h0", "<i4"), ("w0", "<i4"),
                      ("h", "<i4"), ("w", "<i4"), ("top", "<i4"), ("left", "<i4"), ("mode", "<i4"), ("flip", "<i4")])
assert PAIR_DESC.itemsize == _lib._consts["CFT_PAIR_DESC_BYTES"]
PAIR_MAX_REDUCTION = _lib._consts["CFT_PAIR_MAX_REDUCTION"]
MAX_DECODE_THREADS = 16


class LetterboxResizes(AssertionError):
    """Raised where a batch's table is built if the letterbox itself would resize a pair: cft_pair_batch_u8 has one resize stage,
    the loader then assembles that batch pair by pair with ``letterbox_pair``."""


def img2label_paths(img_paths):
    """Label paths as a function of image paths (reference utils/datasets.py:518-521): /images/ -> /labels/, suffix -> txt."""
    sa, sb = os.sep + 'images' + os.sep, os.sep + 'labels' + os.sep  # /images/, /labels/ substrings
    return ['txt'.join(x.replace(sa, sb, 1).rsplit(x.split('.')[-1], 1)) for x in img_paths]


def xywhn2xyxy(x, w=640, h=640, padw=0, padh=0):
    """nx4 boxes from normalised [x, y, w, h] to pixel [x1, y1, x2, y2] (reference utils/general.py:309-316)."""
    y = x.clone() if isinstance(x, torch.Tensor) else np.copy(x)
    y[:, 0] = w * (x[:, 0] - x[:, 2] / 2) + padw  # top left x
    y[:, 1] = h * (x[:, 1] - x[:, 3] / 2) + padh  # top left y
    y[:, 2] = w * (x[:, 0] + x[:, 2] / 2) + padw  # bottom right x
    y[:, 3] = h * (x[:, 1] + x[:, 3] / 2) + padh  # bottom right y
    return y


def xyxy2xywh(x):
    """nx4 boxes from [x1, y1, x2, y2] to [x, y, w, h], tensors and numpy arrays alike (reference utils/general.py:289-296)."""
    y = x.clone() if isinstance(x, torch.Tensor) else np.copy(x)
    y[:, 0] = (x[:, 0] + x[:, 2]) / 2  # x center
    y[:, 1] = (x[:, 1] + x[:, 3]) / 2  # y center
    y[:, 2] = x[:, 2] - x[:, 0]  # width
    y[:, 3] = x[:, 3] - x[:, 1]  # height
    return y


def _exif_size(img):
    """Exif-corrected PIL size (reference utils/datasets.py:89-101)."""
    from PIL import ExifTags
    orientation = next((k for k, v in ExifTags.TAGS.items() if v == 'Orientation'), None)
    s = img.size  # (width, height)
    try:
        rotation = dict(img._getexif().items())[orientation]
        if rotation in (6, 8):  # rotation 270 / 90
            s = (s[1], s[0])
    except Exception:
        pass
    return s


def _list_images(path, prefix=''):
    """Image files of a directory (recursive), a *.txt list, or a list of those (reference utils/datasets.py:859-895)."""
    f = []
    for p in path if isinstance(path, list) else [path]:
        p = Path(p)  # os-agnostic
        if p.is_dir():  # dir
            f += glob.glob(str(p / '**' / '*.*'), recursive=True)
        elif p.is_file():  # file
            with open(p, 'r') as t:
                t = t.read().strip().splitlines()
                parent = str(p.parent) + os.sep
                f += [x.replace('./', parent) if x.startswith('./') else x for x in t]  # local to global path
        else:
            raise Exception(f'{prefix}{p} does not exist')
    return sorted([x.replace('/', os.sep) for x in f if x.split('.')[-1].lower() in img_formats])


def verify_image_label(im_file, lb_file):
    """The per-image checks of the reference's ``cache_labels`` (utils/datasets.py:1097-1127): returns ``(labels [n, 5] float32,
    shape (w, h), state)`` with state 'found' / 'empty' / 'missing'; raises (AssertionError, OSError, ValueError) where the reference
    counts the image as corrupted and ignores it."""
    from PIL import Image
    im = Image.open(im_file)
    im.verify()  # PIL verify
    shape = _exif_size(im)  # image size
    assert (shape[0] > 9) & (shape[1] > 9), f'image size {shape} <10 pixels'
    assert im.format.lower() in img_formats, f'invalid image format {im.format}'
    if not os.path.isfile(lb_file):
        return np.zeros((0, 5), dtype=np.float32), shape, 'missing'
    with open(lb_file, 'r') as f:
        l = [x.split() for x in f.read().strip().splitlines()]
    if any([len(x) > 8 for x in l]):
        raise ValueError('segment labels are not supported (only the box form: class x y w h)')
    l = np.array(l, dtype=np.float32)
    if not len(l):
        return np.zeros((0, 5), dtype=np.float32), shape, 'empty'
    assert l.shape[1] == 5, 'labels require 5 columns each'
    assert (l >= 0).all(), 'negative labels'
    assert (l[:, 1:] <= 1).all(), 'non-normalized or out of bounds coordinate labels'
    assert np.unique(l, axis=0).shape[0] == l.shape[0], 'duplicate labels'
    return l, shape, 'found'


def decode_image(path):
    """One image file as an HWC uint8 array in RGB order (PIL; the reference's cv2.imread gives the same pixels in BGR order)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def use_device_jpeg(dataset_or_loader, enabled=True):
    """Switch the loaders of a paired dataset (or of the loader given) to decoding baseline JPEG files on the GPU: the Huffman half on
    the decode pool (cft_jpeg_entropy), dequantisation, IDCT, chroma upsampling and colour conversion in one cft_jpeg_decode_u8 call per
    batch, byte for byte what PIL decodes.  Files that are not JPEG or not in the supported subset (include/cft_hip.h) go through PIL as
    before, judged per file.  ``enabled=False`` switches back.  Returns its argument."""
    ds = getattr(dataset_or_loader, "dataset", dataset_or_loader)
    if not hasattr(ds, "decode"):
        raise TypeError(f"use_device_jpeg: {type(dataset_or_loader).__name__} is neither a paired dataset nor its loader")
    ds.decode = 'device' if enabled else 'pil'
    return dataset_or_loader


def _probe_jpeg(path):
    """``(bytes, info)`` of a file the device decoder takes, ``(None, None)`` for every other file (it is then read by PIL)."""
    from .jpeg import jpeg_info
    with open(path, 'rb') as f:
        if f.read(2) != b'\xff\xd8':
            return None, None
        f.seek(0)
        blob = f.read()
    info = jpeg_info(blob)
    return (blob, info) if info is not None else (None, None)


class LoadMultiModalImagesAndLabels:  # for testing
    """The reference's paired RGB + IR dataset (utils/datasets.py:820-1288), same constructor, in its non-augmented form:
    ``augment=True`` (mosaic, HSV, flips, perspective) raises NotImplementedError.  Differences that are deliberate:

    * labels are held in memory, no ``.cache`` file is written beside the data;
    * the reference sorts the RGB and the IR list independently (one order for aligned pairs): here the RGB order is applied to
      both lists, a pair that the reference would ignore as corrupted in either list is dropped as a pair, and a pair whose two
      images differ in size raises ValueError;
    * ``cache_images`` (True or 'device') keeps the decoded originals as uint8 CUDA tensors after the first pass of the loader.

    ``shapes`` / ``labels`` / ``img_files_rgb`` / ``img_files_ir`` / ``n`` / ``batch_rgb`` / ``batch_shapes_rgb`` / ``indices_rgb``
    are the reference's attributes, so the object can be handed to ``check_anchors_rgb_ir`` and ``kmean_anchors``."""

    def __init__(self, path_rgb, path_ir, img_size=640, batch_size=16, augment=False, hyp=None, rect=False, image_weights=False,
                 cache_images=False, single_cls=False, stride=32, pad=0.0, prefix=''):
        if augment:
            raise NotImplementedError("LoadMultiModalImagesAndLabels: augment=True (mosaic, HSV, flips, perspective) is not implemented; "
                                      "this package builds the non-augmented validation / rect form only")
        if cache_images not in (False, None, True, 'device'):
            raise ValueError(f"cache_images must be False, True or 'device', got {cache_images!r}")
        self.img_size = img_size
        self.augment = augment
        self.hyp = hyp
        self.image_weights = image_weights
        self.rect = False if image_weights else rect
        self.mosaic = False
        self.stride = stride
        self.path_rgb = path_rgb
        self.path_ir = path_ir
        self.pad = pad
        self.cache_images = bool(cache_images)
        self.decode = 'pil'      # 'device': the loaders decode baseline JPEG files on the GPU (use_device_jpeg), everything else stays with PIL
        self.jpeg_infos = {}     # decode = 'device': path -> cft_jpeg_info of the file, None for a file that PIL has to decode

        try:
            files_rgb, files_ir = _list_images(path_rgb, prefix), _list_images(path_ir, prefix)
            assert files_rgb and files_ir, f'{prefix}No images found'
        except Exception as e:
            raise Exception(f'{prefix}Error loading data from {path_rgb, path_ir}: {e}')
        if len(files_rgb) != len(files_ir):
            raise ValueError(f'{prefix}{len(files_rgb)} RGB images but {len(files_ir)} IR images: the two lists do not pair up')

        # labels and shapes (cache_labels, :1089-1144), in memory
        self.img_files_rgb, self.img_files_ir, labels, shapes = [], [], [], []
        nf = nm = ne = nc = 0  # number found, missing, empty, corrupted
        for f_rgb, f_ir, l_rgb, l_ir in zip(files_rgb, files_ir, img2label_paths(files_rgb), img2label_paths(files_ir)):
            try:
                l, shape, state = verify_image_label(f_rgb, l_rgb)
                _, shape_ir, _ = verify_image_label(f_ir, l_ir)
            except (AssertionError, OSError, ValueError, SyntaxError) as e:
                nc += 1
                print(f'{prefix}WARNING: Ignoring corrupted image and/or label {f_rgb}: {e}')
                continue
            if tuple(shape) != tuple(shape_ir):
                raise ValueError(f'{prefix}unaligned pair: {f_rgb} is {shape[0]}x{shape[1]} but {f_ir} is {shape_ir[0]}x{shape_ir[1]}')
            nf, nm, ne = nf + (state == 'found'), nm + (state == 'missing'), ne + (state == 'empty')
            self.img_files_rgb.append(f_rgb)
            self.img_files_ir.append(f_ir)
            labels.append(l)
            shapes.append(shape)
        self.scan_results = nf, nm, ne, nc, len(files_rgb)
        if not shapes:
            raise Exception(f'{prefix}No usable image pairs in {path_rgb, path_ir}')
        self.labels_rgb = labels
        self.shapes_rgb = np.array(shapes, dtype=np.float64)
        self.label_files_rgb = img2label_paths(self.img_files_rgb)
        self.label_files_ir = img2label_paths(self.img_files_ir)
        if single_cls:
            for x in self.labels_rgb:
                x[:, 0] = 0

        n = len(shapes)  # number of images
        bi = np.floor(np.arange(n) / batch_size).astype(int)  # batch index
        nb = bi[-1] + 1  # number of batches
        self.batch_rgb = bi  # batch index of image
        self.n = self.n_rgb = n
        self.indices_rgb = range(n)

        # Rectangular Training (:1009-1032)
        if self.rect:
            s = self.shapes_rgb  # wh
            ar = s[:, 1] / s[:, 0]  # aspect ratio
            irect = ar.argsort()
            self.img_files_rgb = [self.img_files_rgb[i] for i in irect]
            self.img_files_ir = [self.img_files_ir[i] for i in irect]       # the RGB order, applied to both lists
            self.label_files_rgb = [self.label_files_rgb[i] for i in irect]
            self.label_files_ir = [self.label_files_ir[i] for i in irect]
            self.labels_rgb = [self.labels_rgb[i] for i in irect]
            self.shapes_rgb = s[irect]  # wh
            ar = ar[irect]

            # Set training image shapes
            shapes = [[1, 1]] * nb
            for i in range(nb):
                ari = ar[bi == i]
                mini, maxi = ari.min(), ari.max()
                if maxi < 1:
                    shapes[i] = [maxi, 1]
                elif mini > 1:
                    shapes[i] = [1, 1 / mini]

            self.batch_shapes_rgb = np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride

        self._check_sizes(prefix)

        self.imgs_rgb = [None] * n      # cache_images: the decoded originals, HWC RGB uint8 CUDA tensors
        self.imgs_ir = [None] * n
        self.labels = self.labels_rgb
        self.shapes = self.shapes_rgb
        self.indices = self.indices_rgb

    def _check_sizes(self, prefix=''):
        """The INTER_AREA resize of cft_pair_batch_u8 reduces by at most CFT_PAIR_MAX_REDUCTION per axis: say so before any work."""
        for index, f in enumerate(self.img_files_rgb):
            h0, w0 = self.original_size(index)
            h, w = self.resized_size(h0, w0)
            if h * PAIR_MAX_REDUCTION < h0 or w * PAIR_MAX_REDUCTION < w0:
                raise ValueError(f'{prefix}{f} is {w0}x{h0}: img_size={self.img_size} would reduce it by more than {PAIR_MAX_REDUCTION}x per axis, '
                                 f'which cft_pair_batch_u8 does not do; use a larger img_size (about {-(-max(h0, w0) // PAIR_MAX_REDUCTION)} or more) or smaller images')

    def __len__(self):
        return len(self.img_files_rgb)

    def original_size(self, index):
        """(h0, w0) of pair ``index`` as scanned."""
        w0, h0 = (int(v) for v in self.shapes_rgb[index])
        return h0, w0

    def resized_size(self, h0, w0):
        """(h, w) of load_image_rgb_ir (:1361-1367)."""
        r = self.img_size / max(h0, w0)  # ratio
        return (int(h0 * r), int(w0 * r)) if r != 1 else (h0, w0)

    def letterbox_shape(self, index):
        """The final letterboxed shape of pair ``index``: its batch's rect shape, or ``img_size``."""
        return self.batch_shapes_rgb[self.batch_rgb[index]] if self.rect else self.img_size

    def _letterbox(self, index, scaleup):
        """The resize of load_image_rgb_ir followed by ``letterbox(auto=False, scaleup=scaleup)``:
        ``(h0, w0, h, w, top, left, (H, W), ratio, pad, new_unpad)``."""
        h0, w0 = self.original_size(index)
        h, w = self.resized_size(h0, w0)
        new_unpad, ratio, pad, (top, bottom, left, right) = letterbox_geometry((h, w), self.letterbox_shape(index), auto=False, scaleup=scaleup)
        return h0, w0, h, w, top, left, (new_unpad[1] + top + bottom, new_unpad[0] + left + right), ratio, pad, new_unpad

    def pair_geometry(self, index):
        """Where pair ``index`` lands in its batch: ``(h0, w0, h, w, top, left, mode, (H, W), ratio, pad)`` - the size arithmetic of
        load_image_rgb_ir (:1361-1367) and of ``letterbox(auto=False, scaleup=False)`` (:1205-1207).  ``ratio`` is the letterbox's own:
        (1, 1) for every shape this class builds, and then ``(h, w)`` is what lands at ``(top, left)``; ``build_descriptors`` checks it."""
        h0, w0, h, w, top, left, HW, ratio, pad, _ = self._letterbox(index, scaleup=False)
        r = self.img_size / max(h0, w0)  # ratio
        mode = PAIR_COPY if r == 1 else (PAIR_AREA if r < 1 else PAIR_LINEAR)
        return h0, w0, h, w, top, left, mode, HW, ratio, pad

    def _letterboxed_labels(self, index, h0, w0, h, w, ratio, pad):
        """``(labels [nL, 5] float32 in pixel xyxy, shapes)`` of a pair that is letterboxed on its own (:1209-1213)."""
        labels = self.labels_rgb[index].copy()
        if labels.size:  # normalized xywh to pixel xyxy format
            labels[:, 1:] = xywhn2xyxy(labels[:, 1:], ratio[0] * w, ratio[1] * h, padw=pad[0], padh=pad[1])
        return labels, ((h0, w0), ((h / h0, w / w0), pad))  # for COCO mAP rescaling

    def item_targets(self, index):
        """``(labels_out [nL, 6] float32 with column 0 zero, shapes)`` of ``__getitem__`` (:1209-1213, :1243-1247, :1266-1268)."""
        h0, w0, h, w, top, left, mode, (H, W), ratio, pad = self.pair_geometry(index)
        labels, shapes = self._letterboxed_labels(index, h0, w0, h, w, ratio, pad)
        return _labels_out(labels, H, W), shapes

    def _collate(self, label, indices, shapes):
        """The reference's ``collate_fn`` (:1284-1288) on the ``labels_out`` of the pairs ``indices``: ``(targets, paths, shapes)``."""
        for i, l in enumerate(label):
            l[:, 0] = i  # add target image index for build_targets()
        return torch.cat(label, 0), tuple(self.img_files_rgb[i] for i in indices), tuple(shapes)

    def batch_targets(self, indices):
        """``(targets [nt, 6] float32 CPU, paths, shapes)`` of one batch: ``item_targets`` + the reference's ``collate_fn``."""
        label, shapes = zip(*(self.item_targets(i) for i in indices))
        return self._collate(label, indices, shapes)

    def build_descriptors(self, indices, flip=0):
        """The table of cft_pair_batch_u8 for one batch, source pointers and strides left zero: ``(PAIR_DESC array [B], (H, W))``.
        Raises LetterboxResizes if the letterbox would resize a pair again (never, for the shapes this class builds)."""
        desc = np.zeros(len(indices), dtype=PAIR_DESC)
        HW = None
        for row, index in zip(desc, indices):
            h0, w0, h, w, top, left, mode, hw, ratio, _ = self.pair_geometry(index)
            if ratio != (1.0, 1.0):
                raise LetterboxResizes(f"pair {index}: the letterbox would resize {w}x{h} again (ratio {ratio}); cft_pair_batch_u8 has one resize stage")
            if HW is not None and hw != HW:
                raise AssertionError(f"pair {index}: letterbox {hw} differs from its batch's {HW}")
            HW = hw
            _fill_geometry(row, h0, w0, h, w, top, left, mode, flip)
        return desc, HW

    def load_pair(self, index):
        """The decoded originals of one pair, HWC RGB uint8 numpy arrays; checks them against the scanned shape."""
        h0, w0 = self.original_size(index)
        return _decode_checked(self.img_files_rgb[index], h0, w0), _decode_checked(self.img_files_ir[index], h0, w0)


def _labels_out(labels, H, W, flipud=False, fliplr=False):
    """The tail of ``__getitem__`` (:1243-1268): pixel xyxy labels [nL, 5] float32 (changed in place) to xywh normalised by the batch's
    ``(H, W)``, the two label flips, and ``labels_out`` [nL, 6] float32 with column 0 zero."""
    nL = len(labels)  # number of labels
    if nL:
        labels[:, 1:5] = xyxy2xywh(labels[:, 1:5])  # convert xyxy to xywh
        labels[:, [2, 4]] /= H  # normalized height 0-1
        labels[:, [1, 3]] /= W  # normalized width 0-1
        if flipud:
            labels[:, 2] = 1 - labels[:, 2]
        if fliplr:
            labels[:, 1] = 1 - labels[:, 1]
    labels_out = torch.zeros((nL, 6))
    if nL:
        labels_out[:, 1:] = torch.from_numpy(labels)
    return labels_out


def _decode_checked(path, h0, w0):
    """``decode_image`` of a file whose header said ``w0`` x ``h0`` when it was scanned."""
    im = decode_image(path)
    if im.shape != (h0, w0, 3):
        raise ValueError(f'{path}: decoded to {im.shape[1]}x{im.shape[0]}, scanned as {w0}x{h0}')
    return im


def _fill_geometry(row, h0, w0, h, w, top, left, mode, flip):
    """The geometry fields of one PAIR_DESC row: ``h0 x w0`` resized to ``h x w`` by ``mode``, landing at ``(top, left)``."""
    row["h0"], row["w0"], row["h"], row["w"], row["top"], row["left"], row["mode"], row["flip"] = h0, w0, h, w, top, left, mode, flip


def _fill_source(row, rgb, ir, h0, w0):
    """Source pointers and row strides of one table row or tile, after checking the pair against the size the table states."""
    for t in (rgb, ir):
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.stride(2) != 1 or t.stride(1) != 3 or not t.is_cuda:
            raise ValueError("pair sources must be HWC uint8 CUDA tensors with contiguous pixels")
        if tuple(t.shape[:2]) != (h0, w0):
            raise ValueError(f"pair source is {tuple(t.shape[:2])}, the table says {(h0, w0)}")
    row["src_rgb"], row["src_ir"], row["stride_rgb"], row["stride_ir"] = rgb.data_ptr(), ir.data_ptr(), rgb.stride(0), ir.stride(0)


def _launch_direct(launch, out, table, luts=None):
    """The launch of the direct forms: the host table (and look-up tables) pinned, copied to ``out``'s device without blocking on the
    current stream, then ``launch(table_dev, table_host, [luts_dev,] out)``."""
    def upload(a):
        host = torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
        return host, host.to(out.device, non_blocking=True)
    host, dev = upload(np.ascontiguousarray(table).view(np.uint8).reshape(len(table), -1))
    launch(dev, host, *(() if luts is None else (upload(luts)[1],)), out)
    return out


def pair_batch(desc, out, color=114):
    """Launch cft_pair_batch_u8: ``desc`` is a filled PAIR_DESC array (host), ``out`` the uint8 CUDA [B, 6, H, W] batch to write.
    The device copy of the table is made on the current stream."""
    from ..ops import pair_batch_u8
    return _launch_direct(lambda dev, host, out: pair_batch_u8(dev, host, out, color), out, desc)


def assemble_batch(dataset, indices, device, sources=None):
    """One batch assembled directly: decode (or take ``sources``, a list of (rgb, ir) HWC RGB uint8 CUDA tensors), upload, one launch.
    Returns the uint8 [B, 6, H, W] CUDA tensor.  The loader below does the same with staging buffers and prefetch."""
    if sources is None:
        sources = [tuple(torch.from_numpy(a).to(device) for a in dataset.load_pair(i)) for i in indices]
    try:
        desc, (H, W) = dataset.build_descriptors(indices)
    except LetterboxResizes:
        return assemble_batch_by_pair(dataset, indices, sources)
    _fill_sources(desc, sources)
    out = torch.empty((len(indices), 6, H, W), dtype=torch.uint8, device=device)
    return pair_batch(desc, out)


def assemble_batch_by_pair(dataset, indices, sources):
    """A batch whose letterbox resizes again, pair by pair as the reference does it: the load_image_rgb_ir resize alone (one
    cft_pair_batch_u8 launch per pair, no border), then the existing ``letterbox_pair`` (two cft_letterbox_u8 launches) into the pair's
    block of the batch.  ``sources``: (rgb, ir) HWC RGB uint8 CUDA tensors.  Runs on the current stream."""
    out = None
    for k, (index, pair) in enumerate(zip(indices, sources)):
        h0, w0, h, w, _, _, mode, (H, W), _, _ = dataset.pair_geometry(index)
        desc = np.zeros(1, dtype=PAIR_DESC)
        _fill_geometry(desc[0], h0, w0, h, w, 0, 0, mode, flip=1)   # RGB in, BGR planes out
        _fill_sources(desc, [pair])
        w4 = (w + 3) & ~3                                           # the kernel writes whole dwords of a row
        chw = pair_batch(desc, torch.empty((1, 6, h, w4), dtype=torch.uint8, device=pair[0].device))[0, :, :, :w]
        bgr, ir = chw[:3].permute(1, 2, 0).contiguous(), chw[3:].permute(1, 2, 0).contiguous()      # HWC BGR, what letterbox_pair takes
        if out is None:
            out = torch.empty((len(indices), 6, H, W), dtype=torch.uint8, device=pair[0].device)
        shape = dataset.letterbox_shape(index)
        letterbox_pair(bgr, ir, tuple(int(v) for v in shape) if dataset.rect else shape, auto=False, scaleup=False, out=out[k])
    return out


def _fill_sources(desc, sources):
    for row, (rgb, ir) in zip(desc, sources):
        _fill_source(row, rgb, ir, int(row["h0"]), int(row["w0"]))


# ------------------------------------------------------------------------------ the prefetch pipeline of the three loaders
# PairLoader, AugmentedPairLoader and LoadImagePairs differ in what a batch is and in the kernel that assembles it; how a batch gets to
# the device is one thing, stated here.  While batch k is assembled and used, batch k + 1 is staged: its files are decoded on a pool
# of threads into pinned memory that is reused (``_upload``), and uploaded with its table on a side stream.  Two events per slot order
# the two streams: ``ready``, recorded on the side stream after the uploads, is what the consumer stream waits on before the batch's
# launch; ``consumed``, recorded on the consumer stream after that launch, is what the side stream waits on before it rewrites the
# slot two batches later - the consumer stream may be many batches behind the host.
class _Slot:
    """One of the pipeline's two staging sets: pinned host bytes, their device copy, the table, and the two events that order them."""

    def __init__(self, row_bytes):
        self.row_bytes = row_bytes                 # bytes of table per batch row
        self.pinned = self.staged = self.desc_host = self.desc_dev = None
        self.jpinned = self.jstaged = None      # decode = 'device': table + coefficients + tables (pinned), the same + planes (device)
        self.ready = self.consumed = None       # upload finished (side stream) / batch assembled (consumer stream)

    def reserve(self, nbytes, nrows, device):
        if self.ready is not None:
            self.ready.synchronize()             # the previous upload out of these pinned bytes has finished
        if nbytes and (self.pinned is None or self.pinned.numel() < nbytes):
            self.pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            self.staged = torch.empty(nbytes, dtype=torch.uint8, device=device)
        if self.desc_host is None or self.desc_host.shape[0] < nrows:
            self.desc_host = torch.empty((nrows, self.row_bytes), dtype=torch.uint8).pin_memory()
            self.desc_dev = torch.empty((nrows, self.row_bytes), dtype=torch.uint8, device=device)

    def reserve_jpeg(self, upload_bytes, device_bytes, device):
        """After ``reserve`` (which has waited for the previous upload): room for ``upload_bytes`` of pinned JPEG staging and
        ``device_bytes`` >= that on the device (the upload, then the plane workspace)."""
        if self.jpinned is None or self.jpinned.numel() < upload_bytes:
            self.jpinned = torch.empty(upload_bytes, dtype=torch.uint8).pin_memory()
        if self.jstaged is None or self.jstaged.numel() < device_bytes:
            self.jstaged = torch.empty(device_bytes, dtype=torch.uint8, device=device)

    def upload_table(self, n, *parts):
        """The host arrays ``parts``, one after the other, as the ``n`` rows of the table: written into the pinned copy and uploaded
        without blocking (current = side stream)."""
        host, at = self.desc_host[:n].view(-1).numpy(), 0
        for part in parts:
            raw = part.view(np.uint8).reshape(-1)
            host[at:at + raw.size] = raw
            at += raw.size
        self.desc_dev[:n].copy_(self.desc_host[:n], non_blocking=True)


class _Prefetch:
    """The pipeline itself: the decode pool and the one-thread stager, the side stream, the two slots and the event protocol above.
    ``run(batches, stage, assemble)`` yields ``(item, assemble(slot, item))`` per batch, where ``stage(batch, slot, pool)``, called on
    the stager thread with the side stream current, fills the slot and returns ``(staged, item)``: the device buffer its originals
    were uploaded to (None if there was no upload) and whatever ``assemble``, called on the consumer's thread and stream, needs."""

    def __init__(self, device, workers, row_bytes=PAIR_DESC.itemsize):
        self.device, self.workers = device, workers
        self.side = None
        self.slots = (_Slot(row_bytes), _Slot(row_bytes))

    def run(self, batches, stage, assemble):
        from concurrent.futures import ThreadPoolExecutor
        if self.side is None:
            self.side = torch.cuda.Stream(self.device)
        batches = list(batches)

        def staged_on_side(k, pool):
            slot = self.slots[k % 2]
            with torch.cuda.device(self.device), torch.cuda.stream(self.side):
                # Whatever this does to the slot - the table always, the staging buffer when it is reused - comes after the launch that
                # read the slot two batches ago.
                if slot.consumed is not None:
                    self.side.wait_event(slot.consumed)
                staged = stage(batches[k], slot, pool)
                slot.ready = torch.cuda.Event()
                slot.ready.record(self.side)
            return staged

        with ThreadPoolExecutor(self.workers) as pool, ThreadPoolExecutor(1) as stager:
            nxt = stager.submit(staged_on_side, 0, pool) if batches else None
            for k in range(len(batches)):
                staged, item = nxt.result()
                slot = self.slots[k % 2]
                # the next batch decodes and uploads while this one is assembled and used
                nxt = stager.submit(staged_on_side, k + 1, pool) if k + 1 < len(batches) else None
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(slot.ready)
                out = assemble(slot, item)
                slot.consumed = torch.cuda.Event()
                slot.consumed.record(cur)
                slot.desc_dev.record_stream(cur)                 # allocated on the side stream, read on this one
                if staged is not None:
                    staged.record_stream(cur)
                yield item, out


def _upload(entries, nrows, slot, pool, device, decode='pil', jpeg_infos=None, own_buffer=False):
    """The files ``entries``, ``(path, (h0, w0) as scanned)`` each, as HWC RGB uint8 CUDA tensors: laid out one after the other, 16-byte
    aligned, decoded on the pool and uploaded without blocking (current = side stream) into the slot's device buffer, or with
    ``own_buffer`` into one allocated here, for originals that outlive the batch.  Each pool worker picks its file's decoder.  With
    ``decode == 'device'`` a file the device decoder takes (``jpeg_infos`` remembers the verdict per path) is Huffman-decoded straight
    into the slot's pinned JPEG staging - table rows, then per file coefficients and quantisation tables - which one copy uploads and
    one cft_jpeg_decode_u8 call turns into pixels: those originals never exist on the host.  Every other file goes through PIL into
    the pinned image staging, one copy; where no file qualifies there is no JPEG staging.  Also sizes the slot's table for ``nrows``.
    Returns ``(staged, views, decoded)``: the device buffer (None without entries), and per entry its tensor and PIL's array (None
    for a file decoded on the device)."""
    from . import jpeg as J
    sizes = [h0 * w0 * 3 for _, (h0, w0) in entries]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + _align16(n))
    total = offs.pop()
    slot.reserve(total, nrows, device)
    if not entries:
        return None, [], []
    probed = [(None, None)] * len(entries)                       # (bytes or None, info or None) per file; the header is parsed once per file
    if decode == 'device':
        for k, (f, (h0, w0)) in enumerate(entries):
            if f in jpeg_infos:
                probed[k] = (None, jpeg_infos[f])
            else:
                probed[k] = _probe_jpeg(f)
                jpeg_infos[f] = probed[k][1]
            info = probed[k][1]
            if info is not None and (int(info["height"]), int(info["width"])) != (h0, w0):
                raise ValueError(f'{f}: decodes to {int(info["width"])}x{int(info["height"])}, scanned as {w0}x{h0}')
    infos = [info for _, info in probed]
    plan = jhost = None
    if any(info is not None for info in infos):
        plan = J.decode_plan(infos, reserve=len(entries) * J.JPEG_DESC.itemsize)   # the table rows lead the JPEG upload
        slot.reserve_jpeg(plan.upload_bytes, plan.upload_bytes + plan.plane_total, device)
        jhost = slot.jpinned.numpy()
    staged = torch.empty(total, dtype=torch.uint8, device=device) if own_buffer else slot.staged
    host = slot.pinned.numpy()

    def work(k):
        """None: file k's coefficients are in the JPEG staging; else its PIL decode, which is in the image staging."""
        (f, (h0, w0)), (blob, info) = entries[k], probed[k]
        if info is not None:
            if blob is None:
                with open(f, 'rb') as fh:
                    blob = fh.read()
            if J.entropy_staged(blob, info, jhost, plan, k):
                return None
        im = _decode_checked(f, h0, w0)
        host[offs[k]:offs[k] + im.nbytes] = im.reshape(-1)
        return im

    # two files a task: with one the PNG-bound loaders measured 8 - 12 % slower (profiles/loader_pipeline.md)
    tasks = pool.map(lambda k: [work(j) for j in range(k, min(k + 2, len(entries)))], range(0, len(entries), 2))
    decoded = [im for ims in tasks for im in ims]
    live = [k for k, im in enumerate(decoded) if im is None]
    by_pil = [k for k, im in enumerate(decoded) if im is not None]
    if by_pil:
        lo, hi = offs[by_pil[0]], offs[by_pil[-1]] + sizes[by_pil[-1]]
        staged[lo:hi].copy_(slot.pinned[lo:hi], non_blocking=True)
    if live:
        table = np.zeros(len(live), dtype=J.JPEG_DESC)
        J.fill_decode_rows(table, plan, infos, live, slot.jstaged.data_ptr(), [(staged.data_ptr() + offs[k], 3 * entries[k][1][1]) for k in live])
        nb, jtotal = len(live) * J.JPEG_DESC.itemsize, plan.upload_bytes
        jhost[:nb] = table.view(np.uint8).reshape(-1)
        slot.jstaged[:jtotal].copy_(slot.jpinned[:jtotal], non_blocking=True)
        J.jpeg_decode_u8(slot.jstaged[:nb], slot.jpinned[:nb], len(live), slot.jstaged[jtotal:jtotal + plan.plane_total])
    views = [staged[o:o + n].view(h0, w0, 3) for o, n, (_, (h0, w0)) in zip(offs, sizes, entries)]
    return staged, views, decoded


class PairLoader:
    """The iterable ``create_dataloader_rgb_ir`` returns: yields ``(img6 uint8 cuda [B, 6, H, W], targets float32 CPU [nt, 6], paths,
    shapes)`` per batch, in dataset order.  Batches come through the prefetch pipeline above (``_Prefetch``: decode pool of ``workers``
    threads, reused pinned staging, side stream, the ``ready`` / ``consumed`` events - cached batches included, they reuse the table);
    what is stated here is the batch's table and its single cft_pair_batch_u8 launch.  With ``dataset.decode == 'device'``
    (``use_device_jpeg``) the pool only Huffman-decodes the JPEG files and their pixels are made on the side stream (``_upload``)."""
    ROW_BYTES = PAIR_DESC.itemsize                 # bytes of the slots' table per batch row

    def __init__(self, dataset, batch_size, workers=8, rank=-1, world_size=1, device=None):
        self.dataset = dataset
        self.batch_size = max(1, min(batch_size, len(dataset)))
        self.workers = max(1, min(int(workers), MAX_DECODE_THREADS))
        nb = (len(dataset) + self.batch_size - 1) // self.batch_size
        if rank >= 0:
            from ..distributed import shard_bounds
            self.batch_range = range(*shard_bounds(nb, rank, world_size))
        else:
            self.batch_range = range(nb)
        self.device = torch.device(device if device is not None else "cuda")
        self._pipe = _Prefetch(self.device, self.workers, self.ROW_BYTES)

    def __len__(self):
        return len(self.batch_range)

    def batch_indices(self, b):
        return list(range(b * self.batch_size, min((b + 1) * self.batch_size, len(self.dataset))))

    def _originals(self, indices, nrows, slot, pool):
        """The originals of the pairs ``indices`` (distinct) as HWC RGB uint8 CUDA tensors, ``{index: (rgb, ir)}``: cached ones as they
        are, the others through ``_upload``, RGB then IR per pair - with ``cache_images`` into a buffer of their own, since they stay.
        Returns ``(staged, by_index)``, ``staged`` the device buffer of this upload or None."""
        ds = self.dataset
        by_index = {i: (ds.imgs_rgb[i], ds.imgs_ir[i]) for i in indices if ds.imgs_rgb[i] is not None}
        missing = [i for i in indices if i not in by_index]
        entries = [(files[i], ds.original_size(i)) for i in missing for files in (ds.img_files_rgb, ds.img_files_ir)]
        staged, views, _ = _upload(entries, nrows, slot, pool, self.device, ds.decode, ds.jpeg_infos, own_buffer=ds.cache_images)
        for n, i in enumerate(missing):
            by_index[i] = views[2 * n], views[2 * n + 1]
            if ds.cache_images:
                ds.imgs_rgb[i], ds.imgs_ir[i] = by_index[i]
        return staged, by_index

    def _stage(self, b, slot, pool):
        """Decode and upload batch ``b`` (side stream); returns the upload's buffer and what ``_assemble`` needs."""
        ds, indices = self.dataset, self.batch_indices(b)
        try:
            desc, HW = ds.build_descriptors(indices)
        except LetterboxResizes:                         # assembled pair by pair (assemble_batch_by_pair): only the sizes are checked here
            desc, HW = np.zeros(len(indices), dtype=PAIR_DESC), None
            for row, index in zip(desc, indices):
                _fill_geometry(row, *ds.pair_geometry(index)[:7], flip=0)
        staged, by_index = self._originals(indices, len(indices), slot, pool)
        sources = [by_index[i] for i in indices]
        _fill_sources(desc, sources)
        slot.upload_table(len(indices), desc)
        return staged, (indices, HW, sources)

    def _assemble(self, slot, item):
        from ..ops import pair_batch_u8
        indices, HW, sources = item
        if HW is None:                                   # the letterbox resizes again: the per-image path
            return assemble_batch_by_pair(self.dataset, indices, sources)
        out = torch.empty((len(indices), 6, HW[0], HW[1]), dtype=torch.uint8, device=self.device)
        pair_batch_u8(slot.desc_dev[:len(indices)], slot.desc_host[:len(indices)], out, 114)
        return out

    def __iter__(self):
        for (indices, _, _), img in self._pipe.run(self.batch_range, self._stage, self._assemble):
            yield (img, *self.dataset.batch_targets(indices))


def _align16(n):
    return (n + 15) & ~15


def create_dataloader_rgb_ir(path1, path2, imgsz, batch_size, stride, opt, hyp=None, augment=False, cache=False, pad=0.0, rect=False,
                             rank=-1, world_size=1, workers=8, image_weights=False, quad=False, prefix=''):
    """The reference's ``create_dataloader_rgb_ir`` (utils/datasets.py:223-257) for the non-augmented form: returns ``(loader, dataset)``.
    ``opt`` is read for ``single_cls`` only; the loader is a ``PairLoader`` (a plain iterable with ``__len__``), and with ``rank >= 0``
    it yields that rank's contiguous range of batches (``distributed.shard_bounds``)."""
    if quad:
        raise NotImplementedError("create_dataloader_rgb_ir: quad=True (collate_fn4) belongs to augmented training and is not implemented")
    dataset = LoadMultiModalImagesAndLabels(path1, path2, imgsz, batch_size,
                                            augment=augment,  # augment images
                                            hyp=hyp,  # augmentation hyperparameters
                                            rect=rect,  # rectangular training
                                            cache_images=cache,
                                            single_cls=opt.single_cls,
                                            stride=int(stride),
                                            pad=pad,
                                            image_weights=image_weights,
                                            prefix=prefix)
    return PairLoader(dataset, batch_size, workers=workers, rank=rank, world_size=world_size), dataset


# ------------------------------------------------------------------------------ paired RGB + IR dataset, augmented training form
# The form the reference trains on (train.py:623-626: create_dataloader_rgb_ir(..., augment=True)): per item the mosaic of four pairs
# or the letterbox, the affine warp, HSV per stream and the flips (utils/datasets.py:1155-1281).  The host draws the random numbers
# in the reference's order, computes the labels in numpy and writes one table row per output image; everything between the decoded
# originals and the uint8 [B,6,H,W] batch is ONE launch of cft_augment_batch_u8 per batch (csrc/augment.hip).  It arrives under new
# names: LoadMultiModalImagesAndLabels(augment=True) and create_dataloader_rgb_ir(quad=True) keep their refusals.
AUG_TILE = np.dtype([("src_rgb", "<u8"), ("src_ir", "<u8"), ("stride_rgb", "<i8"), ("stride_ir", "<i8"), ("h0", "<i4"), ("w0", "<i4"),
                     ("h", "<i4"), ("w", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("padw", "<i4"), ("padh", "<i4"),
                     ("reserved", "<i4", (2,))])
# one row of the table cft_augment_batch_u8 reads: cft_aug_desc_t of include/cft_hip.h
AUG_DESC = np.dtype([("ntiles", "<i4"), ("warp", "<i4"), ("canvas_h", "<i4"), ("canvas_w", "<i4"), ("flip", "<i4"), ("reserved", "<i4", (3,)),
                     ("inv", "<f8", (6,)), ("tile", AUG_TILE, (4,))])
assert AUG_TILE.itemsize == _lib._consts["CFT_AUG_TILE_BYTES"] and AUG_DESC.itemsize == _lib._consts["CFT_AUG_DESC_BYTES"]
AUG_FLIPLR, AUG_FLIPUD = _lib._consts["CFT_AUG_FLIPLR"], _lib._consts["CFT_AUG_FLIPUD"]
AUG_LUT_BYTES = 2 * 3 * 256          # per output image: stream (RGB, IR) x (hue, saturation, value) x 256
AUG_HYP_KEYS = ('mosaic', 'degrees', 'translate', 'scale', 'shear', 'perspective', 'hsv_h', 'hsv_s', 'hsv_v', 'flipud', 'fliplr')


def box_candidates(box1, box2, wh_thr=2, ar_thr=20, area_thr=0.1, eps=1e-16):
    """Which boxes survive an augmentation, box1 [4, n] before and box2 [4, n] after (reference utils/datasets.py:1917-1922)."""
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))  # aspect ratio
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) > area_thr) & (ar < ar_thr)


def mosaic_tile_rects(i, xc, yc, w, h, s):
    """Where tile ``i`` (0 top left, 1 top right, 2 bottom left, 3 bottom right) of resized size (h, w) lands in the 2s x 2s canvas
    around the centre (xc, yc): ``(x1, y1, x2, y2, padw, padh)``, the arithmetic of load_mosaic_RGB_IR (:1504-1526)."""
    if i == 0:
        x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
        x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
    elif i == 1:
        x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
        x1b, y1b = 0, h - (y2a - y1a)
    elif i == 2:
        x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
        x1b, y1b = w - (x2a - x1a), 0
    else:
        x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
        x1b, y1b = 0, 0
    return x1a, y1a, x2a, y2a, x1a - x1b, y1a - y1b


def invert_affine(M):
    """The inverse of ``M[:2]`` in double by cv2.warpAffine's closed form, ``(a00, a01, a02, a10, a11, a12)``: what the table carries."""
    m00, m01, m02, m10, m11, m12 = (float(v) for v in np.asarray(M, dtype=np.float64)[:2].reshape(-1))
    D = m00 * m11 - m01 * m10
    D = 1.0 / D if D != 0 else 0.0
    a00, a11 = m11 * D, m00 * D
    a01, a10 = m01 * -D, m10 * -D
    return a00, a01, -a00 * m02 - a01 * m12, a10, a11, -a10 * m02 - a11 * m12


def hsv_luts(gains):
    """The three 256-entry tables of augment_hsv (:1379-1382) for ``gains`` = ``uniform(-1, 1, 3) * [h, s, v] + 1``: uint8 [3, 256]."""
    x = np.arange(0, 256, dtype=np.int16)
    return np.stack([((x * gains[0]) % 180).astype(np.uint8), np.clip(x * gains[1], 0, 255).astype(np.uint8), np.clip(x * gains[2], 0, 255).astype(np.uint8)])


class LoadMultiModalImagesAndLabelsAugmented(LoadMultiModalImagesAndLabels):
    """The reference's paired dataset with ``augment=True``: mosaic (``not rect``), affine warp, HSV per stream, flips.  Same constructor
    with ``hyp`` required; the scan, the rect sort and batch shapes, ``labels`` / ``shapes`` / ``n`` / ``indices*`` and ``cache_images`` are
    the base class's.  An item is not an array here but a plan (``item_plan``): random draws, tile geometry, labels; the pixels of a
    whole batch come from one cft_augment_batch_u8 launch (``assemble_augmented_batch``, ``AugmentedPairLoader``).
    Refused: ``image_weights``, ``hyp['perspective'] != 0`` (cv2.warpPerspective), and - where the non-mosaic branch can be reached -
    a pair whose letterbox would resize a second time."""

    def __init__(self, path_rgb, path_ir, img_size=640, batch_size=16, augment=True, hyp=None, rect=False, image_weights=False,
                 cache_images=False, single_cls=False, stride=32, pad=0.0, prefix=''):
        if not augment:
            raise ValueError("LoadMultiModalImagesAndLabelsAugmented is the augment=True form; LoadMultiModalImagesAndLabels is the other")
        if hyp is None:
            raise ValueError("LoadMultiModalImagesAndLabelsAugmented: hyp (the augmentation hyper-parameters) is required")
        for k in AUG_HYP_KEYS:
            if k not in hyp:
                raise ValueError(f"LoadMultiModalImagesAndLabelsAugmented: hyper-parameter '{k}' is missing from hyp")
        if image_weights:
            raise NotImplementedError("LoadMultiModalImagesAndLabelsAugmented: image_weights=True (weighted index sampling) is not implemented")
        if hyp['perspective'] != 0:
            raise NotImplementedError(f"LoadMultiModalImagesAndLabelsAugmented: hyp['perspective'] = {hyp['perspective']} needs cv2.warpPerspective; "
                                      "cft_augment_batch_u8 warps with the affine form only (perspective = 0)")
        super().__init__(path_rgb, path_ir, img_size, batch_size, augment=False, hyp=hyp, rect=rect, image_weights=False,
                         cache_images=cache_images, single_cls=single_cls, stride=stride, pad=pad, prefix=prefix)
        self.augment = True
        self.mosaic = not self.rect
        self.mosaic_border = [-img_size // 2, -img_size // 2]
        if self.rect or hyp['mosaic'] < 1:      # the non-mosaic branch can be reached: every pair must be one tile of its letterbox
            for index, f in enumerate(self.img_files_rgb):
                h0, w0, h, w, top, left, (H, W), ratio, pad_, new_unpad = self.letterbox_geometry_aug(index)
                if new_unpad != (w, h):
                    raise ValueError(f'{prefix}{f} ({w0}x{h0}) is resized to {w}x{h} and its letterbox to {W}x{H} would resize it a second time, to '
                                     f'{new_unpad[0]}x{new_unpad[1]}: cft_augment_batch_u8 has one resize stage per tile (use mosaic = 1.0 without rect, or another img_size)')

    def _check_sizes(self, prefix=''):
        """load_image_rgb_ir resizes with INTER_LINEAR in both directions when augmenting: any ratio up to the kernel's size limit."""
        limit = _lib._consts["CFT_AUG_MAX_SIDE"]
        for index, f in enumerate(self.img_files_rgb):
            h0, w0 = self.original_size(index)
            if max(h0, w0, 2 * self.img_size) > limit or min(self.resized_size(h0, w0)) < 1:
                raise ValueError(f'{prefix}{f} is {w0}x{h0}: img_size={self.img_size} is outside what cft_augment_batch_u8 takes (sides of 1..{limit})')

    def letterbox_geometry_aug(self, index):
        """The non-mosaic branch's geometry (:1202-1209, letterbox(auto=False, scaleup=True)):
        ``(h0, w0, h, w, top, left, (H, W), ratio, pad, new_unpad)``."""
        return self._letterbox(index, scaleup=True)

    def item_plan(self, index, rng, np_rng):
        """Everything item ``index`` needs, drawing from ``rng`` (random.Random) and ``np_rng`` (numpy.random.RandomState) in exactly
        the reference's order: [mosaic decision] [yc, xc, three indices, eight warp draws] two HSV triples, flipud, fliplr.  Returns a dict:
        ``mosaic``, ``yc``/``xc``, ``indices``, ``tiles`` (dicts index, h0, w0, h, w, x1, y1, x2, y2, padw, padh), ``canvas`` (h, w),
        ``out`` (H, W), ``M`` (3x3 float64 or None), ``gains`` (two float64 triples), ``flipud``/``fliplr``, ``labels_out`` (float32
        [nL, 6], column 0 zero), ``shapes``.  Labels follow the reference's operation order: float32 label arrays, float64 M."""
        hyp, s = self.hyp, self.img_size
        plan = {"index": index, "yc": None, "xc": None, "M": None}
        mosaic = self.mosaic and rng.random() < hyp['mosaic']
        plan["mosaic"] = bool(mosaic)
        if mosaic:
            yc, xc = [int(rng.uniform(-x, 2 * s + x)) for x in self.mosaic_border]  # mosaic center x, y
            indices = [index] + rng.choices(self.indices_rgb, k=3)  # 3 additional image indices
            tiles, labels4 = [], []
            for i, k in enumerate(indices):
                h0, w0 = self.original_size(k)
                h, w = self.resized_size(h0, w0)
                x1, y1, x2, y2, padw, padh = mosaic_tile_rects(i, xc, yc, w, h, s)
                tiles.append({"index": k, "h0": h0, "w0": w0, "h": h, "w": w, "x1": x1, "y1": y1, "x2": x2, "y2": y2, "padw": padw, "padh": padh})
                labels = self.labels_rgb[k].copy()
                if labels.size:
                    labels[:, 1:] = xywhn2xyxy(labels[:, 1:], w, h, padw, padh)  # normalized xywh to pixel xyxy format
                labels4.append(labels)
            labels = np.concatenate(labels4, 0)
            np.clip(labels[:, 1:], 0, 2 * s, out=labels[:, 1:])  # clip when using random_perspective()
            M, labels = self._random_affine(labels, rng, (2 * s, 2 * s), self.mosaic_border)
            plan.update(yc=yc, xc=xc, indices=indices, tiles=tiles, canvas=(2 * s, 2 * s), out=(s, s), M=M, shapes=None)
        else:
            h0, w0, h, w, top, left, (H, W), ratio, pad, new_unpad = self.letterbox_geometry_aug(index)
            assert new_unpad == (w, h), f"pair {index}: the letterbox would resize {w}x{h} again"
            labels, shapes = self._letterboxed_labels(index, h0, w0, h, w, ratio, pad)
            plan.update(indices=[index], canvas=(H, W), out=(H, W), shapes=shapes,
                        tiles=[{"index": index, "h0": h0, "w0": w0, "h": h, "w": w, "x1": left, "y1": top, "x2": left + w, "y2": top + h, "padw": left, "padh": top}])
        # Augment colorspace: one draw of three per stream, RGB first
        gains = [np_rng.uniform(-1, 1, 3) * [hyp['hsv_h'], hyp['hsv_s'], hyp['hsv_v']] + 1 for _ in range(2)]
        flipud = rng.random() < hyp['flipud']
        fliplr = rng.random() < hyp['fliplr']
        plan.update(gains=gains, flipud=bool(flipud), fliplr=bool(fliplr), labels_out=_labels_out(labels, *plan["out"], flipud, fliplr))
        return plan

    def _random_affine(self, targets, rng, canvas, border):
        """random_perspective_rgb_ir (:1819-1914) without its image: the eight draws, ``M = T @ S @ R @ P @ C`` and the boxes warped
        through it, clipped and filtered by ``box_candidates`` (area_thr 0.10).  Returns ``(M, targets)``."""
        import math
        hyp = self.hyp
        height, width = canvas[0] + border[0] * 2, canvas[1] + border[1] * 2
        C = np.eye(3)
        C[0, 2] = -canvas[1] / 2  # x translation (pixels)
        C[1, 2] = -canvas[0] / 2  # y translation (pixels)
        P = np.eye(3)
        P[2, 0] = rng.uniform(-hyp['perspective'], hyp['perspective'])  # drawn whatever the value: 0 here
        P[2, 1] = rng.uniform(-hyp['perspective'], hyp['perspective'])
        R = np.eye(3)
        a = rng.uniform(-hyp['degrees'], hyp['degrees'])
        s = rng.uniform(1 - hyp['scale'], 1 + hyp['scale'])
        ar = a * np.pi / 180                                             # cv2.getRotationMatrix2D(angle=a, center=(0, 0), scale=s)
        alpha, beta = np.cos(ar) * s, np.sin(ar) * s
        R[:2] = [[alpha, beta, 0.0], [-beta, alpha, 0.0]]
        S = np.eye(3)
        S[0, 1] = math.tan(rng.uniform(-hyp['shear'], hyp['shear']) * math.pi / 180)  # x shear (deg)
        S[1, 0] = math.tan(rng.uniform(-hyp['shear'], hyp['shear']) * math.pi / 180)  # y shear (deg)
        T = np.eye(3)
        T[0, 2] = rng.uniform(0.5 - hyp['translate'], 0.5 + hyp['translate']) * width  # x translation (pixels)
        T[1, 2] = rng.uniform(0.5 - hyp['translate'], 0.5 + hyp['translate']) * height  # y translation (pixels)
        M = T @ S @ R @ P @ C  # order of operations (right to left) is IMPORTANT
        n = len(targets)
        if n:
            xy = np.ones((n * 4, 3))
            xy[:, :2] = targets[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)  # x1y1, x2y2, x1y2, x2y1
            xy = (xy @ M.T)[:, :2].reshape(n, 8)
            x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
            new = np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1))).reshape(4, n).T
            new[:, [0, 2]] = new[:, [0, 2]].clip(0, width)
            new[:, [1, 3]] = new[:, [1, 3]].clip(0, height)
            i = box_candidates(box1=targets[:, 1:5].T * s, box2=new.T, area_thr=0.10)
            targets = targets[i]
            targets[:, 1:5] = new[i]
        return M, targets

    def plan_targets(self, plans):
        """``(targets [nt, 6] float32 CPU, paths, shapes)`` of one planned batch: the reference's ``collate_fn`` (:1284-1288)."""
        return self._collate([p["labels_out"].clone() for p in plans], [p["index"] for p in plans], [p["shapes"] for p in plans])


def build_augment_descriptors(plans):
    """The table and the look-up tables of cft_augment_batch_u8 for one planned batch, source pointers and strides left zero:
    ``(AUG_DESC array [B], uint8 [B, 2, 3, 256], (H, W))``."""
    table = np.zeros(len(plans), dtype=AUG_DESC)
    luts = np.empty((len(plans), 2, 3, 256), dtype=np.uint8)
    HW = None
    for row, lut, p in zip(table, luts, plans):
        if HW is not None and tuple(p["out"]) != HW:
            raise AssertionError(f"item {p['index']}: output {tuple(p['out'])} differs from its batch's {HW}")
        HW = tuple(p["out"])
        row["ntiles"], row["warp"] = len(p["tiles"]), int(p["M"] is not None)
        row["canvas_h"], row["canvas_w"] = p["canvas"]
        row["flip"] = (AUG_FLIPLR if p["fliplr"] else 0) | (AUG_FLIPUD if p["flipud"] else 0)
        if p["M"] is not None:
            row["inv"] = invert_affine(p["M"])
        for tile, t in zip(row["tile"], p["tiles"]):
            for k in ("h0", "w0", "h", "w", "x1", "y1", "x2", "y2", "padw", "padh"):
                tile[k] = t[k]
        lut[0], lut[1] = hsv_luts(p["gains"][0]), hsv_luts(p["gains"][1])
    return table, luts, HW


def _fill_aug_sources(table, plans, by_index):
    """Source pointers and strides of every tile from ``by_index``: {pair index: (rgb, ir) HWC RGB uint8 CUDA tensors}."""
    for row, p in zip(table, plans):
        for tile, t in zip(row["tile"], p["tiles"]):
            _fill_source(tile, *by_index[t["index"]], t["h0"], t["w0"])


def augment_batch(table, luts, out):
    """Launch cft_augment_batch_u8: ``table`` a filled AUG_DESC array and ``luts`` uint8 [B, 2, 3, 256] (host), ``out`` the uint8 CUDA
    [B, 6, H, W] batch to write.  The device copies are made on the current stream from pinned memory."""
    from ..ops import augment_batch_u8
    return _launch_direct(augment_batch_u8, out, table, luts)


def assemble_augmented_batch(dataset, indices, device, rng, np_rng, sources=None, return_plans=False):
    """One augmented batch assembled directly: plan every item (drawing from ``rng`` / ``np_rng`` item by item, as one pass over the
    reference's dataset does), decode each distinct pair once (or take ``sources``: {pair index: (rgb, ir) HWC RGB uint8 CUDA tensors}),
    upload, one launch.  Returns the uint8 [B, 6, H, W] CUDA tensor (and the plans).  ``AugmentedPairLoader`` does the same with
    staging buffers and prefetch."""
    plans = [dataset.item_plan(i, rng, np_rng) for i in indices]
    if sources is None:
        sources = {k: tuple(torch.from_numpy(a).to(device) for a in dataset.load_pair(k)) for k in sorted({t["index"] for p in plans for t in p["tiles"]})}
    table, luts, (H, W) = build_augment_descriptors(plans)
    _fill_aug_sources(table, plans, sources)
    out = augment_batch(table, luts, torch.empty((len(plans), 6, H, W), dtype=torch.uint8, device=device))
    return (out, plans) if return_plans else out


def batch_seed(seed, epoch, batch):
    """The 64-bit seed of one batch's generators, an explicit integer mix of (seed, epoch, batch index): the three are combined with
    three odd 64-bit constants and passed through the splitmix64 finaliser, all modulo 2^64.  It depends on nothing else - not on
    which batches were planned before, on prefetch timing or on the rank that assembles the batch."""
    m = (1 << 64) - 1
    x = (0x9E3779B97F4A7C15 * (int(seed) + 1) + 0xBF58476D1CE4E5B9 * (int(epoch) + 1) + 0x94D049BB133111EB * (int(batch) + 1)) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def batch_generators(seed, epoch, batch):
    """``(random.Random, numpy.random.RandomState)`` of one batch: the first seeded with ``batch_seed``, the second with its two halves."""
    import random
    x = batch_seed(seed, epoch, batch)
    return random.Random(x), np.random.RandomState([x & 0xFFFFFFFF, x >> 32])


class AugmentedPairLoader(PairLoader):
    """The iterable ``create_train_dataloader_rgb_ir`` returns: yields ``(img6 uint8 cuda [B, 6, H, W], targets float32 CPU [nt, 6],
    paths, shapes)`` per batch in dataset order (the reference's loader does not shuffle).  Batches come through the same prefetch
    pipeline as ``PairLoader``'s (``_Prefetch``); a batch's up-to-4B distinct pairs are decoded once each, and with ``cache_images``
    only the table and the look-up tables are uploaded once the originals are on the device.  The next batch is planned on the stager
    thread, so the global ``random`` / ``np.random`` are never touched: batch ``b`` of epoch ``e`` draws from
    ``batch_generators(seed, e, b)``.  ``set_epoch(e)`` sets the epoch of the next pass; otherwise every ``__iter__`` advances it."""
    ROW_BYTES = AUG_DESC.itemsize + AUG_LUT_BYTES

    def __init__(self, dataset, batch_size, workers=8, rank=-1, world_size=1, device=None, seed=0):
        super().__init__(dataset, batch_size, workers=workers, rank=rank, world_size=world_size, device=device)
        self.seed = int(seed)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def plan_batch(self, b, epoch):
        """The plans of batch ``b`` of epoch ``epoch``: a function of (seed, epoch, b) and the dataset alone."""
        rng, np_rng = batch_generators(self.seed, epoch, b)
        return [self.dataset.item_plan(i, rng, np_rng) for i in self.batch_indices(b)]

    def _stage(self, b, slot, pool, epoch):
        """Plan, decode and upload batch ``b`` (side stream); returns the upload's buffer and what ``_assemble`` needs."""
        plans = self.plan_batch(b, epoch)
        table, luts, HW = build_augment_descriptors(plans)
        staged, by_index = self._originals(sorted({t["index"] for p in plans for t in p["tiles"]}), len(plans), slot, pool)
        _fill_aug_sources(table, plans, by_index)
        slot.upload_table(len(plans), table, luts)       # the table, then the look-up tables, in one upload
        return staged, (plans, HW)

    def _assemble(self, slot, item):
        from ..ops import augment_batch_u8
        plans, HW = item
        n, nb = len(plans), len(plans) * AUG_DESC.itemsize
        out = torch.empty((n, 6, HW[0], HW[1]), dtype=torch.uint8, device=self.device)
        dev, host = slot.desc_dev[:n].view(-1), slot.desc_host[:n].view(-1)
        augment_batch_u8(dev[:nb].view(n, -1), host[:nb].view(n, -1), dev[nb:].view(n, 2, 3, 256), out)
        return out

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        for (plans, _), img in self._pipe.run(self.batch_range, lambda b, slot, pool: self._stage(b, slot, pool, epoch), self._assemble):
            yield (img, *self.dataset.plan_targets(plans))


def create_train_dataloader_rgb_ir(path1, path2, imgsz, batch_size, stride, opt, hyp, cache=False, rect=False, rank=-1, world_size=1,
                                   workers=8, seed=0, prefix='', pad=0.0, image_weights=False, quad=False):
    """What train.py:623-626 builds with ``create_dataloader_rgb_ir(..., augment=True)``: returns ``(loader, dataset)`` with the
    loader an ``AugmentedPairLoader``.  ``opt`` is read for ``single_cls`` only; with ``rank >= 0`` the loader yields that rank's
    contiguous range of batches (``distributed.shard_bounds``)."""
    if quad:
        raise NotImplementedError("create_train_dataloader_rgb_ir: quad=True (collate_fn4) is not implemented")
    dataset = LoadMultiModalImagesAndLabelsAugmented(path1, path2, imgsz, batch_size, augment=True, hyp=hyp, rect=rect, cache_images=cache,
                                                     single_cls=opt.single_cls, stride=int(stride), pad=pad, image_weights=image_weights,
                                                     prefix=prefix)
    return AugmentedPairLoader(dataset, batch_size, workers=workers, rank=rank, world_size=world_size, seed=seed), dataset


# ------------------------------------------------------------------------------ inference loaders (detect_twostream.py)
# LoadImages of the reference (utils/datasets.py:299-376) and the zip of two of them that detect_twostream.py:66 iterates, with the
# letterbox (auto=True, scale-up allowed, :362) on the device.  Files are decoded with PIL, so the originals are RGB (cv2.imread gives
# the same pixels in BGR order); video files need cv2 and raise.
vid_formats = ['mov', 'avi', 'mp4', 'mpg', 'mpeg', 'm4v', 'wmv', 'mkv']  # acceptable video suffixes (reference :34)


def _letterbox_chw_rgb(img, out, rh, rw, top, left):
    """RGB HWC uint8 CUDA image -> the CHW RGB letterbox ``out`` [3, H, W] (cft_letterbox_u8 without the channel flip)."""
    st = _lib.load().cft_letterbox_u8(img.data_ptr(), img.shape[0], img.shape[1], img.stride(0), out.data_ptr(), out.shape[1], out.shape[2],
                                      out.stride(1), out.stride(2), out.stride(0), 0, rh, rw, top, left, 114, 114, 114, _stream())
    _lib.check(st, "cft_letterbox_u8")


def _inference_geometry(h0, w0, img_size, stride):
    """(H, W, rh, rw, top, left) of LoadImages' letterbox (reference :362: auto=True, scaleup=True)."""
    (rw, rh), _, _, (top, bottom, left, right) = letterbox_geometry((h0, w0), img_size, auto=True, scaleup=True, stride=stride)
    return rh + top + bottom, rw + left + right, rh, rw, top, left


class LoadImages:  # for inference
    """The reference's ``LoadImages`` (utils/datasets.py:299-376): a glob, a directory or one file; iterating yields
    ``(path, img, im0, None)`` with ``img`` the CHW RGB uint8 CUDA letterbox and ``im0`` the HWC RGB uint8 CUDA original."""

    def __init__(self, path, img_size=640, stride=32, device=None):
        p = str(Path(path).absolute())
        if '*' in p:
            files = sorted(glob.glob(p, recursive=True))
        elif os.path.isdir(p):
            files = sorted(glob.glob(os.path.join(p, '*.*')))
        elif os.path.isfile(p):
            files = [p]
        else:
            raise Exception(f'ERROR: {p} does not exist')

        images = [x for x in files if x.split('.')[-1].lower() in img_formats]
        videos = [x for x in files if x.split('.')[-1].lower() in vid_formats]
        if videos:
            raise NotImplementedError(f'LoadImages: video files need cv2.VideoCapture, which this package does not use ({videos[0]})')
        self.img_size = img_size
        self.stride = stride
        self.files = images
        self.nf = len(images)
        self.video_flag = [False] * self.nf
        self.mode = 'image'
        self.cap = None
        self.device = device
        assert self.nf > 0, f'No images or videos found in {p}. ' \
                            f'Supported formats are:\nimages: {img_formats}\nvideos: {vid_formats}'

    def __iter__(self):
        self.count = 0
        return self

    def __next__(self):
        if self.count == self.nf:
            raise StopIteration
        path = self.files[self.count]
        self.count += 1
        img0 = torch.from_numpy(decode_image(path)).to(torch.device(self.device if self.device is not None else "cuda"))
        H, W, rh, rw, top, left = _inference_geometry(img0.shape[0], img0.shape[1], self.img_size, self.stride)
        img = torch.empty((3, H, W), dtype=torch.uint8, device=img0.device)
        _letterbox_chw_rgb(img0, img, rh, rw, top, left)
        return path, img, img0, self.cap

    def __len__(self):
        return self.nf


def image_size(path):
    """(h0, w0) of an image file from its header, as ``decode_image`` will decode it."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


class LoadImagePairs:
    """Two ``LoadImages`` lists zipped as detect_twostream.py:66 zips them, in batches: consecutive pairs of the same original size
    (up to ``batch_size``) form one uint8 ``[B, 6, H, W]`` batch.  Iterating yields ``(paths, img6, originals, shapes)``: ``paths`` a list
    of (rgb path, ir path), ``originals`` a list of (rgb, ir) HWC RGB uint8 CUDA tensors (kept for drawing and cropping: they live in a
    device buffer of their batch's own), ``shapes`` a list of ``((h0, w0), None)`` as ``utils.metrics.geometry`` takes them;
    ``host_originals`` holds the decoded arrays of the batch just yielded.  A batch is one cft_pair_batch_u8 launch (CFT_PAIR_LINEAR, or
    CFT_PAIR_COPY at ratio 1) where that kernel's guards admit it - an enlarging letterbox - else two cft_letterbox_u8 launches per pair.
    Batches come through the prefetch pipeline of the paired loaders (``_Prefetch``), decoded by PIL on at most 16 threads."""

    def __init__(self, source1, source2, img_size=640, stride=32, batch_size=1, workers=8, device=None):
        self.rgb = LoadImages(source1, img_size, stride)
        self.ir = LoadImages(source2, img_size, stride)
        self.img_size, self.stride = img_size, stride
        self.batch_size = max(1, int(batch_size))
        self.workers = max(1, min(int(workers), MAX_DECODE_THREADS))
        self.device = torch.device(device if device is not None else "cuda")
        self.mode = 'image'
        self.pairs = list(zip(self.rgb.files, self.ir.files))       # zip stops at the shorter list, as the reference's loop does
        self.shapes = []
        for a, b in self.pairs:
            sa, sb = image_size(a), image_size(b)
            if sa != sb:
                raise ValueError(f'LoadImagePairs: {a} is {sa[1]}x{sa[0]} but {b} is {sb[1]}x{sb[0]}: a pair must have one size')
            self.shapes.append(sa)
        self.batches = []                                          # lists of consecutive pair indices of one original size
        for i, s in enumerate(self.shapes):
            if self.batches and len(self.batches[-1]) < self.batch_size and self.shapes[self.batches[-1][0]] == s:
                self.batches[-1].append(i)
            else:
                self.batches.append([i])
        self._pipe = _Prefetch(self.device, self.workers)
        self.host_originals = None

    def __len__(self):
        return len(self.batches)

    def batch_mode(self, indices):
        """(resize mode or None, (H, W, rh, rw, top, left)) of a batch: None = the per-pair letterbox path."""
        h0, w0 = self.shapes[indices[0]]
        g = _inference_geometry(h0, w0, self.img_size, self.stride)
        H, W, rh, rw = g[:4]
        if W % 4:
            return None, g
        if (rh, rw) == (h0, w0):
            return PAIR_COPY, g
        if rh >= h0 and rw >= w0:
            return PAIR_LINEAR, g
        return None, g

    def _stage(self, indices, slot, pool):
        """Decode and upload one batch (side stream), with its table where one launch assembles it."""
        entries = [(f, self.shapes[i]) for i in indices for f in self.pairs[i]]
        staged, views, decoded = _upload(entries, len(indices), slot, pool, self.device, own_buffer=True)   # the originals outlive the batch
        originals = list(zip(views[0::2], views[1::2]))
        mode, (H, W, rh, rw, top, left) = self.batch_mode(indices)
        if mode is not None:
            desc = np.zeros(len(indices), dtype=PAIR_DESC)
            for row in desc:
                _fill_geometry(row, *self.shapes[indices[0]], rh, rw, top, left, mode, flip=0)
            _fill_sources(desc, originals)
            slot.upload_table(len(indices), desc)
        return staged, (indices, originals, list(zip(decoded[0::2], decoded[1::2])))

    def _assemble(self, slot, item):
        from ..ops import pair_batch_u8
        indices, originals, _ = item
        mode, (H, W, rh, rw, top, left) = self.batch_mode(indices)
        out = torch.empty((len(indices), 6, H, W), dtype=torch.uint8, device=self.device)
        if mode is not None:
            pair_batch_u8(slot.desc_dev[:len(indices)], slot.desc_host[:len(indices)], out, 114)
        else:
            for k, (rgb, ir) in enumerate(originals):
                _letterbox_chw_rgb(rgb, out[k, :3], rh, rw, top, left)
                _letterbox_chw_rgb(ir, out[k, 3:], rh, rw, top, left)
        return out

    def __iter__(self):
        for (indices, originals, decoded), out in self._pipe.run(self.batches, self._stage, self._assemble):
            self.host_originals = decoded                    # the same pixels on the host, (rgb, ir) numpy arrays of the batch just yielded
            yield [self.pairs[i] for i in indices], out, originals, [(self.shapes[i], None) for i in indices]
