"""Post-processing that sits directly behind the forward in every reference caller
(`test.py:129`, `detect_twostream.py:86`): `non_max_suppression` of the reference's
`utils/general.py:455-543`, as ONE batched HIP kernel instead of a Python loop over images around
`torchvision.ops.nms`."""
import glob
import math
import os
import re
from pathlib import Path

import torch

from .. import _lib
from ..ops import _require_cuda, _stream

MAX_WH = 4096  # class offset in pixels (reference utils/general.py:467)
MAX_NMS = 30000  # boxes that enter the suppression at most (reference utils/general.py:469)


def _class_table(classes, nc, device):
    """uint8 [nc] allow-table for the kernel (exact for any class id, reference :505-506), None = all classes."""
    if classes is None:
        return None
    t = torch.zeros((nc,), dtype=torch.uint8)
    for c in classes:
        if 0 <= int(c) < nc:
            t[int(c)] = 1
    return t.to(device)


def batched_nms(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300,
                max_nms=MAX_NMS, class_table=None):
    """prediction [B, rows, nc+5] (fp32, on the GPU) -> (dets [B, max_det, 6] = (x1,y1,x2,y2,conf,cls),
    counts [B] int32).  ``classes`` is ALWAYS a collection of class ids, as in the reference (:505-506; a list or a tensor
    on any device: one small H2D copy); ``class_table`` instead hands over a ready-made uint8 [nc] allow-table on the
    prediction's device (1 = keep the class) - no host work at all: fit for HIP-graph capture and for all-gathering the
    <= max_det survivors instead of all rows."""
    _require_cuda(prediction, "batched_nms")
    if prediction.dtype != torch.float32 or not prediction.is_contiguous():
        prediction = prediction.float().contiguous()
    B, rows, no = prediction.shape
    nc = no - 5
    multi_label = bool(multi_label) and nc > 1            # reference :472
    cap = rows * (nc if multi_label else 1)
    scratch = torch.empty((B * ((cap + 3) // 4 * 4) * 32,), dtype=torch.uint8, device=prediction.device)
    dets = torch.empty((B, max_det, 6), dtype=torch.float32, device=prediction.device)     # cft_nms zeroes the unused rows itself
    counts = torch.empty((B,), dtype=torch.int32, device=prediction.device)                 # and always writes every count
    if class_table is not None:
        if classes is not None:
            raise ValueError("batched_nms: give either classes (ids) or class_table (allow-table), not both")
        if not (isinstance(class_table, torch.Tensor) and class_table.dtype == torch.uint8 and class_table.numel() == nc
                and class_table.device == prediction.device and class_table.is_contiguous()):
            raise ValueError(f"batched_nms: class_table must be a contiguous uint8 [{nc}] tensor on {prediction.device}")
        allow = class_table                   # the kernel indexes it by class id
    else:
        allow = _class_table(classes.tolist() if isinstance(classes, torch.Tensor) else classes, nc, prediction.device)
    st = _lib.load().cft_nms(prediction.data_ptr(), B, rows, no, float(conf_thres), float(iou_thres), int(bool(agnostic)),
                             int(multi_label), allow.data_ptr() if allow is not None else None, int(max_det), int(max_nms),
                             scratch.data_ptr(), scratch.numel(), dets.data_ptr(), counts.data_ptr(), _stream())
    _lib.check(st, "cft_nms")
    return dets, counts


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
                        labels=()):
    """Same signature and return value as the reference: a list with one (n,6) tensor [xyxy, conf, cls] per
    image, sorted by descending confidence, n <= 300."""
    if labels and any(len(l) for l in labels):
        # autolabelling (reference :480-487): a-priori labels [cls, x, y, w, h] join the image's candidates as rows
        # with obj = 1 and a one-hot class; images with fewer labels get obj = 0 padding rows (filtered in phase 1)
        B, rows, no = prediction.shape
        L = max(len(l) for l in labels)
        extra = torch.zeros((B, L, no), dtype=torch.float32, device=prediction.device)
        for xi, l in enumerate(labels):
            if len(l):
                l = torch.as_tensor(l, dtype=torch.float32, device=prediction.device)
                extra[xi, :len(l), :4] = l[:, 1:5]
                extra[xi, :len(l), 4] = 1.0
                extra[xi, torch.arange(len(l), device=prediction.device), l[:, 0].long() + 5] = 1.0
        prediction = torch.cat((prediction.float(), extra), 1)
    dets, counts = batched_nms(prediction, conf_thres, iou_thres, classes, agnostic, multi_label)
    counts = counts.tolist()
    return [dets[i, :n] for i, n in enumerate(counts)]


def xywh2xyxy(x):
    """[x, y, w, h] -> [x1, y1, x2, y2] (reference utils/general.py:386-393); tiny, used by callers on results."""
    y = x.clone()
    y[..., 0] = x[..., 0] - x[..., 2] / 2
    y[..., 1] = x[..., 1] - x[..., 3] / 2
    y[..., 2] = x[..., 0] + x[..., 2] / 2
    y[..., 3] = x[..., 1] + x[..., 3] / 2
    return y


def xyxy2xywh(x):
    """[x1, y1, x2, y2] -> [x centre, y centre, w, h] (reference utils/general.py:289-296); tiny, used by callers on results."""
    y = x.clone()
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def box_iou(box1, box2):
    """IoU matrix [N, M] of xyxy boxes box1 [N, 4] and box2 [M, 4] (reference utils/general.py:422-444), for callers working on
    results; the evaluation kernels compute their IoUs themselves."""
    area1 = (box1[:, 2] - box1[:, 0]) * (box1[:, 3] - box1[:, 1])
    area2 = (box2[:, 2] - box2[:, 0]) * (box2[:, 3] - box2[:, 1])
    inter = (torch.min(box1[:, None, 2:], box2[:, 2:]) - torch.max(box1[:, None, :2], box2[:, :2])).clamp(0).prod(2)
    return inter / (area1[:, None] + area2 - inter)


def clip_coords(boxes, img_shape):
    """Clip xyxy boxes to the image (height, width), in place (reference utils/general.py:369-374)."""
    boxes[:, 0].clamp_(0, img_shape[1])
    boxes[:, 1].clamp_(0, img_shape[0])
    boxes[:, 2].clamp_(0, img_shape[1])
    boxes[:, 3].clamp_(0, img_shape[0])


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None):
    """Map xyxy boxes from the letterboxed shape back to the original image, in place (reference utils/general.py:353-366)."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    coords[:, [0, 2]] -= pad[0]
    coords[:, [1, 3]] -= pad[1]
    coords[:, :4] /= gain
    clip_coords(coords, img0_shape)
    return coords


def increment_path(path, exist_ok=False, sep='', mkdir=False):
    """Increment file or directory path, i.e. runs/exp --> runs/exp{sep}2, runs/exp{sep}3, ... (reference utils/general.py:641-655).
    The reference searches each similar path's WHOLE string for ``stem(\\d+)``, so a parent directory that happens to contain the stem
    followed by digits (``.../e22a791/crops/a.jpg``) sets the number; here only the last path component is matched, literally."""
    path = Path(path)
    if path.exists() and not exist_ok:
        suffix, base = path.suffix, path.with_suffix('')
        pattern = re.compile(re.escape(base.stem) + re.escape(sep) + r"(\d+)")
        taken = [int(m.group(1)) for m in (pattern.match(Path(d).name) for d in glob.glob(f"{base}{sep}*")) if m]
        path = Path(f"{base}{sep}{max(taken) + 1 if taken else 2}{suffix}")
    folder = path if path.suffix == '' else path.parent
    if mkdir and not folder.exists():
        folder.mkdir(parents=True, exist_ok=True)
    return path


def crop_rectangle(xyxy, im_shape, gain=1.02, pad=10, square=False):
    """The rectangle ``save_one_box`` cuts (reference utils/general.py:630-636) for one box, float32 on the host op for op:
    (x1, y1, x2, y2) integers, the crop is rows [y1, y2) and columns [x1, x2).  ``cft_detect_boxes`` computes the same per slot."""
    xyxy = torch.tensor([float(v) for v in xyxy], dtype=torch.float32).view(-1, 4)
    b = xyxy2xywh(xyxy)
    if square:
        b[:, 2:] = b[:, 2:].max(1)[0].unsqueeze(1)
    b[:, 2:] = b[:, 2:] * gain + pad
    xyxy = xywh2xyxy(b).long()
    clip_coords(xyxy, im_shape)
    return tuple(int(v) for v in xyxy[0])


def save_one_box(xyxy, im, file='image.jpg', gain=1.02, pad=10, square=False, BGR=False, rect=None):
    """Save an image crop as {file} with crop size multiplied by {gain} and padded by {pad} pixels (reference utils/general.py:628-638).
    ``im`` is the undrawn original on the host (HWC uint8 numpy array); ``rect`` = words 8..11 of the box's slot of
    ``cft_detect_boxes`` when the caller has the kernel's output, else the reference's arithmetic runs here on the lone box.  The file
    is written with PIL, which takes RGB: ``BGR=True`` says ``im`` is in cv2's order.  Returns the path written, None for an empty crop
    (cv2.imwrite raises on one)."""
    from PIL import Image
    x1, y1, x2, y2 = (int(v) for v in rect) if rect is not None else crop_rectangle(xyxy, im.shape, gain, pad, square)
    crop = im[y1:y2, x1:x2]
    path = increment_path(Path(file).with_suffix('.jpg'), mkdir=True)       # (the reference increments before it sets the suffix: x.png would overwrite x.jpg)
    if crop.shape[0] == 0 or crop.shape[1] == 0:
        return None
    Image.fromarray(crop[..., ::-1].copy() if BGR else crop).save(str(path))
    return path


def one_cycle(y1=0.0, y2=1.0, steps=100):
    """The reference's learning-rate curve (utils/general.py:220-222): a half cosine from ``y1`` at ``x = 0`` to ``y2`` at ``x = steps``,
    as a function for ``lr_scheduler.LambdaLR`` (``train.py:572``)."""
    def curve(x):
        return ((1 - math.cos(x * math.pi / steps)) / 2) * (y2 - y1) + y1
    return curve


def save_checkpoint(path, epoch, best_fitness, model, ema, optimizer, training_results=None):
    """Write the checkpoint dictionary of ``train.py:850-858``: ``model`` and ``ema`` as half-precision copies of the (unwrapped)
    model and of ``ema.ema``, ``updates``, the optimiser's state dict, ``wandb_id`` None.  The copies carry parameters, buffers and
    attributes but no packed weights, plans or captured graphs, so a model in use can be saved.  ``compat.attempt_load`` reads it."""
    from .torch_utils import de_parallel, detached_copy
    ckpt = {'epoch': epoch,
            'best_fitness': best_fitness,
            'training_results': training_results,
            'model': detached_copy(de_parallel(model)).half(),
            'ema': detached_copy(ema.ema).half() if ema is not None else None,
            'updates': ema.updates if ema is not None else None,
            'optimizer': optimizer.state_dict() if optimizer is not None else None,
            'wandb_id': None}
    torch.save(ckpt, path)
    return ckpt


def strip_optimizer(f='best.pt', s=''):
    """Finalise a checkpoint as the reference does (utils/general.py:546-559): the EMA replaces the model, the optimiser, the
    training results, the W&B id, ``ema`` and ``updates`` become None, ``epoch`` -1, the model half precision and without grad.
    Written over ``f``, or to ``s`` if given."""
    x = torch.load(f, map_location=torch.device('cpu'), weights_only=False)
    if x.get('ema'):
        x['model'] = x['ema']
    for k in 'optimizer', 'training_results', 'wandb_id', 'ema', 'updates':
        x[k] = None
    x['epoch'] = -1
    x['model'].half()
    for p in x['model'].parameters():
        p.requires_grad = False
    torch.save(x, s or f)
    mb = os.path.getsize(s or f) / 1E6
    print(f"Optimizer stripped from {f},{(' saved as %s,' % s) if s else ''} {mb:.1f}MB")
