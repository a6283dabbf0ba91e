"""The reference's ``detect_twostream.py`` on the GPU: a folder of RGB images and a folder of IR images in, pictures with boxes,
label files and crops out.

Per batch: the forward, ``batched_nms``, ``cft_detect_boxes`` (everything the reference's per-detection loop :129-153 computes),
``cft_detect_render`` (unless ``--nosave``), then ONE device-to-host copy of the box buffer, plus one of the drawn originals when
images are saved.  The host formats strings and encodes files from those; it never touches a box on the device.  Image encoding
(PIL, at most 16 threads) is what bounds ``--save-img`` throughput; with ``--nosave --save-txt`` nothing but the box buffer leaves
the device.

The drawing is this project's raster (include/cft_hip.h, ``cft_detect_render``), not cv2's anti-aliased one.  Originals are decoded
with PIL and stay RGB; files are written with PIL.
"""
import argparse
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from .ops import detect_boxes
from .utils.datasets import LoadImagePairs, MAX_DECODE_THREADS
from .utils.general import batched_nms, increment_path, save_one_box
from .utils.jpeg import encode_jpeg_start, is_jpeg_name
from .utils.metrics import _to_device, geometry, txt_line
from .utils.plots import BoxRenderer

MAX_DET = 300          # non_max_suppression's limit (reference utils/general.py:468)


def make_parser():
    """The argparse block of detect_twostream.py:198-221 with its defaults, plus --batch-size."""
    parser = argparse.ArgumentParser()
    parser.add_argument('--weights', nargs='+', type=str, default='/home/fqy/proj/multispectral-object-detection/best.pt', help='model.pt path(s)')
    parser.add_argument('--source1', type=str, default='/home/fqy/DATA/FLIR_ADAS_1_3/align/yolo/test/rgb/', help='source')
    parser.add_argument('--source2', type=str, default='/home/fqy/DATA/FLIR_ADAS_1_3/align/yolo/test/ir', help='source')
    parser.add_argument('--img-size', type=int, default=640, help='inference size (pixels)')
    parser.add_argument('--conf-thres', type=float, default=0.4, help='object confidence threshold')
    parser.add_argument('--iou-thres', type=float, default=0.45, help='IOU threshold for NMS')
    parser.add_argument('--device', default='0', help='cuda device, i.e. 0 or 0,1,2,3 or cpu')
    parser.add_argument('--view-img', default=False, action='store_true', help='display results')
    parser.add_argument('--save-txt', action='store_true', help='save results to *.txt')
    parser.add_argument('--save-conf', action='store_true', help='save confidences in --save-txt labels')
    parser.add_argument('--save-crop', action='store_true', help='save cropped prediction boxes')
    parser.add_argument('--nosave', action='store_true', help='do not save images/videos')
    parser.add_argument('--classes', nargs='+', type=int, help='filter by class: --class 0, or --class 0 2 3')
    parser.add_argument('--agnostic-nms', action='store_true', help='class-agnostic NMS')
    parser.add_argument('--augment', action='store_true', help='augmented inference')
    parser.add_argument('--update', action='store_true', help='update all models')
    parser.add_argument('--project', default='runs/detect', help='save results to project/name')
    parser.add_argument('--name', default='exp', help='save results to project/name')
    parser.add_argument('--exist-ok', action='store_true', help='existing project/name ok, do not increment')
    parser.add_argument('--line-thickness', default=2, type=int, help='bounding box thickness (pixels)')
    parser.add_argument('--hide-labels', default=False, action='store_true', help='hide labels')
    parser.add_argument('--hide-conf', default=True, action='store_true', help='hide confidences')
    parser.add_argument('--batch-size', type=int, default=1, help='pairs of one original size per forward')
    return parser


def check_options(opt):
    """Raise for what this driver does not do (cv2 windows, video and stream sources, --update, augmented inference)."""
    source1 = str(opt.source1)
    if opt.view_img:
        raise NotImplementedError("detect: --view-img needs a cv2 window; save the images instead")
    if opt.update:
        raise NotImplementedError("detect: --update (strip_optimizer over the yolov5 weights) is not part of this package")
    if opt.augment:
        raise NotImplementedError("detect: --augment (test-time augmentation) is not implemented")
    if source1.isnumeric() or source1.endswith('.txt') or source1.lower().startswith(('rtsp://', 'rtmp://', 'http://', 'https://')):
        raise NotImplementedError(f"detect: webcam / stream source '{source1}' needs cv2.VideoCapture; give image files or folders")


def _class_string(hist_row, names):
    """'3 persons, 1 car, ' (detect_twostream.py:134-136): the classes in ascending order, as ``unique()`` gives them."""
    return "".join(f"{n} {names[c]}{'s' * (n > 1)}, " for c, n in enumerate(hist_row) if n > 0)


def _save_image(path, array):
    from PIL import Image
    Image.fromarray(array).save(path)


def boxes_and_render(dets, counts, shapes, img_hw, originals, renderer, nc):
    """The device stage of one batch: ``cft_detect_boxes`` and, with a ``renderer``, ``cft_detect_render`` into ``originals``.  Returns
    ``(boxes, hist, flag)`` on the device.  No synchronisation with the host."""
    geom = _to_device(geometry(shapes, img_hw), dets.device)
    boxes, hist, flag = detect_boxes(dets, counts, geom, nc)
    if renderer is not None:
        renderer(boxes, [o[0] for o in originals], [o[1] for o in originals])
    return boxes, hist, flag


def detect(opt, model=None, log=print, record=None):
    """``detect(opt)`` of detect_twostream.py:19-194.  ``model``: an already loaded model instead of ``opt.weights``.  ``record``: a list
    that receives, per image, a dict of what was computed (paths, NMS output, box buffer, printed line) - for tests and callers.

    ``opt.device_jpeg`` (absent = False): saved images whose name ends in .jpg / .jpeg are encoded by ``utils.jpeg.encode_jpeg_start`` -
    colour conversion, DCT and quantisation on the device, Huffman coding on the pool - to the bytes PIL writes for them; the drawn
    originals are then copied to the host only for ``record`` or for files of another suffix, which stay on PIL."""
    check_options(opt)
    source1, source2, save_txt, imgsz = opt.source1, opt.source2, opt.save_txt, opt.img_size
    save_img = not opt.nosave                                                     # (.txt sources are refused above)
    save_dir = increment_path(Path(opt.project) / opt.name, exist_ok=opt.exist_ok)
    (save_dir / 'labels' if save_txt else save_dir).mkdir(parents=True, exist_ok=True)

    dev = str(opt.device).split(',')[0]
    if dev == 'cpu':
        raise RuntimeError("detect: this package runs on the GPU only (--device cpu)")
    device = torch.device(f"cuda:{int(dev)}" if dev.isnumeric() else dev)
    if model is None:
        from . import compat
        model = compat.attempt_load(opt.weights, map_location="cpu")
    model = model.to(device).eval()
    stride = int(model.stride.max())
    if imgsz % stride:                                                            # check_img_size (utils/general.py:99-104)
        new = max(-(-imgsz // stride) * stride, stride)
        log(f'WARNING: --img-size {imgsz} must be multiple of max stride {stride}, updating to {new}')
        imgsz = new
    names = list(model.module.names if hasattr(model, 'module') else model.names)
    nc = len(names)
    model.half()                                                                  # the reference runs fp16 on a GPU (detect_twostream.py:40-41)

    dataset = LoadImagePairs(source1, source2, imgsz, stride, batch_size=opt.batch_size, device=device)
    draw = save_img                                                               # boxes are drawn only into images that are saved
    device_jpeg = bool(getattr(opt, 'device_jpeg', False)) and save_img
    renderer = BoxRenderer(names, device, opt.line_thickness, opt.hide_labels, opt.hide_conf) if draw else None

    t0 = time.time()
    img_num, fps_sum = 0, 0.0
    with ThreadPoolExecutor(MAX_DECODE_THREADS) as pool:
        jobs = []
        for paths, img, originals, shapes in dataset:
            B, H, W = img.shape[0], img.shape[2], img.shape[3]
            t1 = time.time()
            with torch.no_grad():
                pred = model(img[:, :3], img[:, 3:])[0]
                dets, counts = batched_nms(pred, opt.conf_thres, opt.iou_thres, classes=opt.classes, agnostic=opt.agnostic_nms, max_det=MAX_DET)
            undrawn = [o[0] for o in dataset.host_originals]                      # crops are cut from the undrawn original, on the host
            boxes, hist, flag = boxes_and_render(dets, counts, shapes, (H, W), originals, renderer, nc)
            on_device = [device_jpeg and is_jpeg_name(paths[b][0]) for b in range(B)]
            job, job_slot = None, {}
            if any(on_device):                                                    # started before the box buffer's copy waits for the device
                job_slot = {b: 2 * k for k, b in enumerate(b for b in range(B) if on_device[b])}
                job = encode_jpeg_start([o for b in job_slot for o in originals[b]])
            n_words = boxes.numel()
            packed = torch.cat((boxes.view(-1), hist.view(-1), flag.view(-1))).cpu().numpy()   # the one copy of the box buffer
            t2 = time.time()
            slots = packed[:n_words].reshape(B, MAX_DET, -1)
            hists = packed[n_words:-1].reshape(B, nc)
            if packed[-1]:
                raise RuntimeError(f"detect: a detection's class is outside [0, {nc}) - the model's names do not match its head")
            drawn = None
            if save_img and (record is not None or not all(on_device)):
                drawn = torch.stack([torch.stack(o) for o in originals]).cpu().numpy()     # one copy of the drawn originals (one size per batch)
            for b in range(B):
                p = Path(paths[b][0])
                n = int(slots[b, :, 6].sum())
                s = '%gx%g ' % (H, W) + _class_string(hists[b].tolist(), names)
                xywh = slots[b, :n, 12:16].copy().view(np.float32)
                conf = slots[b, :n, 7].copy().view(np.float32)
                if save_txt and n:
                    with open(save_dir / 'labels' / (p.stem + '.txt'), 'a') as f:
                        f.writelines(txt_line(float(slots[b, r, 4]), xywh[r].tolist(), float(conf[r]) if opt.save_conf else None)
                                     for r in reversed(range(n)))
                if opt.save_crop:
                    for r in reversed(range(n)):
                        save_one_box(slots[b, r, 0:4], undrawn[b], file=save_dir / 'crops' / names[int(slots[b, r, 4])] / f'{p.stem}.jpg',
                                     rect=slots[b, r, 8:12])
                line = f'{s}Done. ({(t2 - t1) / B:.6f}s, {B / max(t2 - t1, 1e-9):.6f}Hz)'
                log(line)
                img_num += 1
                fps_sum += B / max(t2 - t1, 1e-9)
                if save_img:
                    save_path = str(save_dir / p.name)
                    stem, ext = save_path.rsplit('.', 1) if '.' in p.name else (save_path, 'jpg')
                    log(stem + '_rgb.' + ext)
                    if on_device[b]:                                              # the pool waits for the coefficient copy, codes, writes
                        jobs.append(pool.submit(job.save, job_slot[b], stem + '_rgb.' + ext))
                        jobs.append(pool.submit(job.save, job_slot[b] + 1, stem + '_ir.' + ext))
                    else:
                        jobs.append(pool.submit(_save_image, stem + '_rgb.' + ext, drawn[b, 0]))
                        jobs.append(pool.submit(_save_image, stem + '_ir.' + ext, drawn[b, 1]))
                if record is not None:
                    record.append({"paths": paths[b], "shape": shapes[b][0], "img_hw": (H, W), "dets": dets[b, :n].cpu(), "slots": slots[b].copy(),
                                   "hist": hists[b].copy(), "s": s, "drawn": None if drawn is None else drawn[b].copy()})
        for j in jobs:
            j.result()

    if save_txt or save_img:
        s = f"\n{len(list(save_dir.glob('labels/*.txt')))} labels saved to {save_dir / 'labels'}" if save_txt else ''
        log(f"Results saved to {save_dir}{s}")
    log(f'Done. ({time.time() - t0:.3f}s)')
    if img_num:
        log(f'Average Speed: {fps_sum / img_num:.6f}Hz')
    return save_dir
