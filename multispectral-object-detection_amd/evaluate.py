"""mAP evaluation of a model on the GPU: what the reference's ``test.py`` computes for its metrics (:99-236, :292-294).

    from msod_amd.evaluate import evaluate
    (mp, mr, map50, map75, map), maps = evaluate(model, dataloader, nc)
    (mp, mr, map50, map75, map, box, obj, cls), maps = evaluate(model, dataloader, nc, compute_loss=ComputeLoss(model))
    results, maps, extras = evaluate(model, dataloader, nc, confusion=True, save_txt=True, save_json=True, save_dir="runs/val")

Per batch: the forward on the uint8 views (the /255 is fused into Focus), ``batched_nms(multi_label=True,
agnostic=single_cls)`` and ``DetectionEvaluator.update`` - no host synchronisation beyond the iterator's own.  One
synchronisation at the end computes the statistics.  With ``compute_loss`` (``utils.loss.ComputeLoss``) the validation
loss is accumulated on the device too, as test.py does (:121-123, :295).

The rest of what ``python test.py`` gives is behind keywords that are off by default (the default path is unchanged):

* ``confusion``    the (nc+1) x (nc+1) confusion matrix of test.py's ``plots=True`` (``utils.metrics.ConfusionMatrix``: its
                   rules, quirks and tie rule are described there), accumulated on the device, still without synchronisation;
* ``save_txt``     one ``save_dir/labels/<stem>.txt`` per image with detections, a line ``class x y w h`` (normalised, ``%g``) per
                   detection, with the confidence appended if ``save_conf`` (test.py:152-158).  Lines are appended, as there;
* ``save_hybrid``  the batch's labels join the NMS candidates as a-priori rows (test.py:126-129, utils/general.py:480-487); implies
                   ``save_txt`` (test.py:336).  The rows are built on the host from the dataloader's CPU targets;
* ``save_json``    the COCO-style list of test.py:173-182, returned as ``jdict`` and, with a ``save_dir``, written to
                   ``save_dir/predictions.json``.

* ``plots``        the batch mosaics of test.py's ``plots=True`` (:220-225): for the first three batches
                   ``save_dir/test_batch{i}_labels.jpg`` and ``test_batch{i}_pred.jpg`` (``utils.plots.plot_images``, built on the
                   device) with their ``_ir`` twins for the second stream, twelve files, and nothing else;
* ``curves``       the curve images of test.py's ``plots=True`` (utils/metrics.py:71-75): ``save_dir/PR_curve.png``, ``F1_curve.png``,
                   ``P_curve.png`` and ``R_curve.png``, and ``MR_curve.png``, the miss rate over false positives per image with the
                   log-average miss rate (``utils.metrics.curves_per_class`` defines it); with ``confusion`` also
                   ``confusion_matrix.png`` (test.py:239).  The numbers come from one more device stage after the statistics
                   (``DetectionEvaluator.curves``, one more synchronisation); matplotlib draws them on the host.

A single-stream model (``models.yolo.Model``, a single-modality baseline) is evaluated on the same paired loader: ``modality='rgb'`` or
``'ir'`` picks channels [0:3] or [3:6] of each batch (a view, not a copy), and ``augment=True`` - test.py's ``--augment`` - runs its
test-time augmentation.  Everything behind the forward is the same code.  With a two-stream model ``modality`` is refused and ``augment`` meets ``Model.forward``'s own refusal.

The values written come from one kernel (``cft_eval_export``) and one device-to-host copy per batch: the only added
synchronisation, and only when a save option is on.  wandb logging and pycocotools scoring are not done.
"""
import json
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import torch

from .utils.general import batched_nms
from .utils.metrics import DetectionEvaluator, export_batch, export_rows, json_entry, txt_line


def _apriori_rows(targets, B, no, H, W):
    """save_hybrid: the labels of a batch as pre-NMS rows [B, L, no] on the host (utils/general.py:480-487: box in letterbox pixels,
    obj = 1, one-hot class), L = the most labels of one image; images with fewer get obj = 0 rows, which the conf filter drops."""
    if targets.device.type != "cpu":
        raise ValueError("evaluate: save_hybrid builds the a-priori rows on the host and needs the dataloader's CPU targets")
    t = targets.float()
    px = t[:, 2:] * torch.tensor([W, H, W, H], dtype=torch.float32)       # test.py:126, float32 as there
    idx = [(t[:, 0] == b).nonzero().view(-1) for b in range(B)]            # test.py:127
    L = max(len(i) for i in idx)
    if L == 0:
        return None
    cls = t[:, 1].long()
    if len(cls) and (int(cls.min()) < 0 or int(cls.max()) >= no - 5):
        raise ValueError(f"evaluate: save_hybrid labels have a class outside [0, {no - 5})")
    extra = torch.zeros((B, L, no), dtype=torch.float32)
    for b, i in enumerate(idx):
        k = len(i)
        extra[b, :k, :4] = px[i]
        extra[b, :k, 4] = 1.0
        extra[b, torch.arange(k), cls[i] + 5] = 1.0
    return extra


def _save_mosaics(host, event, flag, files):
    """Pool job of ``plots``: wait for the batch's device-to-host copies, check the slot kernel's flag word, encode."""
    from .utils.plots import check_mosaic_flag, save_mosaic
    event.synchronize()
    if flag is not None:
        check_mosaic_flag(int(flag[0]))
    for a, f in zip(host, files):
        save_mosaic(a.numpy(), f)


def _save_mosaics_coded(job, event, flag, files):
    """Pool job of ``plots`` with ``device_jpeg``: wait for the flag word and the coefficients, Huffman-code, write the files."""
    from .utils.plots import check_mosaic_flag
    event.synchronize()
    if flag is not None:
        check_mosaic_flag(int(flag[0]))
    for k, f in enumerate(files):
        job.save(k, f)


def _plot_batch(pool, img, targets, paths, fname, names, device_jpeg=False):
    """One mosaic (both streams) on the device, then its copies to pinned memory; the wait and the encoding go to the pool.  With
    ``device_jpeg`` and a .jpg / .jpeg name what is copied are the quantised coefficients of the device encoder, not the pixels."""
    from .utils.jpeg import encode_jpeg_start, is_jpeg_name
    from .utils.plots import mosaic_file_names, plot_images_device
    mosaics, flag, _ = plot_images_device(img, targets, paths, names)
    coded = device_jpeg and is_jpeg_name(fname)
    if coded:
        job = encode_jpeg_start(list(mosaics))
    else:
        host = [torch.empty(m.shape, dtype=m.dtype).pin_memory().copy_(m, non_blocking=True) for m in mosaics]
    if flag is not None:
        flag = torch.empty(1, dtype=torch.int32).pin_memory().copy_(flag, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    if coded:
        return pool.submit(_save_mosaics_coded, job, event, flag, mosaic_file_names(fname, len(job)))
    return pool.submit(_save_mosaics, host, event, flag, mosaic_file_names(fname, len(host)))


def _save_curves(cv, res, ev, save_dir, names):
    """``curves``: the images of utils/metrics.py:71-75 and test.py:239 from the host copies, plus the MR curve."""
    from .utils import metrics
    names = names if names is not None else ()
    ap = res.ap if len(cv.ap_class) == len(res.ap_class) else [[0.0]] * len(cv.ap_class)      # no TP at all: test.py reports zeros
    metrics.plot_pr_curve(cv, ap, save_dir, names)
    for which in ("f1", "p", "r"):
        metrics.plot_mc_curve(cv, which, save_dir, names)
    metrics.plot_mr_curve(cv, save_dir, names)
    if ev.confusion_matrix is not None:
        ev.confusion_matrix.plot(save_dir=save_dir, names=list(names.values()) if isinstance(names, dict) else list(names))


def evaluate(model, batches, nc, conf_thres=0.001, iou_thres=0.6, single_cls=False, compute_loss=None, confusion=False,
             save_txt=False, save_conf=False, save_hybrid=False, save_json=False, save_dir=None, details=None, plots=False, names=None,
             device_jpeg=False, curves=False, modality=None, augment=False):
    """batches: an iterable of ``(img6_uint8 [B, 6, H, W], targets [nt, 6], paths, shapes)`` as test.py's dataloader yields.
    Returns test.py's ``((mp, mr, map50, map75, map), maps)``; with ``compute_loss``, test.py's
    ``((mp, mr, map50, map75, map, box, obj, cls), maps)``, the losses averaged over the batches.

    With any of ``confusion``, ``save_txt``, ``save_hybrid``, ``save_json`` (module docstring) a third element follows:
    ``{"confusion_matrix": (nc+1, nc+1) float64 numpy array or None, "jdict": list of entries or None}``.

    ``plots`` (needs a ``save_dir``): the label and prediction mosaics of the first three batches, both streams (module docstring), with
    the class ``names`` (None: class numbers); the files are complete when this returns.  It adds no element to the return value.
    ``device_jpeg``: the mosaics are encoded by ``utils.jpeg.encode_jpeg_start`` (device DCT, Huffman coding on the same pool) instead
    of by PIL; the files hold the same bytes.

    ``curves`` (needs a ``save_dir``): the five curve images (module docstring), with ``confusion`` the confusion-matrix image too, named
    with ``names``.  It adds no element to the return value either.

    ``modality`` ('rgb' | 'ir') and ``augment``: for a single-stream model only (module docstring); with ``augment`` the forward returns no
    raw list, so it cannot be combined with ``compute_loss``.

    ``details``: a dict that receives ``"result"``, the ``EvalResult`` behind the returned tuple (per-class p / r / ap, nt, seen - what
    test.py's table prints, tools/val.py) and, with ``curves``, ``"curves"``, the ``EvalCurves``; the return value does not change."""
    if plots and save_dir is None:
        raise ValueError("evaluate: plots needs a save_dir")
    if curves and save_dir is None:
        raise ValueError("evaluate: curves needs a save_dir")
    single = getattr(model, "inputs", 2) == 1
    if single:
        if modality not in ("rgb", "ir"):
            raise ValueError(f"evaluate: a single-stream model needs modality='rgb' or 'ir', got {modality!r}")
        if augment and compute_loss is not None:
            raise ValueError("evaluate: augment=True returns no raw outputs (models/yolo.py:128); the loss cannot be computed with it")
        c0 = 0 if modality == "rgb" else 3
    else:
        if modality is not None:
            raise ValueError("evaluate: modality selects the input of a single-stream model; a two-stream model takes both streams")
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("evaluate: the model must be on the GPU (this package has no CPU path)")
    save_txt = save_txt or save_hybrid                                     # test.py:336
    extras = confusion or save_txt or save_json
    if save_txt:
        if save_dir is None:
            raise ValueError("evaluate: save_txt / save_hybrid need a save_dir")
        (Path(save_dir) / 'labels').mkdir(parents=True, exist_ok=True)    # test.py:54
    if plots or curves:
        Path(save_dir).mkdir(parents=True, exist_ok=True)
    pool, jobs = (ThreadPoolExecutor(max_workers=4), []) if plots else (None, [])
    jdict = [] if save_json else None
    ev = DetectionEvaluator(1 if single_cls else nc, single_cls, confusion=confusion)          # test.py:74, :97
    loss = torch.zeros(3, device=device) if compute_loss is not None else None
    nb = 0
    for img, targets, paths, shapes in batches:
        if img.dim() != 4 or img.shape[1] != 6:
            raise ValueError(f"evaluate: images must be [B, 6, H, W] (RGB and IR stacked), got {tuple(img.shape)}")
        if img.device != device:
            img = img.pin_memory().to(device, non_blocking=True) if img.device.type == "cpu" else img.to(device)
        H, W = img.shape[2], img.shape[3]
        with torch.no_grad():
            if single:
                res = model(img[:, c0:c0 + 3], augment=augment)
            else:                                                          # (augment: Model.forward's own refusal answers)
                res = model(img[:, :3], img[:, 3:], augment=True) if augment else model(img[:, :3], img[:, 3:])
            out = res[0]
            if compute_loss is not None:                                   # test.py:121-123, normalised targets
                loss += compute_loss([x.float().contiguous() for x in res[1]], targets)[1][:3]
            if save_hybrid:
                extra = _apriori_rows(targets, img.shape[0], out.shape[2], H, W)
                if extra is not None:
                    out = torch.cat((out.float(), extra.pin_memory().to(device, non_blocking=True)), 1)
            dets, counts = batched_nms(out, conf_thres, iou_thres, multi_label=True, agnostic=single_cls)
        ev.update(dets, counts, targets, (H, W), shapes)
        if plots and nb < 3:                                               # test.py:220-225
            jobs.append(_plot_batch(pool, img, targets, paths, Path(save_dir) / f'test_batch{nb}_labels.jpg', names, device_jpeg))
            pd = dets
            if single_cls:                                                 # test.py:146-147 zeroes the class in place before it plots `out`
                pd = dets.clone()
                pd[..., 5] = 0
            jobs.append(_plot_batch(pool, img, (pd, counts), paths, Path(save_dir) / f'test_batch{nb}_pred.jpg', names, device_jpeg))
        if save_txt or save_json:
            for stem, rows in export_rows(export_batch(dets, counts, (H, W), shapes, single_cls), paths):
                if save_txt:
                    with open(Path(save_dir) / 'labels' / (stem + '.txt'), 'a') as f:
                        f.writelines(txt_line(r[5], r[8:12], r[4] if save_conf else None) for r in rows)
                if save_json:
                    jdict.extend(json_entry(stem, r[5], r[12:16], r[4]) for r in rows)
        nb += 1
    if pool is not None:
        pool.shutdown(wait=True)                                           # no thread outlives the call: the files are complete
        for j in jobs:
            j.result()
    res = ev.compute()
    if details is not None:
        details["result"] = res
    if curves:
        cv = ev.curves()
        if details is not None:
            details["curves"] = cv
        _save_curves(cv, res, ev, save_dir, names)
    results, maps = res.as_test_tuple()
    if compute_loss is not None:
        losses = (loss.cpu() / nb).tolist() if nb else [0.0, 0.0, 0.0]          # test.py:295
        compute_loss.check()
        results = (*results, *losses)
    if not extras:
        return results, maps
    if save_json and save_dir is not None and len(jdict):                      # test.py:262-268
        Path(save_dir).mkdir(parents=True, exist_ok=True)
        with open(Path(save_dir) / 'predictions.json', 'w') as f:
            json.dump(jdict, f)
    return results, maps, {"confusion_matrix": res.confusion_matrix, "jdict": jdict}
