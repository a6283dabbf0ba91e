"""mAP evaluation of a model on the GPU: what the reference's ``test.py`` computes for its metrics (:99-236, :292-294).

    from msod_amd.evaluate import evaluate
    (mp, mr, map50, map75, map), maps = evaluate(model, dataloader, nc)
    (mp, mr, map50, map75, map, box, obj, cls), maps = evaluate(model, dataloader, nc, compute_loss=ComputeLoss(model))

Per batch: the forward on the uint8 views (the /255 is fused into Focus), ``batched_nms(multi_label=True,
agnostic=single_cls)`` and ``DetectionEvaluator.update`` - no host synchronisation beyond the iterator's own.  One
synchronisation at the end computes the statistics.  With ``compute_loss`` (``utils.loss.ComputeLoss``) the validation
loss is accumulated on the device too, as test.py does (:121-123, :295).  Plots, save_txt / save_json and the confusion
matrix are not computed.
"""
import torch

from .utils.general import batched_nms
from .utils.metrics import DetectionEvaluator


def evaluate(model, batches, nc, conf_thres=0.001, iou_thres=0.6, single_cls=False, compute_loss=None):
    """batches: an iterable of ``(img6_uint8 [B, 6, H, W], targets [nt, 6], paths, shapes)`` as test.py's dataloader yields.
    Returns test.py's ``((mp, mr, map50, map75, map), maps)``; with ``compute_loss``, test.py's
    ``((mp, mr, map50, map75, map, box, obj, cls), maps)``, the losses averaged over the batches."""
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("evaluate: the model must be on the GPU (this package has no CPU path)")
    ev = DetectionEvaluator(1 if single_cls else nc, single_cls)          # test.py:74
    loss = torch.zeros(3, device=device) if compute_loss is not None else None
    nb = 0
    for img, targets, paths, shapes in batches:
        if img.dim() != 4 or img.shape[1] != 6:
            raise ValueError(f"evaluate: images must be [B, 6, H, W] (RGB and IR stacked), got {tuple(img.shape)}")
        if img.device != device:
            img = img.pin_memory().to(device, non_blocking=True) if img.device.type == "cpu" else img.to(device)
        H, W = img.shape[2], img.shape[3]
        with torch.no_grad():
            res = model(img[:, :3], img[:, 3:])
            out = res[0]
            if compute_loss is not None:                                   # test.py:121-123, normalised targets
                loss += compute_loss([x.float().contiguous() for x in res[1]], targets)[1][:3]
            dets, counts = batched_nms(out, conf_thres, iou_thres, multi_label=True, agnostic=single_cls)
        ev.update(dets, counts, targets, (H, W), shapes)
        nb += 1
    if compute_loss is None:
        return ev.compute().as_test_tuple()
    results, maps = ev.compute().as_test_tuple()
    losses = (loss.cpu() / nb).tolist() if nb else [0.0, 0.0, 0.0]          # test.py:295
    compute_loss.check()
    return (*results, *losses), maps
