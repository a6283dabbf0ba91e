"""Validate a checkpoint on a paired RGB + IR dataset on disk: the command-line form of the reference's test.py.

    python tools/val.py DATA.yaml WEIGHTS.pt [--img-size 640] [--batch-size 32] [--single-cls] [--save-txt] [--save-json] [--plots] [--curves] [--verbose]
                        [--modality rgb|ir] [--augment]

DATA.yaml holds ``val_rgb`` and ``val_ir`` (directories or *.txt lists; relative paths are taken from the yaml's directory), ``nc``
and ``names``.  The loader is built as test.py builds it (:86-94: ``rect=True, pad=0.5``, the model's largest stride), every batch is
one cft_pair_batch_u8 launch, ``evaluate`` does the rest on the GPU, and the table printed is test.py's (:100, :239-245).
Every label class must be below ``nc`` unless ``--single-cls`` is given (test.py asserts the same of its data yaml); the check runs
before the first batch.  ``--seeded CFG`` validates a seeded ``models/configs.py`` network instead of a checkpoint: a run without
weights, e.g. on tests/golden/dataset/data.yaml, whose labels hold a class >= nc on purpose and so need ``--single-cls``.
A single-stream checkpoint (``models.yolo.Model``: a YOLOv5-RGB or YOLOv5-IR baseline) is validated on the same paired data with
``--modality rgb`` or ``--modality ir``; ``--augment`` is test.py's flag, test-time augmentation, for such a model (``--seeded`` takes
the stock names yolov5s / m / l / x too)."""
import argparse
import os
import sys
from types import SimpleNamespace

import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.evaluate import evaluate  # noqa: E402
from msod_amd.utils.datasets import create_dataloader_rgb_ir  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("data")
    ap.add_argument("weights", nargs="?")
    ap.add_argument("--seeded", metavar="CFG", help="a named config with seeded weights instead of a checkpoint")
    ap.add_argument("--img-size", type=int, default=640)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--conf-thres", type=float, default=0.001)
    ap.add_argument("--iou-thres", type=float, default=0.6)
    ap.add_argument("--single-cls", action="store_true")
    ap.add_argument("--save-txt", action="store_true")
    ap.add_argument("--save-json", action="store_true")
    ap.add_argument("--plots", action="store_true", help="test_batch{0,1,2}_{labels,pred}[_ir].jpg of the first three batches in --save-dir")
    ap.add_argument("--curves", action="store_true", help="PR / F1 / P / R / MR curve images in --save-dir and an MR^-2 column (log-average miss rate)")
    ap.add_argument("--device-jpeg", action="store_true", help="encode the --plots mosaics on the GPU instead of with PIL (the same bytes)")
    ap.add_argument("--save-dir", default="runs/val")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--modality", choices=("rgb", "ir"), help="single-stream model: the stream of each pair it sees")
    ap.add_argument("--augment", action="store_true", help="single-stream model: test-time augmentation (test.py --augment)")
    opt = ap.parse_args(argv)
    if (opt.weights is None) == (opt.seeded is None):
        ap.error("give WEIGHTS or --seeded CFG")

    with open(opt.data) as f:
        data = yaml.safe_load(f)
    base = os.path.dirname(os.path.abspath(opt.data))
    resolve = lambda p: [resolve(x) for x in p] if isinstance(p, list) else (p if os.path.isabs(p) else os.path.join(base, p))  # noqa: E731
    nc = 1 if opt.single_cls else int(data["nc"])

    device = torch.device("cuda:0")
    if opt.seeded:
        from msod_amd.models.configs import STOCK_YAMLS, named_config, stock_config
        from msod_amd.utils.seeded import seeded_state_dict
        if opt.seeded in STOCK_YAMLS:
            from msod_amd.models.yolo import Model
            model = Model(stock_config(opt.seeded, nc=nc))
        else:
            from msod_amd.models.yolo_test import Model
            model = Model(named_config(opt.seeded))
        model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    else:
        from msod_amd import compat
        model = compat.attempt_load(opt.weights, map_location="cpu")
    model = model.to(device).eval()
    single = getattr(model, "inputs", 2) == 1
    if single and opt.modality is None:
        ap.error("a single-stream model needs --modality rgb or --modality ir")
    if not single and opt.modality:
        ap.error("--modality is for single-stream models; a two-stream model takes both streams")
    gs = max(int(model.stride.max()), 32)  # grid size (max stride)
    names = data.get("names") or [str(i) for i in range(nc)]

    loader, dataset = create_dataloader_rgb_ir(resolve(data["val_rgb"]), resolve(data["val_ir"]), opt.img_size, opt.batch_size, gs,
                                               SimpleNamespace(single_cls=opt.single_cls), pad=0.5, rect=True,
                                               workers=opt.workers, prefix="val: ")
    if not opt.single_cls:
        for f, l in zip(dataset.label_files_rgb, dataset.labels):
            if len(l) and l[:, 0].max() >= nc:
                sys.exit(f"val: {f} holds class {int(l[:, 0].max())}, but {opt.data} says nc: {nc} (classes 0..{nc - 1}); "
                         f"fix the labels or nc, or pass --single-cls")
    details = {}
    evaluate(model, loader, nc, conf_thres=opt.conf_thres, iou_thres=opt.iou_thres, single_cls=opt.single_cls, save_txt=opt.save_txt,
             save_json=opt.save_json, save_dir=opt.save_dir if (opt.save_txt or opt.save_json or opt.plots or opt.curves) else None,
             details=details, plots=opt.plots, names=names if (opt.plots or opt.curves) else None, device_jpeg=opt.device_jpeg, curves=opt.curves,
             modality=opt.modality, augment=opt.augment)
    res = details["result"]
    cv = details.get("curves")
    lamr = {int(c): v for c, v in zip(cv.ap_class, cv.lamr)} if cv is not None else {}

    cols = ('Class', 'Images', 'Labels', 'P', 'R', 'mAP@.5', 'mAP@.75', 'mAP@.5:.95') + (('MR^-2',) if cv is not None else ())
    print(('%20s' + '%12s' * (len(cols) - 1)) % cols)
    pf = '%20s' + '%12i' * 2 + '%12.3g' * (len(cols) - 3)  # print format
    print(pf % (('all', res.seen, int(res.nt.sum()), res.mp, res.mr, res.map50, res.map75, res.map) + ((cv.mlamr,) if cv is not None else ())))
    if (opt.verbose or nc < 50) and nc > 1 and len(res.ap_class):
        ap = res.ap
        for i, c in enumerate(res.ap_class):
            print(pf % ((names[c] if c < len(names) else str(c), res.seen, res.nt[c], res.p[i], res.r[i], ap[i, 0], ap[i, 5], ap[i].mean())
                        + ((lamr[int(c)],) if cv is not None else ())))
    if opt.save_txt or opt.save_json or opt.plots or opt.curves:
        print(f"Results saved to {opt.save_dir}")
    return res


if __name__ == "__main__":
    main()
