"""Generate ``tests/golden/eval/confusion_cases.pt``: the reference's own confusion matrix, save_txt / save_hybrid label files
and save_json list on synthetic batches.

Runs ONLY in the build container (needs the reference checkout next to ``make_golden.py``'s ``REF``).  The reference's
``test.py`` and ``utils/metrics.py`` run unmodified on CPU, set up as in ``make_eval_golden.py`` (stub model, list dataloader,
``torchvision.ops.nms`` bound to ``oracle/nms_oracle.greedy_nms``), with ``plots=True`` and these stand-ins:
  * ``test.plot_images`` is a no-op and ``test.ap_per_class`` is forced to ``plot=False`` (no figures);
  * ``test.ConfusionMatrix`` is a subclass that records every ``process_batch`` input and does not plot;
  * ``test.non_max_suppression`` is wrapped to record its output.
Each case runs four more times into a temporary ``save_dir``: ``save_txt`` with and without ``save_conf``, ``save_hybrid``
(with ``save_txt``, as test.py:336 sets it) and ``save_json``; the written files are read back.

    python tests/golden/make_confusion_golden.py       # rewrites tests/golden/eval/confusion_cases.pt

The file holds data only: inputs, matrices, recorded process_batch inputs and NMS outputs, file texts, the JSON list.

The script asserts that no image has two exactly equal IoUs above 0.45 among its detections above 0.25 (numpy's argsort
is not stable, so the reference's result would depend on it) - pick another seed if it trips - and that the constructed
cases show what they were built for.
"""
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402
from make_eval_golden import StubModel, make_case  # noqa: E402
from oracle.nms_oracle import greedy_nms  # noqa: E402

OUT = os.path.join(HERE, "eval", "confusion_cases.pt")

# the five shapes of cases of make_eval_golden.py (name, nc, labelled classes, single_cls, batches, images per batch, (H, W),
# ratio_pad given, seed, mode); the seeds are those that pass the tie-free assertion
CASES = [
    ("nc3_rect", 3, (0, 1), False, 2, 4, (256, 320), True, 11, "normal"),
    ("nc1_square_nopad", 1, (0,), False, 2, 3, (192, 192), False, 12, "normal"),
    ("nc9_rect", 9, (0, 1, 2, 4, 5, 7, 8), False, 3, 4, (192, 256), True, 613, "normal"),
    ("single_cls", 3, (0,), True, 2, 4, (256, 256), True, 14, "normal"),
    ("no_tp", 3, (0, 1, 2), False, 1, 3, (128, 160), True, 15, "no_tp"),
]


def constructed_case(seed=21):
    """One batch of four images, nc = 3, built for the quirks of process_batch:
    image 0: labels and detections, no detection above 0.25 -> every label is background;
    image 1: two matches, a second detection on a matched label and far detections left over -> they count at [class, nc];
    image 2: detections above 0.25, none overlapping a label -> no match, so the detections are NOT counted (`if n:`);
    image 3: one detection over two labels and two detections over one label."""
    g = np.random.default_rng(seed)
    nc, H, W = 3, 256, 320
    h0, w0 = 480, 600
    r = min(H / h0, W / w0)
    shape = ((h0, w0), ((r, r), ((W - w0 * r) / 2, (H - h0 * r) / 2)))
    j = lambda s=1.5: float(g.normal(0, s))  # noqa: E731
    # per image: labels (cls, cx, cy, w, h) in letterbox pixels; detections (cx, cy, w, h, obj, cls, cls_conf)
    images = [
        ([(0, 80, 90, 60, 50), (1, 200, 120, 70, 60), (2, 150, 200, 50, 40)],
         [(80 + j(), 90 + j(), 60 + j(), 50 + j(), 0.4, 0, 0.5), (200 + j(), 120 + j(), 70 + j(), 60 + j(), 0.3, 1, 0.6),
          (150 + j(), 200 + j(), 50 + j(), 40 + j(), 0.45, 2, 0.5)]),
        ([(0, 70, 80, 60, 60), (1, 220, 100, 80, 70), (2, 160, 190, 40, 50)],
         [(70 + j(), 80 + j(), 60 + j(), 60 + j(), 0.9, 0, 0.9), (220 + j(), 100 + j(), 80 + j(), 70 + j(), 0.8, 2, 0.9),
          (72 + j(3), 83 + j(3), 66 + j(3), 55 + j(3), 0.7, 1, 0.8), (40, 220, 30, 30, 0.9, 1, 0.7), (290, 215, 30, 40, 0.6, 0, 0.8)]),
        ([(1, 90, 90, 50, 50), (2, 230, 180, 60, 50)],
         [(200 + j(), 60 + j(), 40, 40, 0.9, 1, 0.9), (60 + j(), 200 + j(), 50, 40, 0.8, 0, 0.7), (150, 128, 20, 20, 0.7, 2, 0.9)]),
        ([(0, 100, 100, 60, 60), (0, 120, 104, 60, 60), (2, 230, 170, 70, 60)],
         [(110 + j(), 102 + j(), 62 + j(), 60 + j(), 0.9, 0, 0.9), (230 + j(), 170 + j(), 70 + j(), 60 + j(), 0.9, 2, 0.8),
          (233 + j(3), 168 + j(3), 64 + j(3), 66 + j(3), 0.8, 1, 0.9), (228 + j(3), 175 + j(3), 75 + j(3), 52 + j(3), 0.5, 2, 0.4)]),
    ]
    R = 8
    pre = np.zeros((len(images), R, 5 + nc), np.float32)
    pre[:, :, :4] = (W / 2, H / 2, 10, 10)                       # padding rows: obj = 0 (filtered by conf_thres)
    tg = []
    for i, (labels, dets) in enumerate(images):
        for (c, cx, cy, bw, bh) in labels:
            tg.append((i, c, cx / W, cy / H, bw / W, bh / H))
        for k, (cx, cy, bw, bh, obj, c, cc) in enumerate(dets):
            pre[i, k, :4] = (cx, cy, bw, bh)
            pre[i, k, 4] = obj
            pre[i, k, 5:] = g.uniform(0, 0.0009, nc)
            pre[i, k, 5 + c] = cc
    return [{"rows": torch.from_numpy(pre), "targets": torch.tensor(tg, dtype=torch.float32).reshape(-1, 6),
             "shapes": [shape] * len(images), "img_hw": (H, W)}]


def paths_of(name, batches):
    """Image paths: numeric stems for the nc1 case (save_json's image_id is then an int), names for the others."""
    out = []
    for bi, b in enumerate(batches):
        n = b["rows"].shape[0]
        out.append([f"{1000 * (bi + 1) + i:06d}.jpg" if name.startswith("nc1") else f"{name}_b{bi}_{i}.jpg" for i in range(n)])
    return out


def run(test, nc, single_cls, batches, paths, save_dir, record=None, **kw):
    """One test.test() run on CPU.  record: a dict that receives the process_batch inputs, the NMS outputs and the matrix."""
    orig = test.non_max_suppression, test.ap_per_class, test.ConfusionMatrix, test.plot_images
    calls, nms_out, made = [], [], []

    class Recording(orig[2]):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def process_batch(self, detections, labels):
            calls.append((detections.clone(), labels.clone()))
            return super().process_batch(detections, labels)

        def plot(self, *a, **k):
            pass

    def nms(*a, **k):
        out = orig[0](*a, **k)
        nms_out.append([o.clone() for o in out])
        return out

    def ap(*a, **k):
        k["plot"] = False
        return orig[1](*a, **k)

    test.non_max_suppression, test.ap_per_class, test.ConfusionMatrix, test.plot_images = nms, ap, Recording, lambda *a, **k: None
    try:
        model = StubModel(nc, [b["rows"] for b in batches])
        loader = []
        for b, p in zip(batches, paths):
            H, W = b["img_hw"]
            loader.append((torch.zeros((b["rows"].shape[0], 6, H, W), dtype=torch.uint8), b["targets"].clone(), p, b["shapes"]))
        test.test({"nc": nc}, batch_size=len(paths[0]), model=model, dataloader=loader, single_cls=single_cls, plots=True,
                  save_dir=Path(save_dir), **kw)
    finally:
        test.non_max_suppression, test.ap_per_class, test.ConfusionMatrix, test.plot_images = orig
    if record is not None:
        record["process_batch"] = calls
        record["nms"] = nms_out
        record["matrix"] = torch.from_numpy(np.array(made[-1].matrix, dtype=np.float64))
    return nms_out


def read_labels(save_dir):
    d = Path(save_dir) / "labels"
    return {f.stem: f.read_text() for f in sorted(d.glob("*.txt"))}


def check_tie_free(general, name, calls, conf=0.25, thr=0.45):
    for k, (det, lab) in enumerate(calls):
        det = det[det[:, 4] > conf]
        iou = general.box_iou(lab[:, 1:], det[:, :4])
        v = iou[iou > thr]
        assert v.unique().numel() == v.numel(), f"{name}: process_batch call {k} has tied IoUs above {thr}, pick another seed"


def main():
    make_golden.install_reference()
    import torchvision  # the stand-in module
    torchvision.ops = type(sys)("torchvision.ops")
    torchvision.ops.nms = greedy_nms
    torch.set_num_threads(os.cpu_count())
    import test  # the reference's test.py
    from utils import general  # the reference's
    cases = []
    todo = [(c[0], c[1], c[3], make_case(*c)) for c in CASES] + [("constructed", 3, False, constructed_case())]
    for name, nc, single_cls, batches in todo:
        nc_run = 1 if single_cls else nc
        paths = paths_of(name, batches)
        rec = {}
        with tempfile.TemporaryDirectory() as d:
            run(test, nc_run, single_cls, batches, paths, d, record=rec)
        check_tie_free(general, name, rec["process_batch"])
        for b, p, dets in zip(batches, paths, rec["nms"]):
            b["paths"], b["dets"] = p, dets
        case = {"name": name, "nc": nc, "single_cls": single_cls, "conf_thres": 0.001, "iou_thres": 0.6, "batches": batches,
                "matrix": rec["matrix"], "process_batch": rec["process_batch"]}
        for key, kw in (("txt_conf", dict(save_txt=True, save_conf=True)), ("txt", dict(save_txt=True, save_conf=False)),
                        ("hybrid", dict(save_txt=True, save_hybrid=True, save_conf=True)), ("json", dict(save_json=True))):
            with tempfile.TemporaryDirectory() as d:
                if "save_txt" in kw:
                    os.makedirs(os.path.join(d, "labels"))
                nms_out = run(test, nc_run, single_cls, batches, paths, d, **kw)
                if key == "json":
                    f = os.path.join(d, "_predictions.json")
                    case["jdict"] = json.load(open(f)) if os.path.exists(f) else []
                else:
                    case[key] = read_labels(d)
                if key == "hybrid":
                    case["hybrid_dets"] = nms_out
        cases.append(case)
        m = rec["matrix"].numpy()
        print(f"{name}: {len(rec['process_batch'])} process_batch calls, matrix sum {m.sum():.0f}, diagonal {np.trace(m[:nc_run, :nc_run]):.0f}, "
              f"background row {m[nc_run].sum():.0f}, background column {m[:, nc_run].sum():.0f}, {len(case['txt'])} label files, "
              f"{len(case['jdict'])} json entries")
        if name == "constructed":
            pb = rec["process_batch"]
            assert len(pb) == 4
            assert (pb[0][0][:, 4] > 0.25).sum() == 0 and len(pb[0][0]) > 0            # image 0: nothing above 0.25
            iou2 = general.box_iou(pb[2][1][:, 1:], pb[2][0][pb[2][0][:, 4] > 0.25][:, :4])
            assert (pb[2][0][:, 4] > 0.25).sum() >= 2 and not (iou2 > 0.45).any()       # image 2: detections, no match
            # labels: 3 + 3 + 2 + 3; image 1 leaves detections over: the background column is not empty
            assert m[:, :nc].sum() == 11 and m[:nc, nc].sum() >= 3
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save({"cases": cases}, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
