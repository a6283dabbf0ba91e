"""Generate ``tests/golden/eval/eval_cases.pt``: the reference's own ``test.test()`` statistics on synthetic batches.

Runs ONLY in the build container (needs the reference checkout next to ``make_golden.py``'s ``REF``).  The
reference's ``test.py`` and ``utils/metrics.py`` run unmodified on CPU:
  * ``make_golden.install_reference()`` stands in for the import-time-only modules (cv2, torchvision, seaborn);
    ``torchvision.ops.nms`` is bound to ``oracle/nms_oracle.greedy_nms`` (its published algorithm);
  * the model is a stub ``nn.Module`` (one parameter, ``names``) whose ``forward(x, x2, augment)`` returns the
    case's prepared pre-NMS rows and ``None``;
  * the dataloader is a plain list of ``(img6_uint8, targets, paths, shapes)`` batches, ``plots=False``;
  * ``test.non_max_suppression`` and ``test.ap_per_class`` are wrapped to record their inputs and outputs.

    python tests/golden/make_eval_golden.py       # rewrites tests/golden/eval/eval_cases.pt

(In a subdirectory: tests/test_oracle_golden.py and tests/test_gpu_model.py treat every ``golden/*.pt`` as a forward-pass fixture.)

Predictions are jittered copies of the label boxes (IoUs spread over ~0.3-0.99) plus false positives and
predictions of classes without labels.  Confidences are distinct across each case (numpy's argsort is not
stable under ties), which the script asserts.
"""
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402
from oracle.nms_oracle import greedy_nms  # noqa: E402

OUT = os.path.join(HERE, "eval", "eval_cases.pt")

# name, nc (classes of the rows), labelled classes, single_cls, batches, images per batch, (H, W), ratio_pad given, seed, mode
CASES = [
    ("nc3_rect", 3, (0, 1), False, 2, 4, (256, 320), True, 11, "normal"),
    ("nc1_square_nopad", 1, (0,), False, 2, 3, (192, 192), False, 12, "normal"),
    ("nc9_rect", 9, (0, 1, 2, 4, 5, 7, 8), False, 3, 4, (192, 256), True, 13, "normal"),
    ("single_cls", 3, (0,), True, 2, 4, (256, 256), True, 14, "normal"),
    ("no_tp", 3, (0, 1, 2), False, 1, 3, (128, 160), True, 15, "no_tp"),
]


class StubModel(torch.nn.Module):
    """What test.test() needs of a model: parameters (for the device), names, and forward(x, x2, augment)."""

    def __init__(self, nc, rows):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.names = [f"c{i}" for i in range(nc)]
        self.rows = rows                     # pre-NMS rows of each batch, in dataloader order
        self.calls = 0

    def forward(self, x, x2, augment=False):
        r = self.rows[self.calls]
        self.calls += 1
        assert r.shape[0] == x.shape[0]
        return r.clone(), None


def make_image(g, nc, lab_classes, H, W, ratio_pad_given, mode, want_labels, want_preds):
    """One image: (targets [nl, 5] = cls, x, y, w, h normalised to the letterbox, shapes entry, pre-NMS rows)."""
    h0 = int(g.integers(200, 900))
    w0 = int(g.integers(200, 900))
    r = min(H / h0, W / w0)
    padw, padh = (W - w0 * r) / 2, (H - h0 * r) / 2
    shape = ((h0, w0), ((r, r), (padw, padh))) if ratio_pad_given else ((h0, w0), None)
    # content area of the letterbox in pixels
    x0, y0, x1, y1 = padw, padh, W - padw, H - padh
    nl = int(g.integers(1, 13)) if want_labels else 0
    labels = []
    if nl:
        # two close labels of one class now and then: a prediction between them can find its best label already taken
        for k in range(nl):
            bw = float(g.uniform(0.08, 0.45)) * (x1 - x0)
            bh = float(g.uniform(0.08, 0.45)) * (y1 - y0)
            if k > 0 and g.random() < 0.3:
                pc, px, py, pw, ph = labels[-1]
                cx, cy, bw, bh = px * W + g.uniform(-0.25, 0.25) * pw * W, py * H + g.uniform(-0.25, 0.25) * ph * H, pw * W, ph * H
                c = pc
            else:
                cx = float(g.uniform(x0 + bw / 2, x1 - bw / 2))
                cy = float(g.uniform(y0 + bh / 2, y1 - bh / 2))
                c = int(g.choice(lab_classes))
            labels.append((c, cx / W, cy / H, bw / W, bh / H))
    rows = []
    if want_preds:
        for (c, cx, cy, bw, bh) in labels:
            for _ in range(int(g.integers(0, 6))):
                s = float(g.choice([0.02, 0.08, 0.2, 0.45])) if mode == "normal" else 3.0
                px = cx * W + g.normal(0, s) * bw * W
                py = cy * H + g.normal(0, s) * bh * H
                if mode == "no_tp":
                    px, py = (cx * W + 1.5 * bw * W) % W, (cy * H + 1.5 * bh * H) % H
                pw = bw * W * float(np.exp(g.normal(0, s)))
                ph = bh * H * float(np.exp(g.normal(0, s)))
                pc = c if g.random() < 0.85 else int(g.integers(0, nc))
                rows.append((px, py, pw, ph, pc, g.random() < 0.15))
        for _ in range(int(g.integers(0, 4))):                     # false positives, any class (incl. unlabelled ones)
            rows.append((float(g.uniform(0, W)), float(g.uniform(0, H)), float(g.uniform(8, W / 3)), float(g.uniform(8, H / 3)),
                         int(g.integers(0, nc)), False))
    out = []
    for (px, py, pw, ph, pc, second) in rows:
        row = np.zeros(5 + nc, np.float32)
        row[:4] = (px, py, pw, ph)
        row[4] = g.uniform(0.02, 1.0)
        row[5 + pc] = g.uniform(0.3, 1.0)
        if second and nc > 1:                                         # a second class above conf_thres (multi_label)
            row[5 + (pc + 1) % nc] = g.uniform(0.05, 0.6)
        for cc in range(nc):                                          # sub-threshold noise in the other classes
            if row[5 + cc] == 0:
                row[5 + cc] = g.uniform(0, 0.0009)
        out.append(row)
    return labels, shape, out


def make_case(name, nc, lab_classes, single_cls, nbatch, nb, hw, ratio_pad_given, seed, mode):
    g = np.random.default_rng(seed)
    H, W = hw
    batches = []
    for bi in range(nbatch):
        imgs_labels, shapes, rows = [], [], []
        for i in range(nb):
            want_labels = not (bi == 0 and i == 1)                   # one image without labels
            want_preds = not (bi == nbatch - 1 and i == nb - 1)      # one image without detections
            lab, shp, r = make_image(g, nc, lab_classes, H, W, ratio_pad_given, mode, want_labels, want_preds)
            imgs_labels.append(lab)
            shapes.append(shp)
            rows.append(r)
        R = max(8, max(len(r) for r in rows) + int(g.integers(1, 6)))   # padding rows: obj = 0 (filtered by conf_thres)
        pre = np.zeros((nb, R, 5 + nc), np.float32)
        for i, r in enumerate(rows):
            if r:
                pre[i, :len(r)] = np.stack(r)
            pre[i, len(r):, :4] = (W / 2, H / 2, 10, 10)
        # rows in random order, as a real head emits them
        for i in range(nb):
            pre[i] = pre[i][g.permutation(R)]
        tg = [(i, *l) for i, lab in enumerate(imgs_labels) for l in lab]
        targets = torch.tensor(tg, dtype=torch.float32).reshape(-1, 6)
        batches.append({"rows": torch.from_numpy(pre), "targets": targets, "shapes": shapes, "img_hw": (H, W)})
    return batches


def run_case(test, name, nc, lab_classes, single_cls, batches):
    rec = {"nms": [], "ap_in": None, "ap_out": None}
    orig_nms, orig_ap = test.non_max_suppression, test.ap_per_class

    def nms(*a, **k):
        out = orig_nms(*a, **k)
        rec["nms"].append([o.clone() for o in out])
        return out

    def ap(tp, conf, pred_cls, target_cls, **k):
        rec["ap_in"] = {"tp": torch.from_numpy(np.array(tp)), "conf": torch.from_numpy(np.array(conf)),
                        "pred_cls": torch.from_numpy(np.array(pred_cls)),
                        "target_cls": torch.from_numpy(np.array(target_cls, dtype=np.float64))}
        out = orig_ap(tp, conf, pred_cls, target_cls, **k)
        rec["ap_out"] = {k2: torch.from_numpy(np.array(v)) for k2, v in zip(("p", "r", "ap", "f1", "ap_class"), out)}
        return out

    test.non_max_suppression, test.ap_per_class = nms, ap
    try:
        model = StubModel(nc, [b["rows"] for b in batches])
        loader = []
        for b in batches:
            H, W = b["img_hw"]
            img = torch.zeros((b["rows"].shape[0], 6, H, W), dtype=torch.uint8)
            loader.append((img, b["targets"].clone(), [f"{name}_{i}.jpg" for i in range(img.shape[0])], b["shapes"]))
        results, maps, _ = test.test({"nc": nc}, batch_size=len(loader[0][2]), model=model, dataloader=loader,
                                     single_cls=single_cls, plots=False, save_dir=Path("."))
    finally:
        test.non_max_suppression, test.ap_per_class = orig_nms, orig_ap
    return rec, [float(x) for x in results[:5]], torch.from_numpy(np.array(maps, dtype=np.float64))


def main():
    make_golden.install_reference()
    import torchvision  # the stand-in module
    torchvision.ops = type(sys)("torchvision.ops")
    torchvision.ops.nms = greedy_nms
    torch.set_num_threads(os.cpu_count())
    import test  # the reference's test.py
    cases = []
    for (name, nc, lab_classes, single_cls, nbatch, nb, hw, rp, seed, mode) in CASES:
        batches = make_case(name, nc, lab_classes, single_cls, nbatch, nb, hw, rp, seed, mode)
        rec, results, maps = run_case(test, name, nc if not single_cls else 1, lab_classes, single_cls, batches)
        for b, dets in zip(batches, rec["nms"]):
            b["dets"] = dets
        confs = torch.cat([d[:, 4] for b in batches for d in b["dets"]])
        assert confs.unique().numel() == confs.numel(), f"{name}: tied confidences, pick another seed"
        if mode == "no_tp":
            assert rec["ap_in"] is None and results == [0.0] * 5, results
        else:
            assert rec["ap_in"] is not None
        cases.append({"name": name, "nc": nc, "single_cls": single_cls, "conf_thres": 0.001, "iou_thres": 0.6,
                      "batches": batches, "stats": rec["ap_in"], "ap_out": rec["ap_out"], "results": results, "maps": maps})
        print(f"{name}: {sum(len(c) for b in batches for c in b['dets'])} detections, "
              f"{sum(b['targets'].shape[0] for b in batches)} labels, results {results}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save({"cases": cases}, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
