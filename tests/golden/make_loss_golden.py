"""Generate ``tests/golden/loss/loss_cases.pt``: the reference's own ``utils/loss.py`` ``ComputeLoss`` on synthetic heads.

Runs ONLY in the build container (needs the reference checkout next to ``make_golden.py``'s ``REF``).  The reference's
``utils/loss.py`` runs unmodified, on CPU, in float32, with one thread (the last write of ``tobj[b, a, gj, gi]`` wins in
candidate order):
  * ``make_golden.install_reference()`` stands in for the import-time-only modules (cv2, torchvision, seaborn);
  * the model is a stub ``nn.Module`` with ``hyp``, ``gr`` and ``model[-1]`` = a stub Detect (``na, nc, nl, anchors, stride``);
  * ``build_targets`` clamps its long index tensors in place with float 0-dim tensor bounds
    (``gj.clamp_(0, gain[3] - 1)``), which the torch releases of the reference's time accepted and current torch rejects;
    while the recipe runs, ``Tensor.clamp_`` on an integer tensor turns such bounds into Python ints first.  The clamp
    stays in place, so ``tbox`` (``gxy - gij``) sees the clamped ``gij`` exactly as it did then.

    python tests/golden/make_loss_golden.py       # rewrites tests/golden/loss/loss_cases.pt

Per case: the inputs (p, targets, anchors, hyp, gr), build_targets' output, loss and items, and the autograd gradient of
loss with respect to every p[i].  The last case runs the reference's ``test.test(..., compute_loss=ComputeLoss(stub))``.
(In a subdirectory: tests/test_oracle_golden.py and tests/test_gpu_model.py treat every ``golden/*.pt`` as a forward-pass fixture.)
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

OUT = os.path.join(HERE, "loss", "loss_cases.pt")
ANCHORS_PX = ((10, 13, 16, 30, 33, 23), (30, 61, 62, 45, 59, 119), (116, 90, 156, 198, 373, 326))
STRIDES = (8.0, 16.0, 32.0)
H, W = 96, 128                                     # grids 12 x 16, 6 x 8, 3 x 4
HYP = dict(box=0.05, obj=1.0, cls=0.5, cls_pw=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)

_clamp_ = torch.Tensor.clamp_


def _int_clamp_(self, min=None, max=None):
    if not self.is_floating_point():
        min = int(min) if isinstance(min, torch.Tensor) else min
        max = int(max) if isinstance(max, torch.Tensor) else max
    return _clamp_(self, min, max)


class StubDetect(torch.nn.Module):
    def __init__(self, nc):
        super().__init__()
        self.nc, self.no, self.nl, self.na = nc, nc + 5, 3, 3
        self.stride = torch.tensor(STRIDES)
        self.register_buffer("anchors", torch.tensor(ANCHORS_PX).float().view(3, 3, 2) / self.stride.view(-1, 1, 1))


class StubModel(torch.nn.Module):
    """What ComputeLoss and test.test() need of a model; forward returns the prepared (pred rows, raw list) of each batch."""

    def __init__(self, nc, hyp, gr, outputs=()):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.model = torch.nn.ModuleList([StubDetect(nc)])
        self.hyp, self.gr, self.names = dict(hyp), gr, [f"c{i}" for i in range(nc)]
        self.outputs, self.calls = list(outputs), 0

    def forward(self, x, x2, augment=False):
        rows, raws = self.outputs[self.calls]
        self.calls += 1
        return rows.clone(), [r.clone() for r in raws]


def heads(g, B, nc, scale=1.5, hw=(H, W)):
    """Random head outputs whose values are exact in float16 (stored as float16, widened to float32 exactly)."""
    return [torch.from_numpy((g.standard_normal((B, 3, hw[0] // int(s), hw[1] // int(s), nc + 5)) * scale).astype(np.float16).astype(np.float32))
            for s in STRIDES]


def pack_grad(gr):
    """A head gradient as the dense objectness channel plus the rows of the cells with any other non-zero channel."""
    flat = gr.reshape(-1, gr.shape[-1])
    other = torch.cat((flat[:, :4], flat[:, 5:]), 1)
    cells = torch.nonzero((other != 0).any(1)).reshape(-1)
    return {"shape": tuple(gr.shape), "obj": gr[..., 4].clone(), "cells": cells, "rows": flat[cells].clone()}


def unpack_grad(d):
    g = torch.zeros(d["shape"], dtype=torch.float32)
    flat = g.view(-1, d["shape"][-1])
    flat[d["cells"]] = d["rows"]
    g[..., 4] = d["obj"]
    return g


def random_targets(g, B, nt, nc, images=None, wh=(0.03, 0.5)):
    rows = []
    for _ in range(nt):
        b = int(g.choice(images)) if images is not None else int(g.integers(0, B))
        rows.append((b, int(g.integers(0, nc)), g.uniform(0.02, 0.98), g.uniform(0.02, 0.98), g.uniform(*wh), g.uniform(*wh)))
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)


def border_targets(g, B, nc):
    """x, y at grid borders, at gxy <= 1 and gxi <= 1 on every level, on .5 boundaries, at 0 and 1 (the clamp)."""
    xs = [0.0, 1.0, 0.5 / 16, 1.0 / 16, 1.5 / 16, 2.0 / 16, 14.5 / 16, 15.0 / 16, 15.49 / 16, 0.999, 1.0 / 4, 0.75, 0.12501, 0.87499]
    ys = [0.0, 1.0, 0.5 / 12, 1.0 / 12, 1.5 / 12, 11.0 / 12, 10.5 / 12, 0.999, 1.0 / 3, 2.0 / 3, 0.25, 0.5]
    rows = []
    for k, x in enumerate(xs):
        for y in ys[k % 3::3]:
            rows.append((int(g.integers(0, B)), int(g.integers(0, nc)), x, y, g.uniform(0.05, 0.4), g.uniform(0.05, 0.4)))
    return torch.tensor(rows, dtype=torch.float32)


def duplicate_targets(g, B, nc):
    """Clusters of targets in one image at nearly one position, different sizes: several candidates per (b, a, gj, gi)."""
    rows = []
    for _ in range(6):
        b, x, y = int(g.integers(0, B)), g.uniform(0.1, 0.9), g.uniform(0.1, 0.9)
        for _ in range(int(g.integers(2, 5))):
            rows.append((b, int(g.integers(0, nc)), x + g.uniform(-0.01, 0.01), y + g.uniform(-0.01, 0.01), g.uniform(0.05, 0.4),
                         g.uniform(0.05, 0.4)))
    return torch.tensor(rows, dtype=torch.float32)


def run_loss(ComputeLoss, nc, hyp, gr, p, targets, autobalance=False, calls=1):
    """calls > 1: the same ComputeLoss on successive heads (p is then a list of head lists)."""
    model = StubModel(nc, hyp, gr)
    cl = ComputeLoss(model, autobalance=autobalance)
    out = []
    for k in range(calls):
        pk = p[k] if calls > 1 else p
        pk = [t.clone().requires_grad_(True) for t in pk]
        tcls, tbox, indices, anch = cl.build_targets(pk, targets)
        loss, items = cl(pk, targets)
        loss.backward()
        for t in pk:
            assert torch.equal(unpack_grad(pack_grad(t.grad)), t.grad)
        out.append({"p": [t.detach().half() for t in pk], "loss": loss.detach().clone(), "items": items.clone(),
                    "grads": [pack_grad(t.grad) for t in pk], "balance": list(cl.balance),
                    "bt": [{"b": ix[0].clone(), "a": ix[1].clone(), "gj": ix[2].clone(), "gi": ix[3].clone(), "c": c.clone(),
                            "tbox": tb.clone(), "anch": an.clone()} for ix, c, tb, an in zip(indices, tcls, tbox, anch)]})
    return out


def main():
    make_golden.install_reference()
    import torchvision  # the stand-in module
    torchvision.ops = type(sys)("torchvision.ops")
    torchvision.ops.nms = greedy_nms
    torch.set_num_threads(1)
    torch.Tensor.clamp_ = _int_clamp_
    from utils.loss import ComputeLoss  # the reference
    import test  # the reference's test.py
    anchors = StubDetect(1).anchors.clone()
    g = np.random.default_rng(20)
    cases = []

    def add(name, nc, B, targets, hyp=HYP, gr=1.0, autobalance=False, calls=1, scale=1.5, hw=(H, W)):
        p = [heads(g, B, nc, scale, hw) for _ in range(calls)] if calls > 1 else heads(g, B, nc, scale, hw)
        rec = run_loss(ComputeLoss, nc, hyp, gr, p, targets, autobalance, calls)
        cases.append({"name": name, "nc": nc, "B": B, "targets": targets, "anchors": anchors, "hyp": dict(hyp), "gr": gr,
                      "autobalance": autobalance, "img_hw": hw, "calls": rec})
        n = [len(c["b"]) for c in rec[0]["bt"]]
        print(f"{name}: nt {targets.shape[0]}, candidates {n}, items {rec[-1]['items'].tolist()}")

    add("nc3", 3, 4, random_targets(g, 4, 30, 3))
    add("nc1", 1, 3, random_targets(g, 3, 20, 1))
    add("nc80", 80, 1, random_targets(g, 1, 12, 80), hw=(64, 64))
    add("empty", 3, 2, torch.zeros((0, 6)))
    add("images_without_targets", 3, 4, random_targets(g, 4, 16, 3, images=(0, 2)))
    add("anchor_t_fails", 3, 2, torch.tensor([[0, 1, 0.5, 0.5, 0.001, 0.001], [1, 0, 0.3, 0.6, 0.002, 0.9],
                                             [0, 2, 0.7, 0.2, 1e-4, 2e-4]], dtype=torch.float32))
    add("borders", 3, 3, border_targets(g, 3, 3))
    add("duplicates", 3, 2, duplicate_targets(g, 2, 3))
    add("hyp_variants", 3, 2, torch.cat([random_targets(g, 2, 20, 3), duplicate_targets(g, 2, 3)]),
        hyp=dict(HYP, label_smoothing=0.1, cls_pw=1.3, obj_pw=0.7, fl_gamma=1.5), gr=0.5)
    add("autobalance", 3, 2, random_targets(g, 2, 12, 3), autobalance=True, calls=3)

    # end to end: test.test with ComputeLoss on a stub whose forward returns prepared rows and raw heads
    nc, B, nbatch = 3, 2, 2
    hyp = dict(HYP)
    batches, outputs = [], []
    for bi in range(nbatch):
        tg = random_targets(g, B, 6, nc, wh=(0.1, 0.4))
        rows = np.zeros((B, 40, 5 + nc), np.float32)
        for i in range(B):
            for r in range(40):
                rows[i, r, :4] = (g.uniform(0, W), g.uniform(0, H), g.uniform(8, W / 2), g.uniform(8, H / 2))
                rows[i, r, 4] = g.uniform(0.01, 1.0)
                rows[i, r, 5 + int(g.integers(0, nc))] = g.uniform(0.3, 1.0)
        for t in tg.tolist():                      # a near-exact prediction per label, so that some are TPs
            rows[int(t[0]), int(g.integers(0, 40)), :4] = (t[2] * W, t[3] * H, t[4] * W * 1.05, t[5] * H * 0.97)
        shapes = [((int(g.integers(200, 600)), int(g.integers(200, 600))), None) for _ in range(B)]
        shapes = [((h0, w0), ((min(H / h0, W / w0),) * 2, ((W - w0 * min(H / h0, W / w0)) / 2, (H - h0 * min(H / h0, W / w0)) / 2)))
                  for (h0, w0), _ in shapes]
        raws = heads(g, B, nc)
        batches.append({"rows": torch.from_numpy(rows), "raws": [r.half() for r in raws], "targets": tg, "shapes": shapes})
        outputs.append((torch.from_numpy(rows), raws))
    model = StubModel(nc, hyp, 1.0, outputs)
    loader = [(torch.zeros((B, 6, H, W), dtype=torch.uint8), b["targets"].clone(), [f"e2e_{i}.jpg" for i in range(B)], b["shapes"])
              for b in batches]
    results, maps, _ = test.test({"nc": nc}, batch_size=B, model=model, dataloader=loader, compute_loss=ComputeLoss(model),
                                 plots=False, save_dir=Path("."))
    e2e = {"nc": nc, "hyp": hyp, "gr": 1.0, "anchors": anchors, "batches": batches, "img_hw": (H, W),
           "results": [float(x) for x in results], "maps": torch.from_numpy(np.array(maps, dtype=np.float64))}
    print(f"end_to_end: results {e2e['results']}")
    torch.Tensor.clamp_ = _clamp_
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save({"cases": cases, "end_to_end": e2e}, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
