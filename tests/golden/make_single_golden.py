"""Generate the fixtures of the single-stream model under tests/golden/single/.

Runs only where the reference tree is present, on the CPU.  It imports the reference's own ``models.yolo.Model`` unmodified, with
the same empty stand-ins for cv2 / torchvision / seaborn that make_golden.py uses, takes weights and inputs from
``utils/seeded.py`` (so the files hold outputs only) and records:

    reference_single_configs.json   the four stock yamls: the layer table the reference logs while it parses (i, f, type, np, args),
                                    ``save``, the measured strides, the anchors after division, the state-dict layout
    <case>.pt                       forward cases: pred, the raw list and tap_stats of the saved layers; one model.train() case
    tta_<shape>.pt                  forward(x, augment=True): every view's image, every view's forward_once prediction before the
                                    fix-ups, and the returned tensor; and which division the CPU's in-place ``/=`` performed
    ref_single_ckpt_tiny.pt         a checkpoint as train.py writes one, pickled by the reference's classes; *_out.pt its outputs
    pretrained_transfer.json        the keys the reference's intersect_dicts moves from that checkpoint into the two-stream
                                    yolov5s_fusion_transformerx3_vedai network of the same width and depth

    python tests/golden/make_single_golden.py
"""
import ast
import copy
import json
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "single")
REF = "/root/reference"

# name, stock yaml, nc (None: the yaml's 80), batch, H, W, fused, seed
CASES = [
    ("s_64", "yolov5s", 3, 2, 64, 64, False, 20),
    ("s_64_fused", "yolov5s", 3, 2, 64, 64, True, 20),
    ("s_rect_fused", "yolov5s", 3, 1, 96, 64, True, 21),
    ("l_64_fused", "yolov5l", None, 1, 64, 64, True, 22),
]
TRAIN_CASE = ("s_train_64", "yolov5s", 3, 2, 64, 64, 23)
TTA_CASES = [("tta_96x64", 2, 96, 64, 24), ("tta_64x64", 1, 64, 64, 25)]     # yolov5s, nc 3, fused
# 8..128 channels (hidden C3 widths down to 8, the smallest the 16-byte-granule kernels take) and C3 depths 1 / 2 / 2 / 1: under 1 MiB
TINY_WIDTH, TINY_DEPTH, TINY_SEED = 0.125, 0.17, 26


class _TableHandler(logging.Handler):
    """parse_model logs one pre-formatted line per layer - columns of 3, 18, 3 and 10 characters, two spaces, 40 characters of type,
    then the argument list: cut it at those columns."""

    def __init__(self):
        super().__init__()
        self.rows = []

    def emit(self, record):
        msg = record.getMessage()
        if len(msg) < 77 or not msg[:3].strip().isdigit():
            return
        self.rows.append({"i": int(msg[0:3]), "f": ast.literal_eval(msg[3:21].strip()), "n": int(msg[21:24]), "np": int(float(msg[24:34])),
                          "type": msg[36:76].strip(), "args": ast.literal_eval(msg[76:].strip())})


def install_reference():
    for name in ("cv2", "torchvision", "seaborn"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["cv2"].setNumThreads = lambda n: None
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)


def build(Model, yaml_name, nc, seed, seeded_state_dict):
    torch.manual_seed(0)
    model = Model(os.path.join(REF, "models", yaml_name + ".yaml"), nc=nc)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed))
    return model


def main():
    install_reference()
    import msod_amd  # noqa: F401  (package alias; pure-python parts only)
    from make_golden import tap_stats
    from msod_amd.models.configs import named_config, stock_config
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    import models.yolo as ref_yolo  # the reference
    from models.yolo import Model
    from models.yolo_test import Model as TwoStream
    from utils.torch_utils import intersect_dicts

    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(min(16, os.cpu_count()))
    devnull = open(os.devnull, "w")
    stdout = sys.stdout

    # ---- the parsed tables -----------------------------------------------------------------------------------------
    table = _TableHandler()
    ref_yolo.logger.addHandler(table)
    ref_yolo.logger.setLevel(logging.INFO)
    ref_yolo.logger.propagate = False
    configs = {}
    for name in ("yolov5s", "yolov5m", "yolov5l", "yolov5x"):
        table.rows = []
        sys.stdout = devnull                       # the constructor prints the yaml
        try:
            m = Model(os.path.join(REF, "models", name + ".yaml"))
        finally:
            sys.stdout = stdout
        det = m.model[-1]
        configs[name] = {"layers": table.rows, "save": list(m.save), "stride": m.stride.tolist(), "anchors": det.anchors.tolist(),
                         "anchor_grid": det.anchor_grid.view(det.nl, -1, 2).tolist(),
                         "state_dict": sorted([k, list(v.shape)] for k, v in m.state_dict().items())}
        print(f"{name}: {len(table.rows)} layers, strides {m.stride.tolist()}, {len(configs[name]['state_dict'])} state-dict entries")
    ref_yolo.logger.removeHandler(table)
    logging.disable(logging.CRITICAL)
    with open(os.path.join(OUT, "reference_single_configs.json"), "w") as fh:
        json.dump(configs, fh, indent=0)
        fh.write("\n")
    sys.stdout = devnull

    def say(*a):
        print(*a, file=stdout)

    # ---- forward cases ---------------------------------------------------------------------------------------------
    for name, yaml_name, nc, b, h, w, fused, seed in CASES:
        model = build(Model, yaml_name, nc, seed, seeded_state_dict).eval()
        if fused:
            model.fuse()
        x = seeded_inputs(b, h, w, seed)[0]
        taps, hooks = {}, []
        for i, m in enumerate(model.model):
            if i in model.save and type(m).__name__ != "Detect":
                hooks.append(m.register_forward_hook(lambda mod, inp, out, i=i: taps.__setitem__(i, tap_stats(out))))
        with torch.no_grad():
            pred, raw = model(x)
        for hk in hooks:
            hk.remove()
        path = os.path.join(OUT, name + ".pt")
        torch.save({"case": dict(name=name, cfg=yaml_name, nc=nc, batch=b, height=h, width=w, fused=fused, seed=seed), "torch": torch.__version__,
                    "pred": pred.clone(), "raw": [r.clone() for r in raw], "taps": taps}, path)
        say(f"{name:14s} pred {tuple(pred.shape)} raw std {raw[0].std():.3f} -> {os.path.getsize(path) / 1e3:.0f} kB")

    # ---- model.train() ---------------------------------------------------------------------------------------------
    name, yaml_name, nc, b, h, w, seed = TRAIN_CASE
    model = build(Model, yaml_name, nc, seed, seeded_state_dict)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    with torch.no_grad():
        raws = model(seeded_inputs(b, h, w, seed)[0])
    assert isinstance(raws, list) and len(raws) == 3
    stats = {k: v.clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    path = os.path.join(OUT, name + ".pt")
    torch.save({"case": dict(name=name, cfg=yaml_name, nc=nc, batch=b, height=h, width=w, seed=seed, train=True), "torch": torch.__version__,
                "raw": [r.clone() for r in raws], "stats": stats}, path)
    say(f"{name:14s} raw {[tuple(r.shape) for r in raws]} std {raws[0].std():.3f}, {len(stats)} statistics -> {os.path.getsize(path) / 1e3:.0f} kB")

    # ---- test-time augmentation ------------------------------------------------------------------------------------
    for name, b, h, w, seed in TTA_CASES:
        model = build(Model, "yolov5s", 3, seed, seeded_state_dict).eval().fuse()
        x = seeded_inputs(b, h, w, seed)[0]
        views, preds, inner = [], [], model.forward_once

        def recording(xi, *a, **k):
            out = inner(xi, *a, **k)
            views.append(xi.clone())
            preds.append(out[0].clone())              # before the caller de-scales it in place
            return out
        model.forward_once = recording
        with torch.no_grad():
            out, none = model(x, augment=True)
        del model.forward_once
        assert none is None and len(views) == 3 and torch.equal(views[0], x)
        # which arithmetic did the in-place `/=` of a Python scalar perform?  IEEE division by (float)s, or a product with 1 / s
        rows, at, rule = [p.shape[1] for p in preds], 0, {"divide": True, "reciprocal": True}
        for p, s in zip(preds, (1, 0.83, 0.67)):
            got = out[:, at:at + p.shape[1], 2:4].numpy()             # w, h: divided, never mirrored
            src = p[..., 2:4].numpy()
            rule["divide"] &= bool(np.array_equal(got, src / np.float32(s)))
            rule["reciprocal"] &= bool(np.array_equal(got, src * (np.float32(1) / np.float32(s))))
            at += p.shape[1]
        path = os.path.join(OUT, name + ".pt")
        torch.save({"case": dict(name=name, cfg="yolov5s", nc=3, batch=b, height=h, width=w, fused=True, seed=seed), "torch": torch.__version__,
                    "views": views[1:], "view_shapes": [tuple(v.shape) for v in views], "preds": preds, "out": out.clone(), "division": rule}, path)
        say(f"{name:14s} views {[tuple(v.shape[2:]) for v in views]} rows {rows} division {rule} -> {os.path.getsize(path) / 1e3:.0f} kB")

    # ---- a tiny pickled checkpoint and what transfers from it ------------------------------------------------------
    cfg = stock_config("yolov5s", nc=3)
    cfg["width_multiple"], cfg["depth_multiple"] = TINY_WIDTH, TINY_DEPTH
    torch.manual_seed(0)
    model = Model(copy.deepcopy(cfg)).eval()
    model.load_state_dict(seeded_state_dict(model.state_dict(), TINY_SEED))
    model.names = ["person", "car", "bicycle"]
    ck = {"epoch": 3, "best_fitness": 0.25, "training_results": None, "model": copy.deepcopy(model).half(), "ema": None, "optimizer": None,
          "wandb_id": None}
    path = os.path.join(OUT, "ref_single_ckpt_tiny.pt")
    torch.save(ck, path)
    loaded = torch.load(path, map_location="cpu", weights_only=False)["model"].float().fuse().eval()
    x = seeded_inputs(2, 64, 96, TINY_SEED)[0]
    with torch.no_grad():
        pred, raw = loaded(x)
    torch.save({"cfg": cfg, "seed": TINY_SEED, "batch": 2, "height": 64, "width": 96, "pred": pred.clone(), "raw": [r.clone() for r in raw],
                "names": loaded.names, "stride": loaded.stride.clone()}, os.path.join(OUT, "ref_single_ckpt_tiny_out.pt"))
    say(f"ref_single_ckpt_tiny.pt {os.path.getsize(path) / 1e3:.0f} kB, pred {tuple(pred.shape)}, raw std {raw[0].std():.3f}")

    two = copy.deepcopy(named_config("yolov5s_fusion_transformerx3_vedai"))
    two["width_multiple"], two["depth_multiple"], two["nc"] = TINY_WIDTH, TINY_DEPTH, 3
    torch.manual_seed(0)
    target = TwoStream(two)
    src = torch.load(path, map_location="cpu", weights_only=False)["model"].float().state_dict()
    moved = intersect_dicts(src, target.state_dict(), exclude=["anchor"])
    with open(os.path.join(OUT, "pretrained_transfer.json"), "w") as fh:
        json.dump({"target": "yolov5s_fusion_transformerx3_vedai", "width_multiple": TINY_WIDTH, "depth_multiple": TINY_DEPTH, "nc": 3, "exclude": ["anchor"],
                   "source_entries": len(src), "target_entries": len(target.state_dict()), "transferred": sorted(moved)}, fh, indent=0)
        fh.write("\n")
    say(f"pretrained_transfer.json: {len(moved)} of {len(target.state_dict())} entries transfer")
    sys.stdout = stdout


if __name__ == "__main__":
    main()
