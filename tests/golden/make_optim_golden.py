"""Generate ``tests/golden/optim/``: what the reference's optimiser half of a training step computes, on the CPU.

Runs ONLY in the build container (needs the reference checkout at ``make_golden.REF``); ``make_golden.install_reference()`` stands in
for the import-time-only modules.  The reference's own ``ModelEMA`` and ``one_cycle`` and its own ``Model`` run unmodified; the
parameter-group rule and the warm-up are inline statements of its ``train.py`` (:548-555, :736-744): the recipe reads those very
lines from the checkout and executes them on the objects built here.

    python tests/golden/make_optim_golden.py       # rewrites tests/golden/optim/groups.json and optim_cases.pt

  (a) groups.json: the names of the parameters in pg0 / pg1 / pg2 for yolov5s_fusion_add_vedai and yolov5s_fusion_transformerx3_vedai;
  (b) ``ema``: ModelEMA of ``optim_ref.SmallNet`` after updates 1, 2, 3 (model = seeded state k at update k) and after update 2 000
      (the counter set to 1 999, model = seeded state 4), with ``updates`` and the decay used;
  (c) ``one_cycle``: one_cycle(1, 0.2, 300) at a few epochs;
  (d) ``sgd``: five steps of torch.optim.SGD (CPU, foreach=False) under the three groups with the hyp.scratch values, the warm-up
      interpolation applied before each step at ni = NI[step]; per step the lr / momentum of each group, every parameter and every
      momentum buffer.  Gradients of step k: ``optim_ref.seeded_grads(net, k)``.
(In a subdirectory: tests/test_oracle_golden.py and tests/test_gpu_model.py treat every ``golden/*.pt`` as a forward-pass fixture.)
"""
import json
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402
import optim_ref as R  # noqa: E402

OUT = os.path.join(HERE, "optim")
CONFIGS = ("yolov5s_fusion_add_vedai", "yolov5s_fusion_transformerx3_vedai")
HYP = dict(lr0=0.01, lrf=0.2, momentum=0.937, weight_decay=0.0005, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1)   # data/hyp.scratch.yaml
EPOCHS, NBS, TOTAL_BATCH_SIZE, NW = 300, 64, 16, 1000
NI = (0, 1, 400, 800, 1000)
ONE_CYCLE_AT = (0, 1, 2, 75, 150, 151, 299, 300)


def reference_lines(first, last, starts_with):
    """Lines ``first..last`` (1-based, inclusive) of the reference's train.py, dedented; the first must start as expected."""
    with open(os.path.join(make_golden.REF, "train.py")) as fh:
        lines = fh.read().splitlines()[first - 1:last]
    text = textwrap.dedent("\n".join(lines))
    assert text.startswith(starts_with), f"train.py:{first} is not '{starts_with}...': {lines[0]!r}"
    return compile(text, f"train.py:{first}-{last}", "exec")


def groups_of(model):
    """The reference's own statements (train.py:548-555) on ``model``."""
    scope = {"model": model, "nn": torch.nn}
    exec(reference_lines(548, 555, "pg0, pg1, pg2 = [], [], []"), scope)
    return scope["pg0"], scope["pg1"], scope["pg2"]


def warm_up(optimizer, ni, nw, epoch, lf, hyp):
    """The reference's own statements (train.py:736-744); returns accumulate."""
    scope = {"optimizer": optimizer, "ni": ni, "nw": nw, "epoch": epoch, "lf": lf, "hyp": hyp, "np": np, "nbs": NBS,
             "total_batch_size": TOTAL_BATCH_SIZE}
    exec(reference_lines(736, 744, "if ni <= nw:"), scope)
    return scope["accumulate"]


def main():
    make_golden.install_reference()
    import msod_amd  # noqa: F401  (package alias; pure-python parts only)
    from msod_amd.models.configs import named_config
    from models.yolo_test import Model  # the reference
    from utils.general import one_cycle  # the reference
    from utils.torch_utils import ModelEMA  # the reference
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)

    names = {}
    for cfg in CONFIGS:
        torch.manual_seed(0)
        model = Model(named_config(cfg))
        pg = R.group_names(model, groups_of(model))
        names[cfg] = dict(zip(("pg0", "pg1", "pg2"), pg))
        grouped = {n for g in pg for n in g}
        names[cfg]["ungrouped"] = [n for n, _ in model.named_parameters() if n not in grouped]
        print(cfg, [len(g) for g in pg], "ungrouped:", names[cfg]["ungrouped"])
    with open(os.path.join(OUT, "groups.json"), "w") as fh:
        json.dump(names, fh, indent=0)

    net = R.SmallNet()
    net.load_state_dict(R.seeded_state(net, 0))
    ema = ModelEMA(net)
    rec_ema = []
    for k in (1, 2, 3, 4):
        if k == 4:
            ema.updates = 1999
        net.load_state_dict(R.seeded_state(net, k))
        ema.update(net)
        rec_ema.append({"updates": ema.updates, "decay": ema.decay(ema.updates), "model_state": k,
                        "state": {n: v.clone() for n, v in ema.ema.state_dict().items()}})
        print("ema", ema.updates, rec_ema[-1]["decay"])

    lf = one_cycle(1, HYP["lrf"], EPOCHS)
    rec_cycle = {"args": (1, HYP["lrf"], EPOCHS), "x": list(ONE_CYCLE_AT), "y": [float(lf(x)) for x in ONE_CYCLE_AT]}

    net = R.SmallNet()
    net.load_state_dict(R.seeded_state(net, 0))
    pg0, pg1, pg2 = groups_of(net)
    optimizer = torch.optim.SGD(pg0, lr=HYP['lr0'], momentum=HYP['momentum'], nesterov=True, foreach=False)
    optimizer.add_param_group({'params': pg1, 'weight_decay': HYP['weight_decay']})
    optimizer.add_param_group({'params': pg2})
    torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lf)       # sets initial_lr, as train.py:573 does
    epoch, steps = 0, []
    for k, ni in enumerate(NI):
        accumulate = warm_up(optimizer, ni, NW, epoch, lf, HYP)
        for n, g in R.seeded_grads(net, k).items():
            net.get_parameter(n).grad = g
        optimizer.step()
        steps.append({"ni": ni, "accumulate": float(accumulate),
                      "lr": [float(x['lr']) for x in optimizer.param_groups], "momentum": [float(x['momentum']) for x in optimizer.param_groups],
                      "weight_decay": [float(x['weight_decay']) for x in optimizer.param_groups],
                      "params": {n: p.detach().clone() for n, p in net.named_parameters()},
                      "buffers": {n: optimizer.state[p]['momentum_buffer'].clone() for n, p in net.named_parameters()}})
        print("sgd", ni, steps[-1]["lr"], steps[-1]["momentum"])
    rec_sgd = {"hyp": dict(HYP), "epochs": EPOCHS, "nbs": NBS, "total_batch_size": TOTAL_BATCH_SIZE, "nw": NW, "epoch": epoch,
               "groups": R.group_names(net, (pg0, pg1, pg2)), "steps": steps}

    out = os.path.join(OUT, "optim_cases.pt")
    torch.save({"ema": rec_ema, "one_cycle": rec_cycle, "sgd": rec_sgd}, out)
    print(f"wrote {out} ({os.path.getsize(out) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
