"""Generate ``tests/golden/optim/adam_cases.pt``: what the reference's optimiser computes behind ``--adam``, on the CPU.

Runs ONLY in the build container (needs the reference checkout at ``make_golden.REF``).  The optimiser is built and warmed up by the
reference's own statements, read from its ``train.py`` at run time and executed on the objects built here: lines 548-563 (the
parameter groups and ``optim.Adam(pg0, lr=hyp['lr0'], betas=(hyp['momentum'], 0.999))`` with ``opt.adam = True``, then the two
``add_param_group`` calls) and lines 736-744 (the warm-up).  Nothing of them is kept in this file.

    python tests/golden/make_adam_golden.py       # rewrites tests/golden/optim/adam_cases.pt

``adam``: five steps of torch.optim.Adam (CPU, single-tensor path) on ``optim_ref.SmallNet`` from ``seeded_state(net, 0)`` under the
three groups with the hyp.scratch values, the warm-up applied before each step at ni = NI[step]; gradients of step k:
``optim_ref.seeded_grads(net, k)``.  Per step: the lr / betas / eps / weight_decay of each group and, by parameter name, the
parameter, ``exp_avg``, ``exp_avg_sq`` and ``step`` after it.  The groups have no ``momentum`` key, so the warm-up moves only lr.
(In the ``optim/`` subdirectory: tests/test_oracle_golden.py and tests/test_gpu_model.py treat every ``golden/*.pt`` as a forward-pass
fixture.)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402
import optim_ref as R  # noqa: E402
from make_optim_golden import EPOCHS, HYP, NBS, NI, NW, TOTAL_BATCH_SIZE, reference_lines, warm_up  # noqa: E402

OUT = os.path.join(HERE, "optim")


def adam_of(model, hyp):
    """The reference's own statements (train.py:548-563) on ``model`` with ``opt.adam = True``; returns (optimizer, group names)."""
    scope = {"model": model, "nn": torch.nn, "optim": torch.optim, "hyp": hyp, "opt": types.SimpleNamespace(adam=True)}
    exec(reference_lines(548, 563, "pg0, pg1, pg2 = [], [], []"), scope)
    assert type(scope["optimizer"]) is torch.optim.Adam
    return scope["optimizer"], R.group_names(model, (scope["pg0"], scope["pg1"], scope["pg2"]))


def main():
    make_golden.install_reference()
    from utils.general import one_cycle  # the reference
    torch.set_num_threads(1)
    os.makedirs(OUT, exist_ok=True)

    lf = one_cycle(1, HYP["lrf"], EPOCHS)
    net = R.SmallNet()
    net.load_state_dict(R.seeded_state(net, 0))
    optimizer, groups = adam_of(net, dict(HYP))
    for g in optimizer.param_groups:
        g["foreach"] = False                                          # the single-tensor path, whatever the defaults become
    torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lf)       # sets initial_lr, as train.py:573 does
    assert all("momentum" not in g for g in optimizer.param_groups)
    epoch, steps = 0, []
    for k, ni in enumerate(NI):
        accumulate = warm_up(optimizer, ni, NW, epoch, lf, HYP)
        for n, g in R.seeded_grads(net, k).items():
            net.get_parameter(n).grad = g
        optimizer.step()
        steps.append({"ni": ni, "accumulate": float(accumulate),
                      "lr": [float(x['lr']) for x in optimizer.param_groups],
                      "betas": [tuple(float(b) for b in x['betas']) for x in optimizer.param_groups],
                      "eps": [float(x['eps']) for x in optimizer.param_groups],
                      "weight_decay": [float(x['weight_decay']) for x in optimizer.param_groups],
                      "params": {n: p.detach().clone() for n, p in net.named_parameters()},
                      "exp_avg": {n: optimizer.state[p]['exp_avg'].clone() for n, p in net.named_parameters()},
                      "exp_avg_sq": {n: optimizer.state[p]['exp_avg_sq'].clone() for n, p in net.named_parameters()},
                      "step": {n: float(optimizer.state[p]['step']) for n, p in net.named_parameters()}})
        print("adam", ni, steps[-1]["lr"], steps[-1]["betas"])
    rec = {"hyp": dict(HYP), "epochs": EPOCHS, "nbs": NBS, "total_batch_size": TOTAL_BATCH_SIZE, "nw": NW, "epoch": epoch,
           "groups": groups, "steps": steps}
    out = os.path.join(OUT, "adam_cases.pt")
    torch.save({"adam": rec}, out)
    print(f"wrote {out} ({os.path.getsize(out) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
