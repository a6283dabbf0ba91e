"""Time the optimiser half of a training step - ``SGD.step()`` + ``ModelEMA.update()`` (csrc/optim.hip: one launch each) - against
``torch.optim.SGD(foreach=True).step()`` plus a per-tensor EMA loop, on the same device tensors.

    python tools/optim_bench.py [--steps 50] [--warmup 5] [--sweep]
    python tools/optim_bench.py --adam [--steps 50] [--warmup 5]

The parameter set is that of ``cft_config("l", "transformerx3", 3)`` (yolov5l + CFT x3, 206 M parameters, 1 445 state-dict
entries); the model is only a holder of tensors here, no forward runs.  Both paths step the same parameters with the same
gradients under the reference's three groups and average into the same EMA tensors, alternating step by step in one process;
every time ends in a device synchronisation and INCLUDES the host cost of the step (walking 1 000-odd parameters in Python,
comparing the table), which is also reported on its own (``host_ms``: until ``step()`` / ``update()`` return, table unchanged).
The kernels alone are timed back to back between two events (``kernel_ms``), which gives the achieved bytes per second for the
algorithmic traffic - 20 bytes per stepped element (read p, g, buf; write p, buf), 12 per averaged element (read e, m; write e) -
against the 8.0 TB/s HBM3E peak of the MI355X (6.29 TB/s is what a float4 copy reaches).  Launches per step are counted with
torch.profiler.  ``--sweep`` repeats the kernel timing for other chunk sizes and grid caps.  Prints one JSON line.

``--adam`` times ``Adam.step()`` + ``ModelEMA.update()`` instead (``cft_adam_step``: one library call, two launches), in the same way
and in the same run against two torch baselines, ``torch.optim.Adam(foreach=True)`` and ``torch.optim.Adam(fused=True)``, each plus the
per-tensor EMA loop.  The kernel time is that of both launches of the entry together (every bare call counts one more step, which
changes no timing); the traffic is 28 bytes per stepped element (read p, g, m, v; write p, m, v).  ``cft_sgd_step`` is timed in the
same run as the yardstick for bytes per second: the same access pattern with five streams instead of seven.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.models.configs import cft_config  # noqa: E402
from msod_amd.models.yolo_test import Model  # noqa: E402
from msod_amd.utils.optim import SGD, Adam, DeviceTable, param_groups  # noqa: E402
from msod_amd.utils.torch_utils import ModelEMA  # noqa: E402

HBM_PEAK = 8.0e12
HYP = dict(lr0=0.01, momentum=0.937, weight_decay=0.0005)      # data/hyp.scratch.yaml


def three_groups(cls, groups, **kw):
    opt = cls(groups[0], lr=HYP["lr0"], momentum=HYP["momentum"], nesterov=True, **kw)
    opt.add_param_group({"params": groups[1], "weight_decay": HYP["weight_decay"]})
    opt.add_param_group({"params": groups[2]})
    return opt


def torch_ema_update(ema_sd, model_sd, d):
    """ModelEMA.update as the reference writes it: per floating-point entry, scale the average and add the model's share."""
    with torch.no_grad():
        for k, v in ema_sd.items():
            if v.dtype.is_floating_point:
                v *= d
                v += (1. - d) * model_sd[k].detach()


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as ex:  # the profiler is optional here
        return f"n/a ({type(ex).__name__})"


def kernel_ms(launch, reps=10):
    """ms per launch, back to back between two events (the host side of a bare launch is far shorter than the kernel)."""
    launch()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def three_adam_groups(cls, groups, **kw):
    opt = cls(groups[0], lr=HYP["lr0"], betas=(HYP["momentum"], 0.999), **kw)                  # train.py:558
    opt.add_param_group({"params": groups[1], "weight_decay": HYP["weight_decay"]})
    opt.add_param_group({"params": groups[2]})
    return opt


def main_adam(args):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Model(cft_config("l", "transformerx3", 3)).to(dev)
    groups = param_groups(model)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for grp in groups:
        for p in grp:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    n_step = sum(p.numel() for grp in groups for p in grp)
    ema = ModelEMA(model)
    ema_sd, model_sd = ema.ema.state_dict(), model.state_dict()
    n_ema = sum(v.numel() for v in ema_sd.values() if v.dtype.is_floating_point)
    ours = three_adam_groups(Adam, groups)
    baselines = {"foreach": three_adam_groups(torch.optim.Adam, groups, foreach=True), "fused": three_adam_groups(torch.optim.Adam, groups, fused=True)}
    d = ema.decay(2000)

    def fused():
        ours.step()
        ema.update(model)

    def torch_path(opt):
        opt.step()
        torch_ema_update(ema_sd, model_sd, d)

    t_ours, t_torch, h_step, h_ema = [], {k: [] for k in baselines}, [], []
    for it in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ours.step()
        t1 = time.perf_counter()
        ema.update(model)
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        took = {}
        for k, opt in baselines.items():
            ta = time.perf_counter()
            torch_path(opt)
            torch.cuda.synchronize()
            took[k] = (time.perf_counter() - ta) * 1e3
        if it >= args.warmup:
            t_ours.append((t3 - t0) * 1e3)
            h_step.append((t1 - t0) * 1e3)
            h_ema.append((t2 - t1) * 1e3)
            for k in baselines:
                t_torch[k].append(took[k])
    uploads = (ours.table_uploads, ema._table.uploads)
    sgd = three_groups(SGD, groups)                 # the yardstick for bytes per second, on the same tensors in the same run
    sgd.step()
    k_step = kernel_ms(lambda: ours._launch(*ours._last))
    k_sgd = kernel_ms(lambda: sgd._launch(*sgd._last))
    k_ema = kernel_ms(lambda: ema._launch(d))
    med = statistics.median
    bps = {"step": 28 * n_step / (k_step * 1e-3), "sgd_step": 20 * n_step / (k_sgd * 1e-3), "ema_update": 12 * n_ema / (k_ema * 1e-3)}
    out = {"optimizer": "adam", "params": n_step, "ema_elements": n_ema, "tensors_stepped": sum(len(grp) for grp in groups),
           "ema_tensors": len(ema_sd), "steps": args.steps, "warmup": args.warmup,
           "fused_ms": med(t_ours), "fused_ms_mean": statistics.fmean(t_ours),
           "torch_foreach_ms": med(t_torch["foreach"]), "torch_foreach_ms_mean": statistics.fmean(t_torch["foreach"]),
           "torch_fused_ms": med(t_torch["fused"]), "torch_fused_ms_mean": statistics.fmean(t_torch["fused"]),
           "speedup_vs_foreach": med(t_torch["foreach"]) / med(t_ours), "speedup_vs_fused": med(t_torch["fused"]) / med(t_ours),
           "host_ms": {"step": med(h_step), "ema_update": med(h_ema)},
           "table_uploads": {"step": uploads[0], "ema_update": uploads[1]},
           "fused_launches": launches(fused), "torch_foreach_launches": launches(lambda: torch_path(baselines["foreach"])),
           "torch_fused_launches": launches(lambda: torch_path(baselines["fused"])),
           "bytes": {"step": 28 * n_step, "sgd_step": 20 * n_step, "ema_update": 12 * n_ema},
           "kernel_ms": {"step": k_step, "sgd_step": k_sgd, "ema_update": k_ema},
           "bytes_per_s": bps, "step_over_sgd_bytes_per_s": bps["step"] / bps["sgd_step"],
           "hbm_peak_bytes_per_s": HBM_PEAK, "share_of_hbm_peak": {k: v / HBM_PEAK for k, v in bps.items()}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="also time the kernels at other chunk sizes and grid caps")
    ap.add_argument("--adam", action="store_true", help="time Adam.step() against torch.optim.Adam(foreach=True) and (fused=True) instead")
    args = ap.parse_args()
    if args.steps < 50:
        ap.error("at least 50 timed steps")
    if args.adam:
        if args.sweep:
            ap.error("--sweep times the SGD and EMA kernels; run it without --adam")
        return main_adam(args)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Model(cft_config("l", "transformerx3", 3)).to(dev)
    groups = param_groups(model)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for grp in groups:
        for p in grp:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    n_step = sum(p.numel() for grp in groups for p in grp)
    ema = ModelEMA(model)
    ema_sd, model_sd = ema.ema.state_dict(), model.state_dict()
    n_ema = sum(v.numel() for v in ema_sd.values() if v.dtype.is_floating_point)
    ours, theirs = three_groups(SGD, groups), three_groups(torch.optim.SGD, groups, foreach=True)
    d = ema.decay(2000)

    def fused():
        ours.step()
        ema.update(model)

    def torch_path():
        theirs.step()
        torch_ema_update(ema_sd, model_sd, d)

    t_fused, t_torch, h_step, h_ema = [], [], [], []
    for it in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ours.step()
        t1 = time.perf_counter()
        ema.update(model)
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        torch_path()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if it >= args.warmup:
            t_fused.append((t3 - t0) * 1e3)
            t_torch.append((t4 - t3) * 1e3)
            h_step.append((t1 - t0) * 1e3)
            h_ema.append((t2 - t1) * 1e3)
    uploads = (ours.table_uploads, ema._table.uploads)

    k_step = kernel_ms(lambda: ours._launch(*ours._last))
    k_ema = kernel_ms(lambda: ema._launch(d))
    out = {"params": n_step, "ema_elements": n_ema, "tensors_stepped": sum(len(grp) for grp in groups), "ema_tensors": len(ema_sd),
           "steps": args.steps, "warmup": args.warmup,
           "fused_ms": statistics.median(t_fused), "fused_ms_mean": statistics.fmean(t_fused),
           "torch_ms": statistics.median(t_torch), "torch_ms_mean": statistics.fmean(t_torch),
           "speedup": statistics.median(t_torch) / statistics.median(t_fused),
           "host_ms": {"step": statistics.median(h_step), "ema_update": statistics.median(h_ema)},
           "table_uploads": {"step": uploads[0], "ema_update": uploads[1]},
           "fused_launches": launches(fused), "torch_launches": launches(torch_path),
           "bytes": {"step": 20 * n_step, "ema_update": 12 * n_ema},
           "kernel_ms": {"step": k_step, "ema_update": k_ema},
           "bytes_per_s": {"step": 20 * n_step / (k_step * 1e-3), "ema_update": 12 * n_ema / (k_ema * 1e-3)},
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "share_of_hbm_peak": {"step": 20 * n_step / (k_step * 1e-3) / HBM_PEAK, "ema_update": 12 * n_ema / (k_ema * 1e-3) / HBM_PEAK}}
    if args.sweep:
        sweep = []
        for chunk, cap in [(2048, 0), (8192, 0), (16384, 0), (65536, 0), (4096, 1024), (4096, 4096), (4096, 8192), (16384, 4096)]:
            ours._table, ours._max_blocks = DeviceTable(chunk), cap
            ema._table, ema._max_blocks = DeviceTable(chunk), cap
            fused()                                   # builds and uploads the tables of this cut
            ks, ke = kernel_ms(lambda: ours._launch(*ours._last)), kernel_ms(lambda: ema._launch(d))
            sweep.append({"chunk": chunk, "max_blocks": cap or 2048, "step_ms": ks, "ema_update_ms": ke,
                          "step_share": 20 * n_step / (ks * 1e-3) / HBM_PEAK, "ema_update_share": 12 * n_ema / (ke * 1e-3) / HBM_PEAK})
        out["sweep"] = sweep
    print(json.dumps(out))


if __name__ == "__main__":
    main()
