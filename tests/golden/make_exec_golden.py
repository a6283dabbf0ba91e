"""Generate ``tests/golden/exec/``: what the model executor plans (``plans.json``, host only) and which library calls and stream
waits its walks issue (``traces.json``, needs the GPU; ``tests/launch_trace.py`` records them).

    python tests/golden/make_exec_golden.py                      # rewrites plans.json
    python tests/golden/make_exec_golden.py --gpu --commit ID    # rewrites traces.json; ID = the commit whose executor is recorded
                                   [--hashes FILE]               # also writes a sha256 of every case's output tensors to FILE

Only the public ``Model`` API is used, so the script runs unchanged on any revision: a refactor of the executor records both files at
its parent commit and must reproduce them exactly (tests/test_host_logic.py, tests/test_gpu_exec_trace.py).  The files hold data
only: lists of layer indices, entry-point names, lanes and digests of scalar arguments.
"""
import argparse
import hashlib
import json
import os
import sys
from contextlib import contextmanager

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "exec")
X3, X4 = "yolov5s_fusion_transformerx3_vedai", "yolov5s_fusion_transformer_vedai"
# the four graph structures the package knows: add fusion, one CFT block, 3 GPT blocks, 4 GPT blocks (one group without an Add)
STRUCTURES = ("cfg1", "cfg2", X3, X4)
PREFIX_ROWS = (None, 2, 3, 4)
SEED = 3


def plans(model):
    """Every plan of ``model`` in JSON form (dict keys become strings, tuples lists)."""
    return {
        "lanes": list(model.stream_lanes()),
        "concat": {str(k): list(v) for k, v in sorted(model.concat_plan().items())},
        "chain": sorted(model.chain_plan()),
        "cft": {str(k): list(v) for k, v in sorted(model.cft_fusion_plan().items())},
        "prefix": {str(r): [list(s) for s in model.prefix_segments(r)] for r in PREFIX_ROWS},
    }


def host_plans():
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    return {name: {"plain": plans(Model(named_config(name))), "nms": plans(Model(named_config(name)).nms())} for name in STRUCTURES}


# ---- traced walks: name -> what differs from (bf16, eval, every switch at its default, one plain model(x, x2)) ------------------------
# (``c3_attrs``: set on every C3 instance; ``min_rows``: ops.CHAIN_RES_MIN_ROWS during the walk)
def _x3(**kw):
    return dict(cfg=X3, shape=(4, 64, 96), **kw)


CASES = {
    "x3-two-lanes": _x3(),
    "x3-one-lane": _x3(attrs={"overlap_streams": False}),
    "x3-depth-first-two-lanes": _x3(attrs={"depth_first": (2, None)}),
    "x3-depth-first-one-lane": _x3(attrs={"depth_first": (2, None), "overlap_streams": False}),
    "x3-depth-first-3-rows": _x3(attrs={"depth_first": (2, 3)}),
    "x3-no-plan_concats": _x3(attrs={"plan_concats": False}),
    "x3-no-fuse_cft_outputs": _x3(attrs={"fuse_cft_outputs": False}),
    "x3-no-chain_convs": _x3(attrs={"chain_convs": False}),
    "x3-no-splitk": _x3(attrs={"splitk": False}),
    "x3-profile": _x3(profile=True),
    "x3-train": _x3(train=True),
    "x3-fp32": _x3(dtype=torch.float32),
    "x3-nms": _x3(nms=True),
    "cfg1": dict(cfg="cfg1", shape=(2, 64, 64)),
    "cfg2": dict(cfg="cfg2", shape=(2, 64, 64)),
    "x4": dict(cfg=X4, shape=(2, 64, 64)),
    # the only shape that reaches conv2d_chain, conv2d_chain_res and the shortcut-free pair chains (yolov5l widths)
    "cfg3-chains-two-lanes": dict(cfg="cfg3", shape=(2, 192, 256), min_rows=0),
    "cfg3-chains-one-lane": dict(cfg="cfg3", shape=(2, 192, 256), min_rows=0, attrs={"overlap_streams": False}),
    "cfg3-default-heuristic": dict(cfg="cfg3", shape=(2, 192, 256)),
    "cfg3-no-pair-chain": dict(cfg="cfg3", shape=(2, 192, 256), min_rows=0, c3_attrs={"chain_pairs": False}),
    "cfg3-chains-fp16": dict(cfg="cfg3", shape=(2, 192, 256), min_rows=0, dtype=torch.float16),
    "cfg3-chains-depth-first": dict(cfg="cfg3", shape=(4, 192, 256), min_rows=0, attrs={"depth_first": (2, None)}),
    "cfg3-no-splitk": dict(cfg="cfg3", shape=(2, 192, 256), min_rows=0, attrs={"splitk": False}),
}


def build_case(name, dev):
    """(model, x, x2, profile) of case ``name``: seeded weights and images, switches set."""
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    case = CASES[name]
    model = Model(named_config(case["cfg"]))
    model.load_state_dict(seeded_state_dict(model.state_dict(), SEED))
    model = model.to(dev).set_compute_dtype(case.get("dtype", torch.bfloat16))
    for k, v in case.get("attrs", {}).items():
        setattr(model, k, v)
    for k, v in case.get("c3_attrs", {}).items():       # an attribute of every C3 instance (a switch that not every revision's Model knows)
        for m in model.modules():
            if type(m).__name__ == "C3":
                setattr(m, k, v)
    if case.get("train"):
        model.train()
    if case.get("nms"):
        model.nms()
    rgb, ir = seeded_inputs(*case["shape"], SEED)
    return model, rgb.to(dev), ir.to(dev), bool(case.get("profile"))


@contextmanager
def chain_res_min_rows(rows):
    """``ops.CHAIN_RES_MIN_ROWS`` set to ``rows`` (None: left alone) for the duration of the block."""
    from msod_amd import ops
    saved = ops.CHAIN_RES_MIN_ROWS
    if rows is not None:
        ops.CHAIN_RES_MIN_ROWS = rows
    try:
        yield
    finally:
        ops.CHAIN_RES_MIN_ROWS = saved


def traced_forward(model, x, x2, profile=False):
    """(events, output) of one eager ``model(x, x2)``."""
    from launch_trace import recording
    from msod_amd import ops
    ops.manual_dropout_seed(SEED)         # (training walks pass a seed that counts the process's dropout calls)
    with torch.no_grad(), recording(x.device) as events:
        out = model(x, x2, profile=profile)
    torch.cuda.synchronize(x.device)
    return events, out


def run_case(name, dev):
    model, x, x2, profile = build_case(name, dev)
    with chain_res_min_rows(CASES[name].get("min_rows")):
        return traced_forward(model, x, x2, profile)


def _digest(out):
    h = hashlib.sha256()

    def walk(o):
        if isinstance(o, torch.Tensor):
            h.update(repr((tuple(o.shape), str(o.dtype))).encode())
            h.update(o.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        elif o is not None:
            for t in o:
                walk(t)
    walk(out)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--hashes", default=None)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if not args.gpu:
        with open(os.path.join(args.out, "plans.json"), "w") as fh:
            json.dump(host_plans(), fh, indent=1, sort_keys=True)
            fh.write("\n")
        return
    if not args.commit:
        ap.error("--gpu needs --commit: the file says which commit's executor it records")
    dev = torch.device("cuda:0")
    traces, hashes = {}, {}
    for name in CASES:
        events, out = run_case(name, dev)
        traces[name], hashes[name] = events, _digest(out)
        print(f"{name}: {len(events)} events, output sha256 {hashes[name][:16]}", flush=True)
    doc = {"recorded": f"on an MI355X (gfx950) at commit {args.commit}, by tests/golden/make_exec_golden.py --gpu", "cases": traces}
    with open(os.path.join(args.out, "traces.json"), "w") as fh:
        json.dump(doc, fh, indent=0)
        fh.write("\n")
    if args.hashes:
        with open(args.hashes, "w") as fh:
            json.dump(hashes, fh, indent=1)


if __name__ == "__main__":
    main()
