"""GPU tests of the single-stream model ``models/yolo.py``, its test-time augmentation (cft_tta_view, cft_tta_merge), checkpoint
loading, weight transfer and evaluation, against the reference's recording in tests/golden/single/ (written by
tests/golden/make_single_golden.py) and the numpy restatement in tests/tta_ref.py.  Forward tolerances are those of the two-stream
golden tests (tests/test_gpu_model.py: fp32 1e-3, fp16 1e-2 in sigmoid space, bf16 the project's 16-bit bar), train-mode ones those of
tests/test_train.py."""
import ctypes
import io
import contextlib
import os
from copy import deepcopy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tta_ref
from test_gpu_model import _check_bf16, _check_f16, _check_fp32

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SINGLE = os.path.join(HERE, "golden", "single")
DATA = os.path.join(HERE, "golden", "dataset")
CKPT = os.path.join(SINGLE, "ref_single_ckpt_tiny.pt")
FORWARD_CASES = ["s_64", "s_64_fused", "s_rect_fused", "l_64_fused"]
TTA_CASES = ["tta_96x64", "tta_64x64"]
SCALES, FLIPS = (1, 0.83, 0.67), (False, True, False)
_CACHE = {}


def golden(name):
    if name not in _CACHE:
        _CACHE[name] = torch.load(os.path.join(SINGLE, name + ".pt"), weights_only=False)
    return _CACHE[name]


def build(case, dev=None):
    """The seeded model and input of a recorded case."""
    from msod_amd.models.yolo import Model
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    model = Model(case["cfg"] + ".yaml", nc=case["nc"])
    model.load_state_dict(seeded_state_dict(model.state_dict(), case["seed"]))
    if case.get("fused"):
        model.fuse()
    x = seeded_inputs(case["batch"], case["height"], case["width"], case["seed"])[0]
    return (model.to(dev) if dev is not None else model), x


def run(model, x, dtype, **kw):
    model.set_compute_dtype(dtype)
    with torch.no_grad():
        out = model(x, **kw)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_matches_the_recording_in_every_precision(dev, name):
    g = golden(name)
    model, x = build(g["case"], dev)
    x = x.to(dev)
    for dtype, check in ((torch.float32, _check_fp32), (torch.float16, _check_f16), (torch.bfloat16, _check_bf16)):
        pred, raw = run(model, x, dtype)
        assert pred.dtype == torch.float32 and len(raw) == 3
        check(pred.cpu(), [r.float().cpu() for r in raw], g["pred"], g["raw"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_eager_and_captured_runs_agree_bit_for_bit(dev, dtype):
    g = golden("s_rect_fused")
    model, x = build(g["case"], dev)
    x = x.to(dev)
    pred, raw = run(model, x, dtype)
    pred, raw = pred.clone(), [r.clone() for r in raw]
    model.capture(*[x.shape[i] for i in (0, 2, 3)])
    assert len(model._graphs) == 1 and next(iter(model._graphs.values())).ir is None
    for _ in range(2):
        p2, r2 = run(model, x, dtype)
        assert p2 is next(iter(model._graphs.values())).pred                   # a replay, not another walk
        assert torch.equal(p2, pred) and all(torch.equal(a, b) for a, b in zip(r2, raw))


def test_one_lane_walk_and_input_forms(dev):
    """The single-stream graph has one lane (no side stream is made); uint8, fp16 and a channel slice of a six-channel batch are legal
    inputs and bad ones are refused."""
    g = golden("s_rect_fused")
    model, x = build(g["case"], dev)
    assert set(model.stream_lanes()) == {0}
    want, _ = run(model, x.to(dev), torch.float32)
    assert "_side_stream" not in model.__dict__
    six = torch.cat([torch.rand_like(x), x], 1).to(dev)
    assert six[:, 3:].stride(0) == 6 * six.stride(1)                            # a view into the six-channel batch
    assert torch.equal(run(model, six[:, 3:], torch.float32)[0], want)
    u8 = (x * 255).round().to(torch.uint8)
    p8, _ = run(model, u8.to(dev), torch.float32)
    p8f, _ = run(model, (u8.float() / 255).to(dev), torch.float32)
    assert torch.allclose(p8, p8f, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="multiples of the largest stride"):
        model(torch.zeros(1, 3, 48, 64, device=dev))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        model(six)
    with pytest.raises(TypeError, match="uint8, float16 or float32"):
        model(x.double().to(dev))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_train_mode_matches_the_recording(dev, dtype):
    """model.train(): the raw list (fp32 1e-3 on the logits, fp16 1e-2 in sigmoid space) and every running statistic (rtol 1e-4 / 2e-2),
    the bars of tests/test_train.py."""
    g = golden("s_train_64")
    model, x = build(g["case"], dev)
    model.set_compute_dtype(dtype).train()
    with torch.no_grad():
        raws = model(x.to(dev))
    torch.cuda.synchronize()
    assert isinstance(raws, list) and len(raws) == 3
    want = torch.cat([r.reshape(-1) for r in g["raw"]])
    got = torch.cat([r.float().cpu().reshape(-1) for r in raws])
    if dtype == torch.float32:
        assert (got - want).abs().max().item() <= 1e-3
    else:
        assert (got.sigmoid() - want.sigmoid()).abs().max().item() <= 1e-2
    new = model.state_dict()
    tol = {torch.float32: 1e-4, torch.float16: 2e-2}[dtype]
    for k, v in g["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert int(new[k]) == 1, k
        else:
            assert torch.allclose(new[k].float().cpu(), v, rtol=tol, atol=tol * 0.1), (k, (new[k].float().cpu() - v).abs().max())


# ------------------------------------------------------------------------------------------------ cft_tta_view
def _canaried(shape, dev):
    """An output tensor inside a larger buffer filled with a canary value."""
    n = int(np.prod(shape))
    buf = torch.full((n + 1024,), -7.0, dtype=torch.float32, device=dev)
    return buf, buf[512:512 + n].view(shape)


@pytest.mark.parametrize("name", TTA_CASES)
def test_view_kernel_equals_the_restatement_and_the_recording(dev, name):
    """fp32 input: within 1e-6 of the recorded views and equal to tests/tta_ref.py bit for bit; two runs identical; the canary around
    the output untouched.  fp16 and uint8 input and the [:, 3:6] slice of a six-channel batch: equal to the restatement on the same
    values bit for bit (and, for the slice, to the fp32 result)."""
    from msod_amd import ops
    from msod_amd.utils.seeded import seeded_inputs
    g = golden(name)
    c = g["case"]
    x = seeded_inputs(c["batch"], c["height"], c["width"], c["seed"])[0]
    six = torch.cat([torch.rand_like(x), x], 1).to(dev)
    u8 = (x * 255).round().to(torch.uint8)
    for want, ratio, flip in zip(g["views"], SCALES[1:], FLIPS[1:]):
        ref = tta_ref.view(x.numpy(), ratio, 32, flip)
        buf, out = _canaried(ref.shape, dev)
        got = ops.tta_view(x.to(dev), ratio, 32, flip, out=out)
        again = ops.tta_view(x.to(dev), ratio, 32, flip)
        torch.cuda.synchronize()
        assert got is out and torch.equal(got, again)
        assert torch.all(buf[:512] == -7.0) and torch.all(buf[512 + out.numel():] == -7.0)
        err = (got.cpu() - want).abs().max().item()
        print(name, ratio, "max |kernel - recording| =", err, " bit-equal to the restatement:", np.array_equal(got.cpu().numpy(), ref))
        assert err <= 1e-6
        assert np.array_equal(got.cpu().numpy(), ref)
        assert torch.equal(ops.tta_view(six[:, 3:6], ratio, 32, flip), got)
        half = x.half()
        assert np.array_equal(ops.tta_view(half.to(dev), ratio, 32, flip).cpu().numpy(), tta_ref.view(half.numpy(), ratio, 32, flip))
        g8 = ops.tta_view(u8.to(dev), ratio, 32, flip).cpu()
        assert np.array_equal(g8.numpy(), tta_ref.view(u8.numpy(), ratio, 32, flip))
        assert (g8 - want).abs().max().item() <= 0.5 / 255 + 1e-6                # the quantisation of the input, nothing else


def test_view_kernel_on_odd_widths_and_other_grid_sizes(dev):
    """Output widths that are no multiple of the four pixels a thread writes (gs 1, 5, 7), a ratio of 1 with a flip, more than one block."""
    from msod_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 37, 51), generator=g)
    for ratio, gs, flip in ((0.83, 1, True), (0.67, 5, False), (0.5, 7, True), (1.0, 1, True), (0.31, 3, False)):
        ref = tta_ref.view(x.numpy(), ratio, gs, flip)
        buf, out = _canaried(ref.shape, dev)
        ops.tta_view(x.to(dev), ratio, gs, flip, out=out)
        assert np.array_equal(out.cpu().numpy(), ref), (ratio, gs, flip)
        assert torch.all(buf[:512] == -7.0) and torch.all(buf[512 + out.numel():] == -7.0)
    assert torch.equal(ops.tta_view(x.to(dev), 1.0, 1, True).cpu(), x.flip(3))


# ------------------------------------------------------------------------------------------------ cft_tta_merge
@pytest.mark.parametrize("name", TTA_CASES)
def test_merge_kernel_reproduces_the_recorded_tensor_bit_for_bit(dev, name):
    from msod_amd import ops
    g = golden(name)
    preds = [p.to(dev) for p in g["preds"]]
    buf, out = _canaried(tuple(g["out"].shape), dev)
    got = ops.tta_merge(preds, SCALES, FLIPS, g["case"]["width"], out=out)
    torch.cuda.synchronize()
    assert got is out and torch.equal(got.cpu(), g["out"])
    assert torch.all(buf[:512] == -7.0) and torch.all(buf[512 + out.numel():] == -7.0)
    assert torch.equal(ops.tta_merge(preds, SCALES, FLIPS, g["case"]["width"]), got)
    assert np.array_equal(got.cpu().numpy(), tta_ref.merge([p.numpy() for p in g["preds"]], SCALES, FLIPS, g["case"]["width"]))


def test_bad_arguments_are_refused_with_the_output_untouched(dev):
    from msod_amd import _lib
    lib = _lib.load()
    EINVAL = _lib._consts["CFT_EINVAL"]
    B, n, no, H, W = 2, (252, 252, 168), 8, 96, 64
    ys = [torch.rand((B, k, no), device=dev) for k in n]
    out = torch.full((B, sum(n), no), -7.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def merge(y0=ys[0].data_ptr(), y1=ys[1].data_ptr(), y2=ys[2].data_ptr(), n1=n[1], s1=0.83, s2=0.67, mask=2, o=out.data_ptr(), total=sum(n)):
        return lib.cft_tta_merge(y0, y1, y2, B, n[0], n1, n[2], no, 1.0, s1, s2, mask, float(W), o, total, st)
    bad = {"null pointer": merge(y1=None), "null output": merge(o=None), "misaligned pointer": merge(y2=ys[2].data_ptr() + 2),
           "misaligned output": merge(o=out.data_ptr() + 1), "ratio 0": merge(s1=0.0), "ratio above 1": merge(s2=1.5),
           "rows do not add up": merge(total=sum(n) - 1), "an empty view": merge(n1=0, total=sum(n) - n[1]), "flip bit 3": merge(mask=8),
           "view inside the output": merge(y0=out.data_ptr() + 64)}
    img = torch.rand((B, 3, H, W), device=dev)
    vout = torch.full((B, 3, 96, 64), -7.0, device=dev)

    def view(im=img.data_ptr(), ratio=0.83, gs=32, flip=1, o=vout.data_ptr(), Ho=96, Wo=64, dt=2, sb=3 * H * W):
        r = ctypes.c_double(ratio)
        return lib.cft_tta_view(im, dt, B, H, W, sb, H * W, W, 1, ctypes.byref(r), gs, flip, o, Ho, Wo, st)
    bad.update({"view: null pointer": view(im=None), "view: null ratio": lib.cft_tta_view(img.data_ptr(), 2, B, H, W, 3 * H * W, H * W, W, 1, None, 32, 1,
                                                                                          vout.data_ptr(), 96, 64, st),
                "view: misaligned pointer": view(im=img.data_ptr() + 2), "view: misaligned output": view(o=vout.data_ptr() + 4),
                "view: ratio 0": view(ratio=0.0), "view: ratio above 1": view(ratio=1.01), "view: gs 0": view(gs=0), "view: flip 2": view(flip=2),
                "view: other output size": view(Ho=64), "view: unknown dtype": view(dt=3), "view: negative stride": view(sb=-1)})
    torch.cuda.synchronize()
    assert all(v == EINVAL for v in bad.values()), {k: v for k, v in bad.items() if v != EINVAL}
    assert torch.all(out == -7.0) and torch.all(vout == -7.0)
    assert merge() == 0 and view() == 0                                       # the same calls with good arguments run
    torch.cuda.synchronize()
    assert not torch.any(out == -7.0) and not torch.any(vout == -7.0)


# ------------------------------------------------------------------------------------------------ model(x, augment=True)
def _check_augmented(got, want, side, check):
    """Box columns are compared after division by the image side, so they live on the scale of the other columns."""
    got, want = got.clone(), want.clone()
    got[..., :4] /= side
    want[..., :4] /= side
    err = (got - want).abs().max().item()
    print("max |augmented - recording| (boxes / side) =", err)
    assert err <= check


@pytest.mark.parametrize("name", TTA_CASES)
def test_augmented_forward_matches_the_recording(dev, name):
    g = golden(name)
    model, x = build(g["case"], dev)
    x = x.to(dev)
    side = max(g["case"]["height"], g["case"]["width"])
    for dtype, bar in ((torch.float32, 1e-3), (torch.float16, 1e-2), (torch.bfloat16, 2.5e-2)):
        out = run(model, x, dtype, augment=True)
        assert isinstance(out, tuple) and len(out) == 2 and out[1] is None
        assert out[0].dtype == torch.float32 and out[0].shape == g["out"].shape
        _check_augmented(out[0].cpu(), g["out"], side, bar)
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train()(x, augment=True)


def test_augmented_forward_replays_its_graphs_bit_for_bit(dev):
    """Eager, then captured.  A uint8 batch at 96 x 64 needs two graphs (the uint8 input; the two fp32 views share its shape), a uint8
    batch at 128 x 96 three (the input, the 0.83 view at 128 x 96 and the 0.67 view at 96 x 96), the fp32 batch at 96 x 64 one, replayed
    three times.  Replays equal the eager run and each other, bit for bit."""
    from msod_amd import ops
    g = golden("tta_96x64")
    model, x = build(g["case"], dev)
    model.set_compute_dtype(torch.float32)
    big = (torch.rand((1, 3, 128, 96), generator=torch.Generator().manual_seed(9)) * 255).to(torch.uint8)
    for img, ngraphs in (((x * 255).round().to(torch.uint8).to(dev), 2), (big.to(dev), 3), (x.to(dev), 1)):
        B, _, H, W = img.shape
        with torch.no_grad():
            eager = model(img, augment=True)[0].clone()
        graphs = model.capture_augment(B, H, W, img.dtype)
        shapes = {(H, W, img.dtype)} | {(*ops.tta_view_size(H, W, s, 32)[1], torch.float32) for s in SCALES[1:]}
        assert len(graphs) == len(model._graphs) == len(shapes) == ngraphs
        with torch.no_grad():
            first = model(img, augment=True)[0].clone()
            second = model(img, augment=True)[0]
        torch.cuda.synchronize()
        assert torch.equal(first, eager) and torch.equal(second, first)
        model.release_graphs()


# ------------------------------------------------------------------------------------------------ checkpoints and weight transfer
def test_attempt_load_of_the_tiny_checkpoint(dev):
    import sys
    from msod_amd import compat
    from msod_amd.utils.seeded import seeded_inputs
    out = torch.load(os.path.join(SINGLE, "ref_single_ckpt_tiny_out.pt"), weights_only=False)
    try:
        model = compat.attempt_load(CKPT, map_location="cpu").to(dev)
        x = seeded_inputs(out["batch"], out["height"], out["width"], out["seed"])[0].to(dev)
        with torch.no_grad():
            pred, raw = model(x)
        _check_fp32(pred.cpu(), [r.cpu() for r in raw], out["pred"], out["raw"])
        with torch.no_grad():
            model.half()
            p16, r16 = model(x.half())
        _check_f16(p16.cpu(), [r.float().cpu() for r in r16], out["pred"], out["raw"])
        ens = compat.attempt_load([CKPT, CKPT], map_location="cpu").to(dev)
        with torch.no_grad():
            y, none = ens(x)
        n = out["pred"].shape[1]
        assert none is None and y.shape == (out["batch"], 2 * n, out["pred"].shape[2])
        assert torch.allclose(y[:, :n].cpu(), out["pred"], rtol=1e-3, atol=1e-3) and torch.equal(y[:, :n], y[:, n:])
    finally:
        for name in ("models", "models.common", "models.yolo_test", "models.yolo"):
            sys.modules.pop(name, None)


def test_load_pretrained_into_a_two_stream_model(dev):
    """The forward afterwards is bit-identical to a fresh model given the same state dict - also when the target had already run
    (packed weights) and been captured."""
    import json
    import sys
    from msod_amd.models import configs
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    from msod_amd.utils.torch_utils import load_pretrained
    with open(os.path.join(SINGLE, "pretrained_transfer.json")) as fh:
        doc = json.load(fh)
    cfg = deepcopy(configs.named_config(doc["target"]))
    cfg["width_multiple"], cfg["depth_multiple"], cfg["nc"] = doc["width_multiple"], doc["depth_multiple"], doc["nc"]
    target = Model(cfg)
    target.load_state_dict(seeded_state_dict(target.state_dict(), 31))
    target = target.to(dev).set_compute_dtype(torch.float32)
    rgb, ir = (t.to(dev) for t in seeded_inputs(1, 64, 96, 31))
    with torch.no_grad():
        before = target(rgb, ir)[0].clone()
    target.capture(1, 64, 96)
    try:
        keys = load_pretrained(target, CKPT)
    finally:
        for name in ("models", "models.common", "models.yolo_test", "models.yolo"):
            sys.modules.pop(name, None)
    assert sorted(keys) == doc["transferred"] and not target._graphs
    fresh = Model(cfg)
    fresh.load_state_dict({k: v.cpu() for k, v in target.state_dict().items()})
    fresh = fresh.to(dev).set_compute_dtype(torch.float32)
    with torch.no_grad():
        got, want = target(rgb, ir)[0], fresh(rgb, ir)[0]
    assert torch.equal(got, want) and not torch.equal(got, before)


# ------------------------------------------------------------------------------------------------ evaluate
def test_evaluate_a_single_modality_baseline(dev):
    """The ten fixture pairs (the loader keeps eight) in batches of two: 'rgb', 'ir' and augment=True run and give an EvalResult; the
    'rgb' and 'ir' results differ; 'rgb' equals feeding batch[:, :3] by hand through the model, batched_nms and DetectionEvaluator."""
    from msod_amd.evaluate import evaluate
    from msod_amd.models.yolo import Model
    from msod_amd.models.yolo_test import Model as Two
    from msod_amd.models.configs import named_config
    from msod_amd.utils import datasets as D
    from msod_amd.utils.general import batched_nms
    from msod_amd.utils.metrics import DetectionEvaluator, EvalResult
    from msod_amd.utils.seeded import seeded_state_dict
    model = Model("yolov5s.yaml", nc=1)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    model = model.to(dev)
    with contextlib.redirect_stdout(io.StringIO()):
        loader, _ = D.create_dataloader_rgb_ir(os.path.join(DATA, "rgb", "images"), os.path.join(DATA, "ir", "images"), 64, 2, 32,
                                               SimpleNamespace(single_cls=True), pad=0.5, rect=True)
    batches = [(img.clone(), t.clone(), p, s) for img, t, p, s in loader]
    assert len(batches) == 4
    results = {}
    for key, kw in (("rgb", dict(modality="rgb")), ("ir", dict(modality="ir")), ("aug", dict(modality="ir", augment=True))):
        details = {}
        out = evaluate(model, batches, 1, single_cls=True, details=details, **kw)
        assert isinstance(details["result"], EvalResult) and len(out) == 2 and len(out[0]) == 5 and details["result"].seen == 8
        results[key] = details["result"]
        print(key, out[0])
    ev = DetectionEvaluator(1, True)
    seen = []
    for img, targets, paths, shapes in batches:
        img = img.to(dev)
        rgb = img[:, :3]
        assert rgb.data_ptr() == img.data_ptr() and not rgb.is_contiguous()          # a view, not a copy
        with torch.no_grad():
            pred = model(rgb)[0]
            dets, counts = batched_nms(pred, 0.001, 0.6, multi_label=True, agnostic=True)
        ev.update(dets, counts, targets, tuple(img.shape[2:]), shapes)
        seen.append((dets.clone(), counts.clone()))
    hand = ev.compute()
    np.testing.assert_equal(results["rgb"].as_test_tuple()[0], hand.as_test_tuple()[0])
    np.testing.assert_equal(np.asarray(results["rgb"].ap), np.asarray(hand.ap))
    # the other stream gives other detections, hence another result
    with torch.no_grad():
        ir_dets, ir_counts = batched_nms(model(batches[0][0].to(dev)[:, 3:])[0], 0.001, 0.6, multi_label=True, agnostic=True)
    assert not (torch.equal(ir_dets, seen[0][0]) and torch.equal(ir_counts, seen[0][1]))
    r, i = results["rgb"], results["ir"]
    assert (r.as_test_tuple()[0], np.asarray(r.ap).tolist()) != (i.as_test_tuple()[0], np.asarray(i.ap).tolist())
    with pytest.raises(ValueError, match="modality"):
        evaluate(model, batches, 1, single_cls=True)
    two = Two(named_config("cfg2")).to(dev)
    with pytest.raises(ValueError, match="single-stream"):
        evaluate(two, batches, 1, single_cls=True, modality="ir")
    with pytest.raises(NotImplementedError, match="augmented inference is broken for two-stream models"):
        evaluate(two, batches, 1, single_cls=True, augment=True)


def test_two_stream_augment_still_raises_its_text(dev):
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    model = Model(named_config("cfg2")).to(dev)
    x = torch.zeros((1, 3, 64, 64), device=dev)
    with pytest.raises(NotImplementedError) as e:
        model(x, x, augment=True)
    assert str(e.value) == ("augmented inference is broken for two-stream models in the reference "
                            "(models/yolo_test.py:215-230 calls forward_once with one input)")
