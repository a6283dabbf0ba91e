"""Host tests (no GPU) of the single-stream model ``models/yolo.py``: the four stock yamls against the reference's recorded tables,
strides, anchors and state-dict layout (tests/golden/single/, written by tests/golden/make_single_golden.py), the ``models.yolo``
alias and the pickled checkpoint, the weight transfer, the restatement of the two test-time-augmentation kernels against the
reference's recording, and the ABI of the two entry points.  (The entry points' host guards have their own stand-alone program,
tools/micro/tta_guards.hip, built with host ASan + UBSan and run by hand on the CPU.)"""
import ctypes
import json
import os
import sys
from copy import deepcopy

import numpy as np
import pytest
import torch

import tta_ref

import msod_amd  # noqa: F401
from msod_amd import _lib
from msod_amd.models import configs
from msod_amd.models import yolo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SINGLE = os.path.join(HERE, "golden", "single")
CKPT = os.path.join(SINGLE, "ref_single_ckpt_tiny.pt")
TWO_CKPT = os.path.join(HERE, "golden", "ref_ckpt_tiny.pt")
ALIASES = ("models", "models.common", "models.yolo_test", "models.yolo")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(SINGLE, "reference_single_configs.json")) as fh:
        return json.load(fh)


@pytest.fixture()
def aliases():
    yield
    for name in ALIASES:
        sys.modules.pop(name, None)


def _json(v):
    return json.loads(json.dumps(v))


# ------------------------------------------------------------------------------------------------ parsing, strides, layout
@pytest.mark.parametrize("name", sorted(configs.STOCK_YAMLS))
def test_stock_yaml_parses_to_the_recorded_table(recorded, name):
    want = recorded[name]
    rows = []
    layers, save = yolo.parse_model(deepcopy(configs.stock_config(name)), [3], rows=rows)
    assert len(rows) == len(want["layers"]) == 25 and save == want["save"]
    for (i, f, n, np_, t, args), w in zip(rows, want["layers"]):
        assert (i, _json(f), n, np_, t, _json(args)) == (w["i"], w["f"], w["n"], w["np"], w["type"], w["args"]), (name, i)
    for m, w in zip(layers, want["layers"]):
        assert (m.i, _json(m.f), m.type, m.np) == (w["i"], w["f"], w["type"], w["np"])


@pytest.mark.parametrize("name", sorted(configs.STOCK_YAMLS))
def test_strides_anchors_and_state_dict_equal_the_recording(recorded, name):
    want = recorded[name]
    model = yolo.Model(name + ".yaml")
    assert model.inputs == 1 and model.yaml["nc"] == 80 and model.names == [str(i) for i in range(80)] and model.save == want["save"]
    det = model.model[-1]
    assert model.stride.tolist() == want["stride"] == [8.0, 16.0, 32.0] and model.stride is det.stride and model.stride.dtype == torch.float32
    assert det.anchors.tolist() == want["anchors"]                              # divided by the derived strides; check_anchor_order kept the order
    assert det.anchor_grid.view(det.nl, -1, 2).tolist() == want["anchor_grid"]
    assert sorted([k, list(v.shape)] for k, v in model.state_dict().items()) == want["state_dict"]
    assert yolo.graph_strides(model.model) == [8.0, 16.0, 32.0]


def test_strides_follow_the_graph_not_a_constant():
    """A head that reads P2 / P3 / P4 instead: the derivation gives 4 / 8 / 16, and an inconsistent Concat is refused."""
    cfg = configs.stock_config("yolov5s", nc=2)
    cfg["head"][-1][0] = [2, 4, 6]
    cfg["anchors"] = 3
    assert yolo.Model(cfg).stride.tolist() == [4.0, 8.0, 16.0]
    bad = configs.stock_config("yolov5s", nc=2)
    bad["head"][2][0] = [-1, 4]                      # the upsampled P5 lateral joined with P3
    with pytest.raises(ValueError, match="different strides"):
        yolo.Model(bad)


def test_focus_takes_the_graphs_channels():
    """models/yolo.py:229 gives Focus ``ch[f]`` input channels; the two-stream file forces 3."""
    from msod_amd.models import yolo_test
    d = configs.stock_config("yolov5s")
    assert yolo.parse_model(deepcopy(d), [6])[0][0].conv.conv.in_channels == 24
    assert yolo_test.parse_model(deepcopy(d), [6])[0][0].conv.conv.in_channels == 12
    assert len(yolo_test.parse_model.__code__.co_varnames[:yolo_test.parse_model.__code__.co_argcount]) == 2        # the two-stream parser as it was


@pytest.mark.parametrize("cls", ["BottleneckCSP", "C3TR", "DWConv", "Bottleneck", "GPT", "Add"])
def test_a_yaml_naming_another_class_raises(cls):
    cfg = configs.stock_config("yolov5s")
    cfg["backbone"][2][2] = cls
    with pytest.raises(NotImplementedError, match=cls):
        yolo.Model(cfg)


def test_autoshape_is_refused():
    with pytest.raises(NotImplementedError, match="autoShape"):
        yolo.Model("yolov5s.yaml").autoshape()


def test_two_stream_model_is_still_its_own_class():
    from msod_amd.models import yolo_test
    m = yolo_test.Model(configs.named_config("cfg1"))
    assert type(m).__module__.endswith("yolo_test") and not isinstance(m, yolo.Model) and m.stride.tolist() == [8.0, 16.0, 32.0]
    assert issubclass(yolo.Model, yolo_test.Model) and "_run_layer" not in vars(yolo.Model) and "capture" not in vars(yolo.Model)      # one executor
    with pytest.raises(NotImplementedError, match="augmented inference is broken for two-stream models"):
        m(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), augment=True)


# ------------------------------------------------------------------------------------------------ checkpoints and weight transfer
def test_alias_resolves_models_yolo(aliases):
    from msod_amd import compat
    compat.install_reference_aliases()
    import models.yolo as alias
    from models.yolo import Detect, Model
    assert alias is yolo and Model is yolo.Model and Detect is yolo.Detect and sys.modules["models"].yolo is yolo


def test_tiny_checkpoint_unpickles_into_this_package(aliases):
    from msod_amd import compat
    from msod_amd.models import common
    out = torch.load(os.path.join(SINGLE, "ref_single_ckpt_tiny_out.pt"), weights_only=False)
    assert os.path.getsize(CKPT) < 1 << 20
    compat.install_reference_aliases()
    raw = torch.load(CKPT, map_location="cpu", weights_only=False)["model"]
    assert type(raw) is yolo.Model and type(raw.model[-1]) is yolo.Detect and type(raw.model[0]) is common.Focus
    assert raw.compute_dtype == torch.float16 and raw._graphs == {}                  # __setstate__: the precision its weights carry
    model = compat.attempt_load(CKPT, map_location="cpu")
    assert type(model) is yolo.Model and model.inputs == 1 and not model.training and model.compute_dtype == torch.float32
    assert model.names == out["names"] and torch.equal(model.stride, out["stride"])
    assert not any(hasattr(m, "bn") for m in model.modules() if type(m) is common.Conv)          # fused
    assert type(model.model[11]) is common.Upsample and model.model[11].f == -1
    fresh = yolo.Model(out["cfg"])
    assert {k: tuple(v.shape) for k, v in fresh.fuse().state_dict().items()} == {k: tuple(v.shape) for k, v in model.state_dict().items()}
    ens = compat.attempt_load([CKPT, CKPT], map_location="cpu")
    assert type(ens).__name__ == "Ensemble" and len(ens) == 2 and ens.names == out["names"]
    assert list(ens.forward.__code__.co_varnames[:3]) == ["self", "x", "augment"]


def test_mixed_checkpoint_list_raises_and_names_both_files(aliases):
    from msod_amd import compat
    with pytest.raises(ValueError) as e:
        compat.attempt_load([CKPT, TWO_CKPT], map_location="cpu")
    assert CKPT in str(e.value) and TWO_CKPT in str(e.value)


def _two_stream_target(doc):
    from msod_amd.models.yolo_test import Model
    cfg = deepcopy(configs.named_config(doc["target"]))
    cfg["width_multiple"], cfg["depth_multiple"], cfg["nc"] = doc["width_multiple"], doc["depth_multiple"], doc["nc"]
    return Model(cfg)


def test_load_pretrained_transfers_exactly_the_recorded_keys(aliases):
    from msod_amd.utils.torch_utils import intersect_dicts, load_pretrained
    with open(os.path.join(SINGLE, "pretrained_transfer.json")) as fh:
        doc = json.load(fh)
    target = _two_stream_target(doc)
    assert len(target.state_dict()) == doc["target_entries"]
    before = {k: v.clone() for k, v in target.state_dict().items()}
    target.__dict__["_wlist"] = "stale"                                     # a cache invalidate_packed drops
    keys = load_pretrained(target, CKPT, exclude=tuple(doc["exclude"]))
    assert sorted(keys) == doc["transferred"] and "_wlist" not in target.__dict__
    src = {k: v.float() for k, v in torch.load(CKPT, map_location="cpu", weights_only=False)["model"].state_dict().items()}
    assert len(src) == doc["source_entries"]
    for k, v in target.state_dict().items():
        assert torch.equal(v, src[k] if k in keys else before[k]), k
    assert not any("anchor" in k for k in keys)
    # the helper itself: key, shape and exclusion
    da = {"a": torch.zeros(2), "b": torch.zeros(3), "anchors": torch.zeros(1), "c": torch.zeros(1)}
    db = {"a": torch.ones(2), "b": torch.ones(4), "anchors": torch.ones(1)}
    assert list(intersect_dicts(da, db)) == ["a", "anchors"] and list(intersect_dicts(da, db, exclude=("anchor",))) == ["a"]
    # a single-stream target takes everything but the anchors
    single = yolo.Model(torch.load(os.path.join(SINGLE, "ref_single_ckpt_tiny_out.pt"), weights_only=False)["cfg"])
    assert len(load_pretrained(single, CKPT)) == len(src) - 2


# ------------------------------------------------------------------------------------------------ test-time augmentation
@pytest.fixture(scope="module", params=["tta_96x64", "tta_64x64"])
def tta_case(request):
    from msod_amd.utils.seeded import seeded_inputs
    g = torch.load(os.path.join(SINGLE, request.param + ".pt"), weights_only=False)
    c = g["case"]
    return g, seeded_inputs(c["batch"], c["height"], c["width"], c["seed"])[0]


def test_view_sizes_of_the_recorded_cases():
    """0.83 and 0.67 of 96 x 64: 79 x 53 and 64 x 42, odd sizes, padded on both axes - both to 96 x 64, because 96 * 0.67 = 64.32 is just
    above two grid cells (ceil(64.32 / 32) = 3); of 64 x 64: 53 and 42, padded to 64."""
    assert tta_ref.sizes(96, 64, 0.83, 32) == ((79, 53), (96, 64)) and tta_ref.sizes(96, 64, 0.67, 32) == ((64, 42), (96, 64))
    assert tta_ref.sizes(64, 64, 0.83, 32) == ((53, 53), (64, 64)) and tta_ref.sizes(64, 64, 0.67, 32) == ((42, 42), (64, 64))
    assert tta_ref.sizes(640, 640, 0.83, 32) == ((531, 531), (544, 544)) and tta_ref.sizes(640, 640, 0.67, 32) == ((428, 428), (448, 448))
    from msod_amd import ops
    for args in ((96, 64, 0.83, 32), (640, 512, 0.67, 32), (64, 64, 0.67, 64)):
        assert ops.tta_view_size(*args) == tta_ref.sizes(*args)


def test_restated_views_reproduce_the_recording(tta_case):
    """Within 1e-6 absolute: values lie in [0, 1] and each output passes through at most about 16 roundings of 2^-24 (torch's CPU kernel
    may contract a product and a sum; the restatement never does)."""
    g, x = tta_case
    assert g["division"] == {"divide": True, "reciprocal": False}
    for want, ratio, flip in zip(g["views"], (0.83, 0.67), (True, False)):
        got = tta_ref.view(x.numpy(), ratio, 32, flip)
        assert got.shape == tuple(want.shape) and got.dtype == np.float32
        err = np.abs(got - want.numpy()).max()
        print(g["case"]["name"], ratio, "max |view - recording| =", err)
        assert err <= 1e-6
        (hs, ws), _ = tta_ref.sizes(x.shape[2], x.shape[3], ratio, 32)
        assert np.all(got[:, :, hs:] == np.float32(0.447)) and np.all(got[:, :, :, ws:] == np.float32(0.447))


def test_restated_merge_reproduces_the_recording_bit_for_bit(tta_case):
    g, x = tta_case
    got = tta_ref.merge([p.numpy() for p in g["preds"]], (1, 0.83, 0.67), (False, True, False), x.shape[3])
    assert got.dtype == np.float32 and np.array_equal(got, g["out"].numpy())


def test_restated_view_normalises_uint8_and_half():
    g = np.random.default_rng(5)
    u8 = g.integers(0, 256, (1, 3, 32, 64), dtype=np.uint8)
    assert np.array_equal(tta_ref.view(u8, 0.67, 32), tta_ref.view(u8.astype(np.float32) / np.float32(255), 0.67, 32))
    h = g.random((1, 3, 32, 64)).astype(np.float16)
    assert np.array_equal(tta_ref.view(h, 0.83, 32, True), tta_ref.view(h.astype(np.float32)[..., ::-1], 0.83, 32))


def test_header_and_wrappers_agree():
    c = _lib._consts
    assert (c["CFT_TTA_U8"], c["CFT_TTA_F16"], c["CFT_TTA_F32"]) == (0, 1, 2)
    i, l, f, v = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    assert _lib.SIGNATURES["cft_tta_view"] == (i, [v, i, i, i, i, l, l, l, l, v, i, i, v, i, i, v])
    assert _lib.SIGNATURES["cft_tta_merge"] == (i, [v, v, v, i, i, i, i, i, f, f, f, i, f, v, i, v])
    assert "tta.hip" in _lib.SOURCES and not _lib.missing_symbols()
    lib = _lib.load()
    assert lib.cft_tta_view.argtypes == _lib.SIGNATURES["cft_tta_view"][1]
    # the wrappers refuse what they can see without a device
    from msod_amd import ops
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.tta_view(torch.zeros(1, 3, 32, 32), 0.83, 32)
    with pytest.raises(ValueError, match="three views"):
        ops.tta_merge([torch.zeros(1, 4, 8)], (1,), (False,), 32)


# ------------------------------------------------------------------------------------------------ evaluate / val
def test_evaluate_modality_rules_come_before_any_device_work():
    from msod_amd.evaluate import evaluate
    from msod_amd.models.yolo_test import Model as Two
    single = yolo.Model("yolov5s.yaml", nc=1)
    with pytest.raises(ValueError, match="modality='rgb' or 'ir'"):
        evaluate(single, [], 1)
    with pytest.raises(ValueError, match="modality"):
        evaluate(single, [], 1, modality="thermal")
    with pytest.raises(ValueError, match="no raw outputs"):
        evaluate(single, [], 1, modality="ir", augment=True, compute_loss=object())
    with pytest.raises(ValueError, match="single-stream"):
        evaluate(Two(configs.named_config("cfg1")), [], 1, modality="rgb")
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        evaluate(single, [], 1, modality="rgb")                                   # accepted; this package has no CPU path
