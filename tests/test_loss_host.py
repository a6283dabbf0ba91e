"""CPU tests of the ComputeLoss port: the host restatement (tests/loss_ref.py) against the reference's own ComputeLoss recorded
in tests/golden/loss/loss_cases.pt, and the Python-side input validation of msod_amd.utils.loss."""
import os
import sys

import numpy as np
import pytest
import torch

import loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss", "loss_cases.pt")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_loss_golden import unpack_grad  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def _grad_ok(got, want):
    want = np.asarray(want, np.float64)
    tol = 1e-5 * np.abs(want) + 1e-6 * np.abs(want).max()
    return bool(np.all(np.abs(np.asarray(got, np.float64) - want) <= tol))


def test_fixture_covers_the_cases(golden):
    names = {c["name"] for c in golden["cases"]}
    assert {"nc1", "nc3", "nc80", "empty", "images_without_targets", "anchor_t_fails", "borders", "duplicates", "hyp_variants",
            "autobalance"} <= names
    assert len(next(c for c in golden["cases"] if c["name"] == "autobalance")["calls"]) == 3
    assert len(golden["end_to_end"]["results"]) == 8


def test_restatement_reproduces_reference(golden):
    for c in golden["cases"]:
        bal = [4.0, 1.0, 0.4]
        for k, call in enumerate(c["calls"]):
            what = f"{c['name']} call {k}"
            r = loss_ref.compute([t.float() for t in call["p"]], c["targets"], c["anchors"], c["hyp"], c["gr"], bal,
                                 c["autobalance"], ssi=1)
            bal = r["balance"]
            assert r["err"] == 0, what
            for bt, cd in zip(call["bt"], r["cand"]):
                for key in ("b", "a", "gj", "gi") + (("c",) if c["nc"] > 1 else ()):
                    assert np.array_equal(bt[key].numpy(), cd[key]), f"{what} {key}"
                assert np.array_equal(bt["tbox"].numpy(), cd["tbox"]), what
            want = call["items"].double().numpy()
            np.testing.assert_allclose(r["items"], want, rtol=1e-6, atol=1e-7, err_msg=what)
            assert abs(r["loss"] - call["loss"].item()) <= 1e-6 * abs(call["loss"].item()), what
            np.testing.assert_allclose(bal, call["balance"], rtol=1e-9, err_msg=what)
            for g, gd in zip(r["grads"], call["grads"]):
                assert _grad_ok(g, unpack_grad(gd).numpy()), what


def test_fixture_has_duplicates_and_clamped_cells(golden):
    """The cases the GPU's last-writer and accumulation rules are tested on really occur."""
    c = next(c for c in golden["cases"] if c["name"] == "duplicates")
    bt = c["calls"][0]["bt"][0]
    cells = list(zip(bt["b"].tolist(), bt["a"].tolist(), bt["gj"].tolist(), bt["gi"].tolist()))
    assert len(set(cells)) < len(cells)
    c = next(c for c in golden["cases"] if c["name"] == "borders")
    tb = torch.cat([bt["tbox"] for bt in c["calls"][0]["bt"]])
    assert (tb[:, :2] >= 1.0).any()          # gxy - gij with gij clamped at the far border


def test_restatement_skips_invalid_image_and_class():
    """The skip rule of tests/loss_ref.py (the package's own behaviour is tested on the GPU, and by the message test below)."""
    anchors = np.ones((1, 1, 2), np.float32)
    shapes = [(2, 1, 4, 4, 8)]
    t = np.array([[0, 1, 0.5, 0.5, 0.25, 0.25], [2, 1, 0.5, 0.5, 0.25, 0.25], [0, 5, 0.5, 0.5, 0.25, 0.25]], np.float32)
    cand, err = loss_ref.build_targets(shapes, t, anchors, 4.0, 3)
    assert err == 3
    assert set(cand[0]["b"].tolist()) == {0} and set(cand[0]["c"].tolist()) == {1}


def test_skipped_targets_message():
    import msod_amd  # noqa: F401
    from msod_amd.utils.loss import ERR_CLASS, ERR_IMAGE, skipped_targets_message
    assert skipped_targets_message(0, 3) is None
    assert "image index outside [0, batch size)" in skipped_targets_message(ERR_IMAGE, 3)
    m = skipped_targets_message(ERR_IMAGE | ERR_CLASS, 7)
    assert "image index" in m and "class outside [0, 7)" in m
    assert "unknown error bits 0x8" in skipped_targets_message(8, 3)


def test_validation_errors():
    import msod_amd  # noqa: F401
    from msod_amd.utils.loss import ComputeLoss, smooth_BCE, validate_inputs
    assert smooth_BCE(0.1) == (0.95, 0.05)
    good = [torch.zeros(2, 3, 4, 4, 8), torch.zeros(2, 3, 2, 2, 8)]
    tg = torch.zeros(0, 6)
    validate_inputs(good, tg, 2, 3, 3)
    with pytest.raises(ValueError, match="float32"):
        validate_inputs([good[0].double(), good[1]], tg, 2, 3, 3)
    with pytest.raises(ValueError, match="contiguous"):
        validate_inputs([good[0].transpose(2, 3), good[1]], tg, 2, 3, 3)
    with pytest.raises(ValueError, match="nc \\+ 5"):
        validate_inputs(good, tg, 2, 3, 4)
    with pytest.raises(ValueError, match="batch"):
        validate_inputs([good[0], torch.zeros(3, 3, 2, 2, 8)], tg, 2, 3, 3)
    with pytest.raises(ValueError, match="anchors"):
        validate_inputs([good[0], torch.zeros(2, 2, 2, 2, 8)], tg, 2, 3, 3)
    with pytest.raises(ValueError, match="list of 3"):
        validate_inputs(good, tg, 3, 3, 3)
    with pytest.raises(ValueError, match="targets"):
        validate_inputs(good, torch.zeros(4, 5), 2, 3, 3)

    class CpuModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
    with pytest.raises(RuntimeError, match="GPU"):
        ComputeLoss(CpuModel())
