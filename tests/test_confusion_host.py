"""Host tests of the confusion matrix and the save_txt / save_json formats: tests/confusion_ref.py (a restatement from the rules)
and the package's formatters against the reference's own results in tests/golden/eval/confusion_cases.pt."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import confusion_ref
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "confusion_cases.pt")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLDEN, weights_only=False)["cases"]


def _nc(case):
    return 1 if case["single_cls"] else case["nc"]


def test_golden_is_data_and_covers_the_quirks(cases):
    assert os.path.getsize(GOLDEN) < 1 << 20
    names = [c["name"] for c in cases]
    assert names == ["nc3_rect", "nc1_square_nopad", "nc9_rect", "single_cls", "no_tp", "constructed"]
    con = cases[-1]
    pb = con["process_batch"]
    assert len(pb[0][0]) and not (pb[0][0][:, 4] > 0.25).any()             # labels and detections, none above 0.25
    m2, _ = confusion_ref.process_image(pb[2][0].numpy(), pb[2][1].numpy(), 3)
    assert (pb[2][0][:, 4] > 0.25).sum() >= 2 and m2[:3, :].sum() == 0 and m2[3, :3].sum() == len(pb[2][1])     # the `if n:` quirk
    m1, _ = confusion_ref.process_image(pb[1][0].numpy(), pb[1][1].numpy(), 3)
    assert m1[:3, :3].sum() >= 2 and m1[:3, 3].sum() >= 3                  # matches and leftover detections


def test_restatement_reproduces_reference_matrices(cases):
    for case in cases:
        nc, want = _nc(case), case["matrix"].numpy()
        # from the inputs the reference handed to process_batch
        m = np.zeros((nc + 1, nc + 1), np.int64)
        for det, lab in case["process_batch"]:
            mi, bad = confusion_ref.process_image(det.numpy(), lab.numpy(), nc, single_cls=case["single_cls"])
            assert bad == 0
            m += mi
        assert np.array_equal(m.astype(np.float64), want), case["name"]
        # and from the NMS output and the dataloader's targets (the transforms restated too)
        m = np.zeros((nc + 1, nc + 1), np.int64)
        for b in case["batches"]:
            mi, bad = confusion_ref.batch_matrix([d.numpy() for d in b["dets"]], b["targets"].numpy(), b["img_hw"], b["shapes"], nc,
                                                 single_cls=case["single_cls"])
            assert bad == 0
            m += mi
        assert np.array_equal(m.astype(np.float64), want), case["name"]


def test_tie_rule_of_the_restatement():
    # two identical detections of two classes on one label: the lower detection index is the match, the other is left over
    lab = np.array([[1, 10, 10, 50, 50]], np.float32)
    det = np.array([[10, 10, 50, 50, 0.9, 2], [10, 10, 50, 50, 0.8, 0]], np.float32)
    m, _ = confusion_ref.process_image(det, lab, 3)
    assert m[2, 1] == 1 and m[0, 3] == 1 and m.sum() == 2
    # one detection on two identical labels: the lower label index is matched, the other is background
    lab = np.array([[1, 10, 10, 50, 50], [2, 10, 10, 50, 50]], np.float32)
    m, _ = confusion_ref.process_image(det[:1], lab, 3)
    assert m[2, 1] == 1 and m[3, 2] == 1 and m.sum() == 2


def _formatters():
    import msod_amd  # noqa: F401
    from msod_amd.utils import metrics
    return metrics


def _expected(case, batches_dets, save_conf):
    m = _formatters()
    files, jdict = {}, []
    for b, dets in zip(case["batches"], batches_dets):
        for si, d in enumerate(dets):
            if len(d) == 0:
                continue
            stem = Path(b["paths"][si]).stem
            cls, conf, nxywh, tl = confusion_ref.export_values(d.numpy(), b["img_hw"], b["shapes"][si], case["single_cls"])
            for k in range(len(d)):
                line = m.txt_line(float(cls[k]), [float(v) for v in nxywh[k]], float(conf[k]) if save_conf else None)
                files[stem] = files.get(stem, "") + line
                jdict.append(m.json_entry(stem, float(cls[k]), [float(v) for v in tl[k]], float(conf[k])))
    return files, jdict


def test_formatters_reproduce_reference_files(cases):
    for case in cases:
        dets = [b["dets"] for b in case["batches"]]
        files, jdict = _expected(case, dets, True)
        assert files == case["txt_conf"], case["name"]
        assert _expected(case, dets, False)[0] == case["txt"], case["name"]
        assert jdict == case["jdict"], case["name"]
        assert _expected(case, case["hybrid_dets"], True)[0] == case["hybrid"], case["name"]
    ids = [e["image_id"] for e in cases[1]["jdict"]]
    assert ids and all(isinstance(i, int) for i in ids)                     # numeric stems become ints
    assert all(isinstance(e["image_id"], str) for e in cases[0]["jdict"])


def test_header_declares_new_exports_returning_int():
    import ctypes
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    for name in ("cft_eval_confusion", "cft_eval_confusion_workspace_bytes", "cft_eval_export"):
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name
    assert _lib.ABI_VERSION >= 15
    assert len(_lib.SIGNATURES["cft_eval_confusion"][1]) == 19


def test_confusion_kernels_use_no_scratch():
    notes = helpers.kernel_notes(os.path.join(ROOT, "multispectral-object-detection_amd", "csrc", "confusion.hip"))
    names = sorted(notes)
    assert len(notes) == 2 and any("eval_confusion_kernel" in n for n in names) and any("eval_export_kernel" in n for n in names), names
    for name, m in notes.items():
        assert m["private_segment_fixed_size"] == 0, name
        assert m["vgpr_spill_count"] == 0, name
        assert m["sgpr_spill_count"] == 0, name
