"""The guarded-buffer harness (tests/guarded.py) on CPU tensors with fake "kernels" written in torch: each planted defect is reported,
a correct kernel passes - and the coverage lock: every entry point of include/cft_hip.h that can write memory is in the sweep table of
tests/test_gpu_memory_hygiene.py or exempt with a reason.  No GPU needed."""
import re

import pytest
import torch

import guarded as G

CPU = torch.device("cpu")


def _x(n=37, seed=0, lo=0.5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) + lo           # strictly positive: a zero slack element never wins a maximum


def _past(t, n):
    """The first n elements starting at ``t``'s first, whatever the view's own length: what a kernel indexing past its tensor sees."""
    return torch.as_strided(t, (n,), (1,))


def _scale_case(defect=None):
    """y = 2 x on an NHWC channel slice [B, 8, 3, 5] at channels [8, 16) of 24, plus a dense copy."""
    x = torch.arange(2 * 8 * 3 * 5, dtype=torch.float32).reshape(2, 8, 3, 5) + 1

    def case(run):
        xd = run.inp("x", x, layout="nhwc", ld=16, off=8)
        y = run.out("y", x.shape, torch.float32, layout="nhwc", ld=24, off=8)
        flat = run.out("flat", (x.numel(),), torch.float32)
        y.copy_(2 * xd)
        flat.copy_(xd.reshape(-1))
        if defect == "past_payload":
            _past(flat, flat.numel() + 1)[-1] = 5.0
        if defect == "neighbour_channel":
            _past(y, 9)[8] = 5.0                   # pixel (0, 0, 0): channel 16 of the buffer, one past the slice
        if defect == "input_written":
            xd[0, 0, 0, 0] = -1.0
        run.status(0, "fake")
    return case


def test_correct_fake_kernel_passes():
    out = G.check_case(_scale_case(), CPU)
    assert torch.equal(out["y"], 2 * (torch.arange(240, dtype=torch.float32).reshape(2, 8, 3, 5) + 1))


def test_store_past_the_payload_is_reported():
    problems, _ = G.run_case(_scale_case("past_payload"), CPU)
    assert any("band of out 'flat' overwritten" in p and "0 bytes past the payload" in p for p in problems), problems


def test_store_into_a_neighbouring_channel_is_reported():
    problems, _ = G.run_case(_scale_case("neighbour_channel"), CPU)
    assert any("band of out 'y' overwritten" in p and "slack of the channel slice" in p for p in problems), problems
    assert not any("'flat'" in p for p in problems)


def test_written_input_and_bad_status_are_reported():
    problems, _ = G.run_case(_scale_case("input_written"), CPU)
    assert any("input 'x' changed" in p for p in problems), problems

    def bad(run):
        run.out("y", (4,), torch.float32).zero_()
        run.status(-1, "fake")
    problems, _ = G.run_case(bad, CPU)
    assert any("status -1" in p for p in problems)

    def silent(run):
        run.out("y", (4,), torch.float32).zero_()
    problems, _ = G.run_case(silent, CPU)
    assert any("recorded no status" in p for p in problems)


def test_workspace_accumulated_without_clearing_is_reported():
    x = _x()

    def case(run, clear):
        xd = run.inp("x", x)
        ws = run.work("ws", (1,), torch.float32)
        y = run.out("y", (1,), torch.float32)
        if clear:
            ws.zero_()
        ws += xd.sum()
        y.copy_(ws)
        run.status(0)
    problems, _ = G.run_case(lambda r: case(r, False), CPU)
    assert any("output 'y' differs" in p for p in problems), problems
    assert G.run_case(lambda r: case(r, True), CPU)[0] == []


def _reduce_case(op, slack):
    x = _x()

    def case(run):
        xd = run.inp("x", x)
        y = run.out("y", (1,), torch.float32)
        v = _past(xd, x.numel() + slack)
        if op == "max":                      # fmaxf semantics: a NaN operand is dropped
            acc = v[0]
            for e in v[1:]:
                acc = torch.fmax(acc, e)
            y[0] = acc
        else:
            y[0] = v.sum()
        run.status(0)
    return case


def test_max_over_one_slack_element_needs_the_large_finite_fill():
    """0x00 gives 0, which never wins over positive data; 0xFF gives a NaN, which fmax drops: only 0x7B shows it."""
    assert G.run_case(_reduce_case("max", 1), CPU, fills=(0x00, 0xFF))[0] == []
    problems, _ = G.run_case(_reduce_case("max", 1), CPU)
    assert len(problems) == 1 and "fill 0x7B: output 'y' differs" in problems[0], problems
    assert G.run_case(_reduce_case("max", 0), CPU)[0] == []


def test_sum_over_one_slack_element_is_reported():
    problems, _ = G.run_case(_reduce_case("sum", 1), CPU)
    assert any("fill 0xFF: output 'y' differs" in p for p in problems), problems
    assert G.run_case(_reduce_case("sum", 0), CPU)[0] == []


def test_defined_mask_limits_the_comparison_and_nothing_else():
    """Slots past ``count`` are unspecified: garbage there passes under the mask, garbage in a valid slot does not, and a store
    outside the tensor is reported whatever the mask says."""
    def case(run, spoil_valid=False, overrun=False):
        dets = run.out("dets", (6, 4), torch.float32, defined=lambda o: (torch.arange(6) < int(o["count"][0])).view(6, 1))
        count = run.out("count", (1,), torch.int32)
        count[0] = 3
        dets[:3] = 1.0                         # rows 3.. keep the fill byte
        if spoil_valid:
            dets[2, 1] = float(run.fill)
        if overrun:
            _past(dets, 25)[24] = 9.0
        run.status(0)
    assert G.run_case(case, CPU)[0] == []
    assert any("output 'dets' differs" in p for p in G.run_case(lambda r: case(r, spoil_valid=True), CPU)[0])
    assert any("band of out 'dets'" in p for p in G.run_case(lambda r: case(r, overrun=True), CPU)[0])


def test_launched_names_are_collected_and_held_objects_kept():
    launched = set()

    def case(run):
        run.out("y", (4,), torch.float32).zero_()
        run.hold(bytearray(8))
        run.status(0, "cft_a")
        run.status(0, "cft_b")
        assert len(run.held) == 1
    G.check_case(case, CPU, launched=launched)
    assert launched == {"cft_a", "cft_b"}


def test_band_geometry():
    for shape, dtype in (((3,), torch.uint8), ((300, 1280), torch.float32), ((0,), torch.float32)):
        g = G.guarded(shape, dtype, CPU, 0x7B)
        assert g.band % 512 == 0 and g.band >= max(64 * 1024, g.payload_bytes)
        assert g.raw.numel() == 2 * g.band + g.payload_bytes
        assert g.bands_intact() == (True, None)
    g = G.guarded((2, 8, 3, 5), torch.float16, CPU, 0xFF, layout="nhwc", ld=24, off=16)
    assert g.t.shape == (2, 8, 3, 5) and g.t.stride() == (3 * 5 * 24, 1, 5 * 24, 24) and g.t.storage_offset() * 2 == g.band + 32
    assert bool(torch.isnan(G.guarded((4,), torch.bfloat16, CPU, 0xFF).t.float()).all())
    assert float(G.guarded((4,), torch.float16, CPU, 0x7B).t[0]) == 61280.0
    assert float(G.guarded((4,), torch.float32, CPU, 0x7B).t[0]) > 1e36 and int(G.guarded((4,), torch.int32, CPU, 0x7B).t[0]) == 0x7B7B7B7B


# ------------------------------------------------------------------------------ coverage lock
# Entry points with a non-const pointer parameter that the sweep does not run, each with its reason.  Only functions that touch no
# device memory (host halves, sizers) and the clock probe belong here.
_HOST = "host only, no device memory"
EXEMPT = {
    "cft_jpeg_info": _HOST, "cft_jpeg_entropy": _HOST, "cft_jpeg_layout": _HOST, "cft_jpeg_quality_tables": _HOST,
    "cft_jpeg_write_bound": _HOST, "cft_jpeg_write": _HOST, "cft_last_error": _HOST,
    "cft_batchnorm_train_workspace": _HOST, "cft_eval_match_workspace_bytes": _HOST, "cft_eval_ap_workspace_bytes": _HOST,
    "cft_loss_workspace_bytes": _HOST, "cft_eval_curves_workspace_bytes": _HOST, "cft_eval_confusion_workspace_bytes": _HOST, "cft_loss_workspace_offsets": _HOST,
    "cft_anchor_kmeans_workspace_bytes": _HOST, "cft_anchor_evolve_workspace_bytes": _HOST,
    "cft_clock_probe": "measures (spins on the clocks), does not compute",
}


def writers(text):
    """Names of the prototypes with at least one pointer parameter that is not ``const``, among the functions _lib.parse_header finds."""
    from msod_amd import _lib
    sigs, _ = _lib.parse_header(text)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    found = set()
    for name, args in re.findall(r"\b(cft_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name in sigs
        if any("*" in a and not re.match(r"\s*const\b", a) for a in args.split(",")):
            found.add(name)
    return found


def test_writers_parser():
    text = ("int cft_a(const float* x, float* y, int n);\n/* int cft_c(float* y); */\nlong cft_b(const void* x, int n);\n"
            "int cft_d(const float* const* p, void* stream);\nint cft_e(float* const* grad);\nconst char* cft_f(void);")
    assert writers(text) == {"cft_a", "cft_d", "cft_e"}          # (a stream is a non-const pointer too: nearly every launcher counts)


def test_every_writing_entry_point_is_swept_or_exempt():
    from msod_amd import _lib
    import test_gpu_memory_hygiene as sweep
    with open(_lib.HEADER) as fh:
        need = writers(fh.read())
    swept = set(sweep.swept_entry_points())
    assert not (swept - set(_lib.SIGNATURES)), f"sweep table names unknown entry points: {sorted(swept - set(_lib.SIGNATURES))}"
    assert not (set(EXEMPT) & swept), f"both swept and exempt: {sorted(set(EXEMPT) & swept)}"
    assert not (set(EXEMPT) - set(_lib.SIGNATURES)), f"exempt but not in the header: {sorted(set(EXEMPT) - set(_lib.SIGNATURES))}"
    missing = sorted(need - swept - set(EXEMPT))
    assert not missing, f"entry points that write memory and are neither swept nor exempt: {missing}"
    for name, reason in EXEMPT.items():
        assert reason == _HOST or name == "cft_clock_probe", f"{name}: only host-only functions, sizers and the clock probe are exempt"
