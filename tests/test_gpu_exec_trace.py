"""The model executor issues the recorded launch plan: for every case of tests/golden/make_exec_golden.py the sequence of library calls
(entry point, lane, scalar arguments) and stream waits of an eager walk equals tests/golden/exec/traces.json, event for event.  The
file was recorded on the MI355X by the executor it names; a refactor of the host logic must not move a launch, a lane or a wait -
under HIP-graph capture these are the nodes and edges of the graph."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_exec_golden as recipe  # noqa: E402
from launch_trace import first_difference  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "exec", "traces.json")) as fh:
        doc = json.load(fh)
    assert "MI355X" in doc["recorded"] and "commit" in doc["recorded"]
    assert sorted(doc["cases"]) == sorted(recipe.CASES)
    return doc["cases"]


@pytest.mark.parametrize("name", [n for n in recipe.CASES if "min_rows" not in recipe.CASES[n]])
def test_walk_issues_the_recorded_launches_and_waits(dev, recorded, name):
    events, _ = recipe.run_case(name, dev)
    assert first_difference(events, recorded[name]) is None, first_difference(events, recorded[name])


@pytest.mark.parametrize("name", [n for n in recipe.CASES if "min_rows" in recipe.CASES[n]])
def test_chained_walk_issues_the_recorded_launches_and_follows_the_size_heuristic(dev, recorded, name):
    """cfg3 at 2 x 192 x 256 with ``ops.CHAIN_RES_MIN_ROWS = 0``: the only shape that reaches cft_conv2d_chain, cft_conv2d_chain_res and the
    shortcut-free pair chains.  With the heuristic restored the same model's next walk issues no chained 3x3 + shortcut + 1x1 launch:
    the C3s' cached decision is keyed on the value it was taken under."""
    model, x, x2, profile = recipe.build_case(name, dev)
    with recipe.chain_res_min_rows(recipe.CASES[name]["min_rows"]):
        events, _ = recipe.traced_forward(model, x, x2, profile)
    assert first_difference(events, recorded[name]) is None, first_difference(events, recorded[name])
    assert sum(ev.startswith("cft_conv2d_chain_res ") for ev in events) == 16
    again, _ = recipe.traced_forward(model, x, x2, profile)
    assert not [ev for ev in again if ev.startswith("cft_conv2d_chain_res ")]
    assert sum(ev.startswith("cft_conv2d_chain ") for ev in again) == sum(ev.startswith("cft_conv2d_chain ") for ev in events)
