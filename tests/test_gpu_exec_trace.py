"""The model executor issues the recorded launch plan: for every case of tests/golden/make_exec_golden.py the sequence of library calls
(entry point, lane, scalar arguments) and stream waits of an eager walk equals tests/golden/exec/traces.json, event for event.  The
file was recorded on the MI355X by the executor it names; a refactor of the host logic must not move a launch, a lane or a wait -
under HIP-graph capture these are the nodes and edges of the graph.  Only the host query cft_conv2d_chain_ok is left out of the
comparison; its count on a warm walk is asserted instead."""
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


QUERY, CHAINED = "cft_conv2d_chain_ok", ("cft_conv2d_chain", "cft_conv2d_chain_res")
# the walks of the size-heuristic test below: cfg3 with ops.CHAIN_RES_MIN_ROWS = 0 and the C3 pair chains on
HEURISTIC = [n for n in recipe.CASES if recipe.CASES[n].get("min_rows") == 0 and "c3_attrs" not in recipe.CASES[n]]
WARM_QUERIES = {"x3-two-lanes": 4, "cfg3-chains-two-lanes": 24, "cfg3-chains-one-lane": 24}      # (the recorded executor asked 10 and 56 times)


def count(events, *names):
    return sum(ev.split(" ", 1)[0] in names for ev in events)


def launches(events):
    """The events without the host query cft_conv2d_chain_ok: it enqueues nothing, and how often a cold walk asks is not part of the plan."""
    return [ev for ev in events if not ev.startswith(QUERY + " ")]


def walk_twice(name, dev):
    """(model, inputs, events of the first walk of case ``name``); a walk that chains is repeated on the same model and shape: the warm walk
    chains as often and asks cft_conv2d_chain_ok once per chained launch (the ops wrapper's own guard) - the C3s' plans are cached."""
    model, x, x2, profile = recipe.build_case(name, dev)
    with recipe.chain_res_min_rows(recipe.CASES[name].get("min_rows")):
        events, _ = recipe.traced_forward(model, x, x2, profile)
        if count(events, *CHAINED):
            warm, _ = recipe.traced_forward(model, x, x2, profile)
            assert count(warm, QUERY) == count(warm, *CHAINED) == count(events, *CHAINED) == WARM_QUERIES.get(name, count(events, *CHAINED))
    return model, (x, x2, profile), events


@pytest.mark.parametrize("name", [n for n in recipe.CASES if n not in HEURISTIC])
def test_walk_issues_the_recorded_launches_and_waits(dev, recorded, name):
    _, _, events = walk_twice(name, dev)
    assert first_difference(launches(events), launches(recorded[name])) is None, first_difference(launches(events), launches(recorded[name]))


@pytest.mark.parametrize("name", HEURISTIC)
def test_chained_walk_issues_the_recorded_launches_and_follows_the_size_heuristic(dev, recorded, name):
    """cfg3 at 2 x 192 x 256 with ``ops.CHAIN_RES_MIN_ROWS = 0``: the only shape that reaches cft_conv2d_chain, cft_conv2d_chain_res and the
    shortcut-free pair chains.  With the heuristic restored the same model's next walk issues no chained 3x3 + shortcut + 1x1 launch:
    the C3s' cached plan is keyed on the value it was made under."""
    model, inputs, events = walk_twice(name, dev)
    assert first_difference(launches(events), launches(recorded[name])) is None, first_difference(launches(events), launches(recorded[name]))
    assert count(events, "cft_conv2d_chain_res") == 16
    again, _ = recipe.traced_forward(model, *inputs)
    assert count(again, "cft_conv2d_chain_res") == 0
    assert count(again, "cft_conv2d_chain") == count(events, "cft_conv2d_chain")
