"""The outer loop of the four manifold-only entry points (ManiSDP_onlyunitdiag with a real and with a complex Hermitian C,
ManiSDP_onlyunitblockdiag, ManiSDP_posegraph) against a scripted handle, no library loaded: for every scenario of
unitdiag_loop_fake.py the sequence of handle calls with their arguments, the printed lines, obj, data and the returned factor --
or the exception and whether the handle was closed -- equal the recorded ones of tests/golden/unitdiag_loop_traces.json exactly.
The same NumPy operations in the same order on the same scripted answers give the same bytes; an entry that differs means the
loop called, computed or printed something else than it did when the fixture was recorded (see the helper's docstring)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unitdiag_loop_fake as F  # noqa: E402

with open(F.FIXTURE) as _fh:
    TRACES = json.load(_fh)


def test_the_fixture_holds_every_scenario_and_no_other():
    assert sorted(TRACES) == sorted(F.SCENARIOS)
    assert set(F.INTENDED_CHANGES) <= set(F.SCENARIOS)


@pytest.mark.parametrize("name", sorted(F.SCENARIOS))
def test_scenario_takes_the_recorded_course(name):
    got, want = F.record(F.SCENARIOS[name]), TRACES[name]
    for key in sorted(set(got) | set(want)):
        assert got.get(key) == want.get(key), (name, key)


def test_a_handle_whose_set_up_raises_is_closed():
    """Every scenario that raises after its handle exists leaves it closed."""
    for name, trace in TRACES.items():
        if "raised" in trace:
            assert all(trace["closed"]), name
