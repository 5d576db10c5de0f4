"""The op layer's launch sequence, call for call: every C-ABI call dn-splatter_amd/_ops.py issues in the scenarios of
tests/_launch_trace.py — entry point, stream, order, every scalar argument and the null-ness of every pointer — against the
sequence recorded from the op layer before its argument builders were factored out (tests/golden/op_layer_trace.json).  A launch
that moved, a second dnsplat_bin_prepare or a pointer field that turned null fails here, at its cause, not in a parity test."""
import json

import pytest

import _launch_trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(_launch_trace.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_exactly_the_scenarios(golden):
    assert sorted(golden) == sorted(_launch_trace.SCENARIOS)
    assert len(_launch_trace.EXCLUDED) <= 4, "more than a handful of excluded fields: fix the scenario instead"


@pytest.mark.parametrize("name", sorted(_launch_trace.SCENARIOS))
def test_launch_sequence_equals_the_recorded_one(dns, golden, name):
    got = json.loads(json.dumps(_launch_trace.record(_launch_trace.SCENARIOS[name])))
    want = golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: entry {i} differs\n got  {json.dumps(g, sort_keys=True)}\n want {json.dumps(w, sort_keys=True)}"
    assert len(got) == len(want), f"{name}: {len(got)} entries, recorded {len(want)}"
