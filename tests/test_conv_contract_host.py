"""CPU: the shape contracts of the conv entry points answer what tests/golden/conv_contract.json recorded.

The ``*_supported`` predicates look at the descriptor alone, and a refused call returns in front of any launch, so none of this needs
a GPU.  The cases (an explicit grid, single-field departures from an accepted descriptor, the upsample source's own terms) and the
refused calls are built by tools/make_conv_contract_golden.py, which also wrote the recorded answers.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location("make_conv_contract_golden", os.path.join(ROOT, "tools", "make_conv_contract_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_tool()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_contract.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("pred", G.PREDICATES)
def test_supported_answers_match_recorded(golden, pred):
    lib = G.L.load()
    cases = G.cases(pred)
    assert len(cases) == golden["cases"][pred]
    got, want = G.to_hex(G.answers(lib, pred)), golden["answers"][pred]
    if got != want:
        a, b = (bin(int(h, 16))[2:].zfill(4 * len(h)) for h in (got, want))
        diff = [f"{cases[i][0]}: {a[i]} (recorded {b[i]})" for i in range(len(cases)) if a[i] != b[i]]
        pytest.fail(f"{pred}: {len(diff)} answers changed: " + "; ".join(diff[:12]))
    assert sum(G.answers(lib, pred)) >= 20  # (the table is not vacuous)


@pytest.mark.parametrize("name", sorted(G.REFUSALS))
def test_refused_call_reports_recorded_message(golden, name):
    yes, rc, msg = G.refuse(G.L.load(), name)
    assert yes == 0, f"{name}: the predicate accepts the layer, the call is not made"
    assert rc != 0
    assert msg == golden["refusals"][name]
