"""The kernels each kind of batch runs are the ones recorded in tests/golden/route_kernels.json (tools/route_kernels.py, run
on the MI355X BEFORE the encoder's dispatch was gathered into plan_route): per case, the set of timing slots with non-zero
time after an analysis and a frame assembly, and whether the candidate kernel's hand-over is enabled.  Every case is 3 frames
and must also decode back to its input on the device."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import route_kernels as rk  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "route_kernels.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(c["name"] for c in rk.CASES)


@pytest.mark.parametrize("case", rk.CASES, ids=[c["name"] for c in rk.CASES])
def test_route_runs_the_recorded_kernels(case):
    got = rk.run_case(case)
    want = GOLDEN[case["name"]]
    print(case["name"], got)
    assert got["verified"]
    assert got["kernels"] == want["kernels"]
    assert got["hand"] == want["hand"]
