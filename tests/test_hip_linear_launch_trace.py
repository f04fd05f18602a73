"""The Linear launchers start the kernels, and write the bits, recorded in tests/golden/linear_launch_trace.json.

The fixture was recorded by tests/golden/make_linear_launch_trace.py before the launchers' kernel choice moved into
csrc/vs_linear_pick.h: per case the ordered device kernel names (template arguments included, so a 128x128-tile
gemm_nt_128 and a 256x256-tile one differ) and the SHA-256 of the outputs.  The cases - the per-op C entries at the
shapes the pick decides on, scoring forwards in every arithmetic, training steps in fp32 / bf16 / fp16 - are in
tests/linear_launch_cases.py.  Equality, no tolerance: the same kernels on the same grids give the same bits.
"""
import json
import os

import pytest

import linear_launch_cases as llc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_launch_trace.json")) as _f:
    FIXTURE = json.load(_f)
CASES = llc.cases()


def test_fixture_and_case_list_agree():
    assert sorted(FIXTURE["cases"]) == sorted(name for name, _, _ in CASES)


@pytest.mark.parametrize("name,rows,fn", CASES, ids=[c[0] for c in CASES])
def test_launches_and_bits_match_the_recorded_trace(vsa, name, rows, fn):
    want = FIXTURE["cases"][name]
    names, digest = llc.trace(vsa, rows, fn)
    assert names == [FIXTURE["names"][i] for i in want["kernels"]]
    assert digest == want["sha256"]
