"""What csrc/launch_plan.h plans — scratch words, LDS offsets, the capacities and periods in KParams, the one-cluster kernel, and per
packed layout its eligibility and launch-size floor — over the grid of tools/launch_plan_dump.cpp (every node program x workers per
node x cluster size x nemesis x journal x latency x loss x inbox capacity x developer flags: 59008 accepted configurations), line by
line against tests/golden/launch_plan.txt.xz.  The recorded lines are those of the code before the two tables existed (its if-chains
and nested ternaries, printed by a patch of that code), so equality here is the proof that the tables plan what they planned.  The
tool runs under AddressSanitizer and UBSan as a stand-alone program and itself checks that the grid reaches every row of both tables
and that no two packed layouts other than duo / bcast8 are eligible together.

A deliberate change of a layout changes these lines: re-record the fixture in the same commit (python tools/launch_plan_dump.py
--record) and say in its message which lines moved and why."""
import lzma
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.timeout(1800)
def test_launch_plans_equal_the_recorded_ones():
    if shutil.which(os.environ.get("HIPEMU_CXX", "g++")) is None:
        pytest.skip("no host C++ compiler for the emulator build")
    import launch_plan_dump as D
    rc, out = D.run(D.build())
    assert rc == 0, "the tool's own checks (coverage of both tables, exclusive packed rows, sanitizers) failed"
    with lzma.open(D.GOLDEN, "rb") as f:
        want = f.read().split(b"\n")
    got = out.split(b"\n")
    assert len(got) == len(want) and len(got) > 50000
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n got {g.decode()}\nwant {w.decode()}"
