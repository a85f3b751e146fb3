"""tests/test_duo_block_plan_hipemu.py's cases on the device: the block plan of the two-clusters-per-wavefront broadcast kernel
(csrc/duo.hip, latency 0: in front of the steady run's loop lane k of a half plans draw k of the block of generator draws, and the
longest prefix of ops that pass the loop's own tests is committed at once, a planned read writing what its node's set must hold), bit
for bit against the oracle (history, payload, meta with n_rounds, the six net-stats counters).  Every case is a handful of clusters at a
time limit of at most 1 s of virtual time (CASES of tests/test_duo_flood_memo_hipemu.py: the oracle flags none of them); the poisoned
cases run with every device buffer filled with 0xA5, in a process of their own under a time limit; the capacities moved over every op of
one block are compared by their flags, and every unflagged instance in full.  The comparison with a -DDUO_NO_BLOCK_PLAN build under
round limits, the build without the plan's facts and the count of ops taken by plans run on the emulator."""
import os
import subprocess
import sys

import pytest

from test_duo_halves_gpu import _run
from test_duo_block_plan_hipemu import CASES, POISONED, ROOT, plan_capacity_sweeps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_duo_block_plan_equals_the_oracle(lib, case):
    _run(case, True)


def test_duo_block_plan_with_poisoned_buffers(lib):
    """MSIM_POISON is read once per process: the cases run in a process of their own"""
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + POISONED, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(POISONED), r.stdout


def test_duo_block_plan_stopped_by_a_capacity_inside_a_plan(lib):
    plan_capacity_sweeps()
