"""tests/test_duo_flood_memo_hipemu.py's cases on the device: the flood memo of the two-clusters-per-wavefront broadcast kernel
(csrc/duo.hip, latency 0: a wavefront simulates the flood of a broadcast once per origin and applies the record of that simulation to
later broadcasts from the same origin; two halves with nothing in flight go from one op round straight to the next), bit for bit against
the oracle (history, payload, meta with n_rounds, the six net-stats counters).  Every case is a handful of clusters at a time limit of at
most 1 s of virtual time (CASES: the oracle flags none of them, see that module's test_no_case_is_flagged); the poisoned cases run with
every device buffer filled with 0xA5, in a process of their own under a time limit; the shapes that a capacity stops are compared by
their flags.  The comparison with a -DDUO_NO_MEMO build under round limits, the -DDUO_MEMO_VERIFY build and the count of recorded and
replayed floods run on the emulator."""
import os
import subprocess
import sys

import pytest

from test_duo_halves_gpu import _run
from test_duo_flood_memo_hipemu import CASES, POISONED, ROOT, check_stops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_duo_flood_memo_equals_the_oracle(lib, case):
    _run(case, True)


def test_duo_flood_memo_with_poisoned_buffers(lib):
    """MSIM_POISON is read once per process: the cases run in a process of their own"""
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + POISONED, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(POISONED), r.stdout


def test_duo_flood_memo_stopped_by_a_capacity(lib):
    check_stops()
