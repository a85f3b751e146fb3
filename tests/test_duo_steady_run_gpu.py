"""tests/test_duo_steady_run_hipemu.py's cases on the device: the steady run of the two-clusters-per-wavefront broadcast kernel
(csrc/duo.hip, latency 0: the loop of the read runs also takes a broadcast whose flood the wavefront remembers, so that a half goes
through a block of generator draws inside the loop), bit for bit against the oracle (history, payload, meta with n_rounds, the six
net-stats counters).  Every case is a handful of clusters at a time limit of at most 1 s of virtual time (CASES of
tests/test_duo_flood_memo_hipemu.py: the oracle flags none of them); the poisoned cases run with every device buffer filled with 0xA5, in
a process of their own under a time limit; the capacities that stop a cluster inside a run are compared by their flags, and every
unflagged instance in full.  The comparison with a -DDUO_NO_STEADY_RUN build under round limits, the -DDUO_MEMO_VERIFY build and the
count of op wave-rounds run on the emulator."""
import os
import subprocess
import sys

import pytest

from test_duo_halves_gpu import _run
from test_duo_steady_run_hipemu import CASES, POISONED, ROOT, capacity_sweeps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_duo_steady_run_equals_the_oracle(lib, case):
    _run(case, True)


def test_duo_steady_run_with_poisoned_buffers(lib):
    """MSIM_POISON is read once per process: the cases run in a process of their own"""
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + POISONED, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(POISONED), r.stdout


def test_duo_steady_run_stopped_by_a_capacity_inside_a_run(lib):
    capacity_sweeps()
