"""tests/test_duo_steady_leave_hipemu.py's cases on the device: the steady leave of the two-clusters-per-wavefront broadcast kernel
(csrc/duo.hip, latency 0: a flood stretch that ends because a steady half has run dry parks that half or goes to the op round without a
pass through R0 and the exit test), bit for bit against the oracle (history, payload, meta with n_rounds, the six net-stats counters).
Every case is that module's shape with a handful of clusters at a time limit of at most 1 s of virtual time (GPU_CASES: the oracle flags
none of them, see that module's test_no_case_is_flagged); the poisoned cases run with every device buffer filled with 0xA5, in a process
of their own under a time limit; the shapes that a capacity stops are compared by their flags.  The comparison with the recorded
sweeps under round limits (clusters stopped with envelopes in flight) and the count of steady leaves run on the emulator."""
import os
import subprocess
import sys

import pytest

from test_duo_halves_gpu import _run
from test_duo_steady_leave_hipemu import GPU_CASES, GPU_POISONED, ROOT, check_stops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", GPU_CASES)
def test_duo_steady_leave_equals_the_oracle(lib, case):
    _run(case, True)


def test_duo_steady_leave_with_poisoned_buffers(lib):
    """MSIM_POISON is read once per process: the cases run in a process of their own"""
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + GPU_POISONED, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(GPU_POISONED), r.stdout


def test_duo_steady_leave_stopped_by_a_capacity(lib):
    check_stops()
