"""tests/test_duo_trim_hipemu.py's cases on the device: the trims of the flood instantiation of the two-clusters-per-wavefront broadcast
kernel (csrc/duo.hip, latency 0: servers_recv by conservation, the flood's set word written back once, the half's offsets once per op
wave-round), bit for bit against the oracle (history, payload, meta with n_rounds, the six net-stats counters); one case with every
device buffer poisoned, in a process of its own; and the shapes that a capacity stops, compared by their flags as that module says.
The comparison with the recorded sweeps under round limits (clusters stopped with envelopes in flight) runs on the emulator."""
import os
import subprocess
import sys

import pytest

from test_duo_halves_gpu import _run
from test_duo_trim_hipemu import CASES, FEW_VALUES, POISONED, ROOT, check_stops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_duo_trim_equals_the_oracle(lib, case):
    _run(case, True)


def test_duo_trim_with_poisoned_buffers(lib):
    """MSIM_POISON is read once per process: the cases run in a process of their own"""
    cases = POISONED + [FEW_VALUES]
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + cases, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(cases), r.stdout


def test_duo_trim_stopped_by_a_capacity(lib):
    check_stops()
