"""tests/test_duo_stretch_hipemu.py's cases on the device: the flood stretch and the fan-out masks of the two-clusters-per-wavefront
broadcast kernel (csrc/duo.hip, latency 0), bit for bit against the oracle (history, payload, meta with n_rounds, net stats); the shapes
that a capacity stops, compared by their flags as that module says; and two clusters under a sweep of round limits
(MSIM_FLAG_ROUND_LIMIT alone, at least L + 1 rounds, rows and payload a prefix of the oracle's).  Whether flood rounds are taken in
stretches at all is checked on the emulator, by the counters of a -DDUO_PROF -DDUO_PROF_STRETCH build."""
import os
import subprocess
import sys

import pytest

from test_duo_halves_gpu import _run
from test_duo_stretch_hipemu import CASES, POISONED, ROOT, check_pair_limits, check_stops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_duo_stretch_equals_the_oracle(lib, case):
    _run(case, True)


def test_duo_stretch_with_poisoned_buffers(lib):
    """MSIM_POISON is read once per process: the case runs in a process of its own"""
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + POISONED, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(POISONED), r.stdout


def test_duo_stretch_stopped_by_a_capacity(lib):
    check_stops()


def test_duo_stretch_with_a_round_limit(lib):
    check_pair_limits()
