"""tests/test_set_explain_gpu.py (the explained set-full verdicts on the device, csrc/set_full_body.inc behind set_explain_kernel)
through the host wavefront emulator: the kernel sources compiled by tools/hipemu/build_emu.py with the host compiler and loaded
through MSIM_LIB in a child process, lanes out of lockstep (HIPEMU_DIVERGENT: a barrier missing between the per-element outcomes and
the compaction, or between the latencies and the eight maxima, shows as a wrong record).  The module's own child (poisoned
allocations) inherits the emulator library."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which(os.environ.get("HIPEMU_CXX", "g++")) is None:
        pytest.skip("no host C++ compiler for the emulator build")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hipemu", "build_emu.py")], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(EMU)
    return EMU


@pytest.mark.timeout(1800)
def test_explained_set_full_on_the_emulator_equals_the_host_entry(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1")
    env.pop("MSIM_DEV_FLAGS", None)
    env.pop("MSIM_POISON", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_set_explain_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "8 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
