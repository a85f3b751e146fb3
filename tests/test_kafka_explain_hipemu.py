"""tests/test_kafka_explain_gpu.py (the explanation of unclean kafka histories on the device, csrc/kafka_check_dev.hip
kafka_explain_kernel) through the host wavefront emulator: the kernel sources compiled by tools/hipemu/build_emu.py with the host
compiler and loaded through MSIM_LIB in a child process, lanes out of lockstep (HIPEMU_DIVERGENT: a barrier the kernel lacks between the
stride that keeps the first rows and the scan that reads them, or between the gather and the sort, shows as wrong bytes).  The module's
own child (poisoned allocations, chunked launches) inherits the emulator library, so every route of the device run is walked here first."""
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
def test_kafka_explanation_on_the_emulator_equals_the_host_entry(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1")
    env.pop("MSIM_DEV_FLAGS", None)
    env.pop("MSIM_POISON", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_kafka_explain_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "12 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
