"""tests/test_check_ahead_gpu.py — the set-full / echo check queued behind its simulation at launch time — on the host wavefront
emulator, with divergent lanes and every device slab between pattern-filled red zones (MSIM_GUARD=3, csrc/guard.cpp).  The emulator runs
every launch to its end before it returns, so what this holds is the state machine: armed / queued / taken, what is visible before
check(), the checker's scratch regrown in front of the launch, the developer flag and the poisoned buffers; the batches are a few clusters
(tests/pipeline_cases.py).  That a queued check runs beside other launches, and the case on the caller's own stream, need the device."""
import os
import re
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
def test_check_ahead_on_the_emulator_equals_the_oracle_and_the_host_checker(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    env.pop("MSIM_DEV_FLAGS", None)
    env.pop("MSIM_POISON", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rs", os.path.join(ROOT, "tests", "test_check_ahead_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    failed = re.findall(r"^FAILED \S+::(\S+)", r.stdout, re.M)
    assert "[msim guard] 0 damaged byte(s)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and not failed, f"{failed}\n" + r.stdout[-3000:] + r.stderr[-3000:]
    skipped = re.findall(r"^SKIPPED \[\d+\] (\S+?):", r.stdout, re.M)
    assert len(skipped) == 1 and " 1 skipped" in r.stdout and "11 passed" in r.stdout, r.stdout[-3000:]   # the caller's stream, and nothing else
