"""tests/test_pipeline_gpu.py — the asynchronous, pipelined launch path against the oracle and the reference checkers — on the host
wavefront emulator, with divergent lanes and every device slab between pattern-filled red zones (MSIM_GUARD=3, csrc/guard.cpp).  The
emulator runs every launch to its end before it returns, so what this holds is the state machine of the path (fetched / fetch_pending /
checked), the pinned mirrors and device slabs regrown while a context's batch grows and shrinks, and the compaction kernels; the batches
are 4 / 6 / 3 clusters (tests/pipeline_cases.py).  The test on the caller's own stream needs the device and is skipped here."""
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
def test_pipelined_launch_path_on_the_emulator_equals_the_oracle(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    env.pop("MSIM_DEV_FLAGS", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rs", os.path.join(ROOT, "tests", "test_pipeline_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    failed = re.findall(r"^FAILED \S+::(\S+)", r.stdout, re.M)
    assert "[msim guard] 0 damaged byte(s)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and not failed, f"{failed}\n" + r.stdout[-3000:] + r.stderr[-3000:]
    skipped = re.findall(r"^SKIPPED \[\d+\] (\S+?):", r.stdout, re.M)
    assert len(skipped) == 1 and " 1 skipped" in r.stdout, r.stdout[-3000:]   # the caller's stream, and nothing else
