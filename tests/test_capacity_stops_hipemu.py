"""tests/test_capacity_stops_gpu.py — capacity stops in every kernel layout beside clusters that run on, and the device checkers on
truncated and whole histories side by side (the table of tests/capacity_stop_cases.py) — on the host wavefront emulator, with divergent
lanes and every device slab between pattern-filled red zones (MSIM_GUARD=3, csrc/guard.cpp): a stop must not write a byte outside a slab.
About a minute and a half for the whole table."""
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
def test_capacity_stops_on_the_emulator_equal_the_oracle(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    env.pop("MSIM_DEV_FLAGS", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_capacity_stops_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    failed = re.findall(r"^FAILED \S+::(\S+)", r.stdout, re.M)
    assert "[msim guard] 0 damaged byte(s)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and not failed, f"{failed}\n" + r.stdout[-3000:] + r.stderr[-3000:]
