"""tests/test_rw_large_components_gpu.py (strongly connected components beyond the LDS matrix of the rw-register classification:
csrc/rw_check_dev.hip, single_by_search) through the host wavefront emulator, as tests/test_rw_classify_hipemu.py runs its file: the
kernel sources compiled by tools/hipemu/build_emu.py with the host compiler and loaded through MSIM_LIB in a child process, lanes out
of lockstep (HIPEMU_DIVERGENT: a barrier the search lacks between taking transactions off the worklist and pushing to it shows as a
wrong record).  Every case runs, the 1500-transaction ones and the engine's histories included (about two minutes)."""
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
def test_large_components_on_the_emulator_equal_the_host_analysis(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1")
    env.pop("MSIM_DEV_FLAGS", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_rw_large_components_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and " passed" in last and "skipped" not in last and "failed" not in last and "error" not in last, r.stdout[-3000:] + r.stderr[-3000:]
