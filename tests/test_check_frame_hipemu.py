"""tests/test_check_frame_gpu.py (what the frames the device checkers share must keep: csrc/check_run.h — the host route, the explaining
entries' refusals, set-full's explanation on an armed context, the edges of the explanation slabs) through the host wavefront emulator:
the sources compiled by tools/hipemu/build_emu.py with the host compiler and loaded through MSIM_LIB in a child process, lanes out of
lockstep (HIPEMU_DIVERGENT).  The frames are host code, so what the module pins is walked here in full, without a device."""
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
def test_the_shared_frames_on_the_emulator(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1")
    env.pop("MSIM_DEV_FLAGS", None)
    env.pop("MSIM_POISON", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_check_frame_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "17 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
