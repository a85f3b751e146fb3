"""tests/test_small_explain_gpu.py (the explanation of pn-counter, unique-ids and echo verdicts on the device: pn_explain_kernel,
unique_explain_kernel / unique_explain_lds_kernel, echo_explain_kernel) through the host wavefront emulator: the kernel sources compiled
by tools/hipemu/build_emu.py with the host compiler and loaded through MSIM_LIB in a child process, lanes out of lockstep
(HIPEMU_DIVERGENT: a lane runs on its own up to the next barrier or wavefront operation) and every device slab fenced (MSIM_GUARD=3: a
record written past a history's slab fails the test that wrote it).  The module's own children (poisoned allocations, the HBM tables in
chunks) inherit the emulator library.

What this run protects, found by taking one barrier or atomic out at a time: the workgroup barrier between unique_explain_body's two
row sweeps (2 tests fail without it), the atomicMin that keeps the second row (1: a plain store keeps the LAST row), the barrier in
front of echo_explain_kernel's writing sweep (1).  What it does NOT protect: the emulator runs the lanes between two such points one
after the other, in ascending order, so a read-modify-write that is not atomic still counts right — the atomicAdd that hands out the
list slots and the one that counts the acknowledgements in unique_explain_body — and an order that holds by ascending lanes holds
without its fence (wv_fence behind echo_explain_kernel's atomicMin; pn_body.inc's barrier behind the bitmap's store, which a
wavefront operation follows at once).  Those are held only by tests/test_small_explain_gpu.py on the device, where lanes do race."""
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
def test_small_explanations_on_the_emulator_equal_the_host_entries(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    env.pop("MSIM_DEV_FLAGS", None)
    env.pop("MSIM_POISON", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_small_explain_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "13 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
