"""tests/test_txn_findings_gpu.py (the non-cycle findings on the device: txn_findings_kernel / rw_findings_kernel, csrc/txn_findings.inc)
through the host wavefront emulator: the kernel sources compiled by tools/hipemu/build_emu.py with the host compiler and loaded through
MSIM_LIB in a child process, lanes out of lockstep (HIPEMU_DIVERGENT), device slabs fenced (MSIM_GUARD=3: a record written past the
region or past a history's slab fails the test that wrote it).  The module's own children (at most 7 histories per launch, poisoned
allocations) inherit the emulator library.

Seen to protect, by taking one out at a time (the child then fails at the test named; with it, it passes):
  * f_slot's shuffle of the leader's base to the lanes that emit with it (without it every other lane of the group takes slot 0 + its
    rank, records overwrite one another: test_every_case_as_a_batch[list-append]);
  * `pass == 0` at the emission points of pass E and of rw_body's two passes (without it every such finding is there twice:
    test_every_case_as_a_batch[list-append]);
  * the completion row as the last word of the order in f_finish's ranking (without it two rows outside the payload area take the same
    rank, one record is lost and a slot stays zero: test_every_case_as_a_batch[rw-register]).
The barrier behind the counter's reset cannot be seen here: the emulator runs lane 0 up to its first cross-lane operation before any
other lane starts.  Only the device run protects that and: that the lanes of a divergent branch which reach f_slot together are what
__ballot(1) names (the emulator groups the lanes parked at the same call site, whatever branch took them there), that the leader's
atomic is ordered before the group's stores as the hardware issues them, and that the region's plain stores are visible to the other
lanes behind the workgroup barrier."""
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
def test_findings_on_the_emulator_equal_the_host_entry(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    env.pop("MSIM_DEV_FLAGS", None)
    env.pop("MSIM_POISON", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_txn_findings_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "13 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
