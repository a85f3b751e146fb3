"""tests/test_journal_messages_gpu.py (the net journal's messages on the device: journal_messages_kernel) through the host wavefront
emulator: the kernel sources compiled by tools/hipemu/build_emu.py with the host compiler and loaded through MSIM_LIB in a child
process, lanes out of lockstep (HIPEMU_DIVERGENT: a lane runs on its own up to the next barrier or wavefront operation) and every
device slab fenced (MSIM_GUARD=3: a record or table word written past a journal's slab fails the test that wrote it).  The module's
own children (poisoned allocations, the chunked launches) inherit the emulator library.

What this run protects, found by taking one barrier or atomic out at a time: the barrier behind the clearing of the table (3 tests fail
without it: a lane's send is entered, a later lane clears the word), the barrier of a block of sweep 1 that publishes the wavefronts'
send counts (5: the record indices), the barrier behind sweep 2 in front of the quantiles and the summary (6), the barrier inside
wg_sum (6: the bisection counts).  What it does NOT protect: the emulator runs the lanes between two such points one after the other, in
ascending order, so an order that holds by ascending lanes holds without its barrier — the barrier BETWEEN THE TWO SWEEPS, which puts
every wavefront's table words and records in front of the recvs that read them (a recv's send lies at a lower position, so at a lower
lane of its block or in an earlier block) — and a read-modify-write that is not atomic still counts right: the compare-and-swap that
enters a send in the table and the one by which a recv claims its send, the additions of the counters in LDS, the bits of the endpoint
bitmap.  Nor does it miss the second slot of the two alternating LDS arrays (the wavefronts' totals of a block, wg_sum's partial sums),
which spare a barrier a block: a fast wavefront overwrites what a slow one still reads only where wavefronts run side by side.  Those
are held only by tests/test_journal_messages_gpu.py on the device, where wavefronts do race."""
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
def test_journal_messages_on_the_emulator_equal_the_host_entry(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    env.pop("MSIM_DEV_FLAGS", None)
    env.pop("MSIM_POISON", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_journal_messages_gpu.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "10 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
