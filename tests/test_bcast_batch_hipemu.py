"""The batched-gossip arm of the general kernel (csrc/sim_kernel_general.inc, MSIM_NODE_BCAST_BATCH) on the host wavefront emulator
(tools/hipemu, built from the kernel sources as tests/test_hipemu_parity.py builds it) against the model on the bridge's scheduler
(tests/bcast_batch_ref.py): decoded history, net stats, round count and flags, and with the journal on every event — on a machine
without a GPU."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")

CASES = [
    dict(node_count=5, rate=20, time_limit=5, seed=41, n=3),                                                       # fault-free
    dict(node_count=9, rate=30, time_limit=8, latency=20, nemesis=["partition"], nemesis_interval=2, seed=42, n=2),  # partitions: timeouts, re-sent batches
    dict(node_count=6, rate=30, time_limit=6, latency=30, latency_dist="exponential", p_loss=0.15, topology="total", seed=43, n=2),   # loss
    dict(node_count=7, concurrency=3, rate=30, time_limit=6, latency=50, topology="line", p_loss=0.05, nemesis=["partition"], nemesis_interval=2,
         seed=44, n=2, journal_capacity=100000),                                                                   # journal on
    # the partition run that real demo/python/broadcast.py processes reproduced (tests/golden/bcast_batch_digests.json "pinned")
    dict(node_count=9, rate=20, time_limit=8, latency=20, nemesis=["partition"], nemesis_interval=2, seed=32, n=2, journal_capacity=200000),
]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which(os.environ.get("HIPEMU_CXX", "g++")) is None:
        pytest.skip("no host C++ compiler for the emulator build")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hipemu", "build_emu.py")], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(EMU)
    return EMU


@pytest.mark.timeout(1800)
def test_kernel_on_the_emulator_equals_the_model(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    args = [json.dumps(c) for c in CASES]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bcast_batch_ref.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(CASES), r.stdout[-3000:]
