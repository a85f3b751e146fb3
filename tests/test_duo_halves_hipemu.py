"""The two-clusters-per-wavefront broadcast kernel (csrc/duo.hip) where the two halves of a wavefront go different ways, on the host
wavefront emulator against the oracle, bit for bit: a wavefront whose upper half holds no cluster, clusters that run out of values and
stop while their partner runs on, reads that overflow the payload capacity, random and constant latency, the echo-back program on a line,
and topologies with nodes of degree above four (the generic-degree path).  Dev flag 0x400 requires the duo layout, so that a case cannot pass on another
kernel.  tests/test_duo_halves_gpu.py runs the same cases on the device."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")

CASES = [
    "{'workload':'broadcast','node_count':25,'rate':50,'time_limit':4,'n':5,'flags':0x400}",                              # odd count: the last wavefront's upper half is empty
    "{'workload':'broadcast','node_count':25,'rate':80,'time_limit':4,'n':6,'max_values':40,'seed':4,'flags':0x400}",       # values overflow: a cluster stops, its partner runs on
    "{'workload':'broadcast','node_count':25,'rate':80,'time_limit':4,'n':6,'max_payload_words':60,'seed':5,'flags':0x400}",   # read payload overflow
    "{'workload':'broadcast','node_count':25,'rate':80,'time_limit':4,'latency':10,'n':5,'max_payload_words':80,'seed':6,'flags':0x400}",
    "{'workload':'broadcast','node_count':9,'rate':60,'time_limit':4,'latency':30,'latency_dist':'uniform','n':5,'max_payload_words':50,'seed':8,'flags':0x400}",
    "duo25uni", "duo25lat10", "duo9total",
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':12,'rate':50,'time_limit':4,'topology':'line','n':3,'flags':0x400}",
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':12,'rate':50,'time_limit':4,'latency':5,'topology':'line','n':4,'flags':0x400}",
    "{'workload':'broadcast','node_count':21,'rate':50,'time_limit':4,'topology':'tree4','n':3,'flags':0x400}",           # degree 5: the generic-degree path
    "{'workload':'broadcast','node_count':10,'rate':50,'time_limit':4,'topology':'total','n':5,'max_values':30,'flags':0x400}",
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
def test_duo_halves_on_the_emulator_equal_the_oracle(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + CASES, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(CASES), r.stdout
    assert "guard: 0 damaged byte(s)" in r.stdout, r.stdout[-2000:]
