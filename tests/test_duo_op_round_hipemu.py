"""The op round of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, latency 0): a cluster whose scheduler acts while the
cluster is quiescent runs its generator's op in a gossip round plus the op, and every other GENERAL round keeps the full body.  On the
host wavefront emulator against the oracle, bit for bit: one half with an op round while the other gossips and both halves with op
rounds (several clusters per launch), reads in op rounds with and without a payload overflow, requests that queue behind gossip (high
rates: the generator's next op is due before the cluster is quiescent), the op that ends the main phase (every case), values and rows
running out, an odd cluster count, the echo-back program and the generic-degree path.  Dev flag 0x400 requires the duo layout.
tests/test_duo_op_round_gpu.py runs the same cases on the device."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")

CASES = [
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':7,'inbox_capacity':6,'flags':0x400}",                         # odd count
    "{'workload':'broadcast','node_count':25,'rate':400,'time_limit':3,'n':4,'seed':12,'flags':0x400}",                                  # busy clusters: requests queue behind gossip
    "{'workload':'broadcast','node_count':25,'rate':3000,'time_limit':2,'n':4,'seed':13,'flags':0x400}",                                 # next op due at once (gen_next == T)
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':6,'max_payload_words':90,'seed':14,'flags':0x400}",           # read payload overflow in op rounds
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':6,'max_values':70,'seed':15,'flags':0x400}",                  # values run out
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':6,'max_values':33,'seed':16,'flags':0x400}",                  # values run out at a word boundary
    "{'workload':'broadcast','node_count':9,'rate':100,'time_limit':4,'topology':'total','n':5,'seed':17,'flags':0x400}",                 # generic degree
    "{'workload':'broadcast','node_count':21,'rate':200,'time_limit':3,'topology':'tree4','n':4,'seed':18,'flags':0x400}",                # generic degree
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':16,'rate':100,'time_limit':3,'topology':'line','n':3,'seed':19,'flags':0x400}",
    "{'workload':'broadcast','node_count':32,'rate':150,'time_limit':3,'topology':'tree3','n':4,'seed':20,'flags':0x400}",               # 32 nodes: every lane holds one
    "{'workload':'broadcast','node_count':2,'rate':50,'time_limit':3,'n':3,'seed':21,'flags':0x400}",
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
def test_duo_op_rounds_on_the_emulator_equal_the_oracle(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + CASES, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(CASES), r.stdout
    assert "guard: 0 damaged byte(s)" in r.stdout, r.stdout[-2000:]
