"""The two-clusters-per-wavefront broadcast kernel (csrc/duo.hip) with the nodes' seen sets in HBM scratch (a region per cluster,
word-major), on the host wavefront emulator against the oracle, bit for bit: the headline shape on a few clusters, reads of whole sets,
sets that fill every word, an odd cluster count (the last wavefront's upper half holds no cluster and shares the lower one's region),
latency 10 constant / uniform / exponential, the echo-back program, a topology of degree above four and the largest set region
(max_values 8160).  The sets must not depend on what the scratch held before: a second pass fills every device buffer with a
non-zero byte before each launch (MSIM_POISON).  Dev flag 0x400 requires the duo layout, so that a case cannot pass on another kernel.
tests/test_duo_hbm_sets_gpu.py runs the same cases on the device."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")

CASES = [
    # the headline shape (bench.py headline_config) on a few clusters
    "{'workload':'broadcast','bin':'broadcast-ff','node_count':25,'rate':100,'time_limit':20,'inbox_capacity':6,'topology':'grid','n':4,'seed':21,'flags':0x400}",
    # read-heavy: many reads per second, several readers of one cluster in a round copy whole sets
    "{'workload':'broadcast','node_count':25,'rate':400,'time_limit':3,'inbox_capacity':6,'n':4,'seed':22,'flags':0x400}",
    # values up to max_values: the sets fill all W words (some clusters run out of values)
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'max_values':192,'n':4,'seed':23,'flags':0x400}",
    # odd cluster count
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'inbox_capacity':6,'n':5,'seed':24,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'latency':10,'n':3,'seed':25,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'latency':10,'latency_dist':'uniform','n':3,'seed':26,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'latency':10,'latency_dist':'exponential','n':3,'seed':27,'flags':0x400}",
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':25,'rate':100,'time_limit':4,'topology':'grid','n':3,'seed':28,'flags':0x400}",
    "{'workload':'broadcast','node_count':21,'rate':100,'time_limit':4,'topology':'tree4','n':3,'seed':29,'flags':0x400}",   # degree 5
    # the largest set region a configuration can have (max_values 8160: W = 255 words per node), odd cluster count
    "{'workload':'broadcast','node_count':32,'rate':100,'time_limit':4,'topology':'total','max_values':8160,'n':3,'seed':30,'flags':0x400}",
]
POISONED = [CASES[0], CASES[2], CASES[3], CASES[4], CASES[6], CASES[9]]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which(os.environ.get("HIPEMU_CXX", "g++")) is None:
        pytest.skip("no host C++ compiler for the emulator build")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hipemu", "build_emu.py")], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(EMU)
    return EMU


def _compare(emu_lib, cases, extra_env):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3", **extra_env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + cases, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(cases), r.stdout
    assert "guard: 0 damaged byte(s)" in r.stdout, r.stdout[-2000:]


@pytest.mark.timeout(1800)
def test_duo_hbm_sets_on_the_emulator_equal_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(1800)
def test_duo_hbm_sets_do_not_depend_on_what_the_scratch_held(emu_lib):
    _compare(emu_lib, POISONED, {"MSIM_POISON": "0xA5"})
