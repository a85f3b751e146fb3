"""Flood mode of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, latency 0, at most four neighbours): between two ops of a
quiescent cluster every envelope in flight carries one value, so a node's queue is kept as a count and its set word in a register, and a
wave-round whose live halves are all in that mode runs a flood body.  On the host wavefront emulator (lanes out of lockstep) against the
oracle, bit for bit: floods of one value (odd cluster counts; rings smaller than a round's arrivals, where flood mode stands aside), two
values in flight (an op that meets a cluster that is not quiescent: the GENERAL body materialises the queues, the next op round enters flood
mode again, one half leaves while its partner stays), four envelopes in flight to one node (echo-back), a topology with two neighbours,
the generic-degree instantiation (no flood mode) and two nodes.  Dev flag 0x400 requires the duo layout.

One shape overflows its inboxes (MSIM_FLAG_INBOX_OVERFLOW in all three instances).  There the kernel has always equalled the oracle in rows,
payload, meta (n_rounds included) and every send counter, and counted the dropped envelopes differently on the receive side: the receive
counters are held to the values the kernel gave before flood mode (OVERFLOW_RECV).  tests/test_duo_flood_round_gpu.py runs all of it on
the device."""
import ast
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")

CASES = [
    # one value in flight
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':7,'inbox_capacity':6,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':3,'inbox_capacity':2,'spill_capacity':1,'seed':23,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':3,'inbox_capacity':1,'spill_capacity':1,'seed':25,'flags':0x400}",
    # two values in flight: flood mode is left and entered with envelopes queued; instance 1 of the second leaves while its partner stays
    "{'workload':'broadcast','node_count':25,'rate':2000,'time_limit':2,'n':3,'inbox_capacity':2,'spill_capacity':1,'seed':26,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':3000,'time_limit':2,'n':4,'seed':13,'flags':0x400}",
    # four envelopes in flight to one node
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':25,'rate':100,'time_limit':3,'n':3,'inbox_capacity':2,'spill_capacity':2,'seed':30,'flags':0x400}",
    # two neighbours, the generic-degree instantiation, two nodes
    "{'workload':'broadcast','node_count':24,'rate':100,'time_limit':4,'topology':'line','n':3,'seed':28,'flags':0x400}",
    "{'workload':'broadcast','node_count':32,'rate':150,'time_limit':3,'topology':'tree3','n':4,'seed':20,'flags':0x400}",
    "{'workload':'broadcast','node_count':9,'rate':100,'time_limit':4,'topology':'total','n':5,'seed':17,'flags':0x400}",
    "{'workload':'broadcast','node_count':2,'rate':50,'time_limit':3,'n':3,'seed':21,'flags':0x400}",
]

OVERFLOW = "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':25,'rate':100,'time_limit':3,'n':3,'inbox_capacity':2,'spill_capacity':1,'seed':30,'flags':0x400}"
OVERFLOW_RECV = [(10840, 11564), (10754, 11474), (11082, 11812)]   # servers_recv, all_recv per instance (the oracle: 10880 / 11604, 10800 / 11520, 11120 / 11850)
MSIM_FLAG_INBOX_OVERFLOW = 1 << 0


def check_overflow_case():
    """Runs OVERFLOW on whatever library MSIM_LIB names (the device library by default); asserts as the module's docstring says."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from maelstrom_amd import engine as E
    import oracle_lib as O
    kw = ast.literal_eval(OVERFLOW)
    n, flags = kw.pop("n"), kw.pop("flags")
    cfg = E.test_config(seed=kw.pop("seed"), **kw)
    ora = O.run(cfg, 0, n)
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags)
        eng.run(0, n)
        eng.fetch()
        for i in range(n):
            rows, pay = eng.raw_history(i)
            orows, opay = ora.history(i)
            assert rows.tobytes() == orows.tobytes() and pay.tobytes() == opay.tobytes(), f"history of instance {i} differs from the oracle"
            m, om = eng.meta(i), ora.meta[i]
            assert (m.n_rows, m.n_payload_words, m.flags, m.n_rounds) == (om["n_rows"], om["n_payload_words"], om["flags"], om["n_rounds"]), f"meta of instance {i}"
            assert m.flags & E.FLAG_INBOX_OVERFLOW if hasattr(E, "FLAG_INBOX_OVERFLOW") else m.flags != 0, f"instance {i} is not flagged"
            st = eng.net_stats_raw(i)
            for f in ("all_send", "clients_send", "servers_send", "clients_recv"):
                assert int(getattr(st, f)) == int(ora.stats[i][f]), f"{f} of instance {i} differs from the oracle"
            got = (int(st.servers_recv), int(st.all_recv))
            print(f"instance {i}: servers_recv / all_recv {got[0]} / {got[1]} (expected {OVERFLOW_RECV[i][0]} / {OVERFLOW_RECV[i][1]})", flush=True)
            assert got == OVERFLOW_RECV[i], f"receive counters of instance {i}: {got}"
    print("overflow case: OK")


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which(os.environ.get("HIPEMU_CXX", "g++")) is None:
        pytest.skip("no host C++ compiler for the emulator build")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hipemu", "build_emu.py")], cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(EMU)
    return EMU


@pytest.mark.timeout(1800)
def test_duo_flood_rounds_on_the_emulator_equal_the_oracle(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + CASES, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(CASES), r.stdout
    assert "guard: 0 damaged byte(s)" in r.stdout, r.stdout[-2000:]


@pytest.mark.timeout(900)
def test_duo_flood_rounds_on_the_emulator_with_overflowing_inboxes(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "overflow case: OK" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    check_overflow_case()
