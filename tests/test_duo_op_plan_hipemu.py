"""Read runs of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, latency 0, at most four neighbours): an op round of a
quiescent cluster executes the reads that lie ahead of its next broadcast (or of the end of what an op round may take) as cluster rounds
of their own inside one wave-round, and the block of generator draws lives in LDS.  On the host wavefront emulator (lanes out of
lockstep) against the oracle, bit for bit: rows, payload, meta (n_rounds included) and the six net-stats counters.  Dev flag 0x400
requires the duo layout.

CASES: the headline shape at a short time limit with an odd cluster count (an empty upper half); a cutoff inside the first block of draws
and a run that the cutoff ends (time_limit 0.35, rate 1); ops that meet a cluster that is not quiescent (rate 2000 and 3000: the GENERAL
body takes them, one half leaves flood mode while its partner stays); echo-back; a line of 24 nodes; two nodes; the generic-degree
instantiation (9 nodes, `total`: no runs); a shape with several blocks of draws per cluster.  No instance of CASES is flagged by the
oracle (test_no_case_is_flagged).  POISONED runs with every device buffer filled with 0xA5 before the launch.

STOPS: a payload, a row and a value capacity that end a cluster inside a run (the oracle flags 0x2, 0x1 and 0x8 in all three instances).
As everywhere in this project a flagged instance is compared by its flags.

LIMIT_CASE: a round limit that falls inside a run of reads.  The oracle's limit is fixed at 50 000 000 rounds, so the kernel's is set
through MSIM_DUO_ROUND_LIMIT and swept over LIMITS, round by round.  The kernel looks at the limit in R0 of a wave-round in which one of
the wavefront's halves has nothing due, for both halves, so where a cluster in mid-flood stops depends on its partner; the case is
therefore ONE cluster (the upper half is empty, the limit is looked at in every round), and then, for every limit L, the cluster must
carry MSIM_FLAG_ROUND_LIMIT alone, have counted exactly L + 1 rounds (R0 of round L + 1 finds rounds >= L and forces a GENERAL round,
whose scheduler's view stops the cluster), and hold a history and payload that are a prefix of the oracle's, bit for bit.  The sweep
must contain limits at which the last three ops the cluster executed were read, read, op and the two limits before each stopped the
cluster one op earlier: then the three ran in rounds L - 1, L and L + 1, the second read in round L behind the first read of its run,
where the run's own test of the limit decides.  On the emulator the
library built with -DDUO_NO_FLOOD (no flood mode, so no runs, pairs or stretches: the generic code that the other instantiations of the
kernel run) must give the same digests, limit for limit.  This is the one live build-against-build test of the one-cluster sweep; the
sweep's digests are also recorded in tests/golden/duo_round_limits.json (see tests/test_duo_trim_hipemu.py).
tests/test_duo_op_plan_gpu.py runs all of this on the device (but for the -DDUO_NO_FLOOD build)."""
import ast
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CASES = [
    # a. the headline shape, short, seven clusters
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':7,'inbox_capacity':6,'seed':2026,'flags':0x400}",
    # b. a cutoff inside the first block of draws; a handful of ops
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':0.35,'n':5,'inbox_capacity':6,'seed':33,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':1,'time_limit':12,'n':5,'inbox_capacity':6,'seed':34,'flags':0x400}",
    # c. ops that meet a cluster that is not quiescent
    "{'workload':'broadcast','node_count':25,'rate':2000,'time_limit':2,'n':3,'inbox_capacity':2,'spill_capacity':1,'seed':26,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':3000,'time_limit':2,'n':4,'seed':13,'flags':0x400}",
    # e. echo-back, f. a line of 24 nodes, g. two nodes, h. the generic-degree instantiation
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':25,'rate':100,'time_limit':3,'n':3,'inbox_capacity':2,'spill_capacity':2,'seed':30,'flags':0x400}",
    "{'workload':'broadcast','node_count':24,'rate':100,'time_limit':4,'topology':'line','n':3,'seed':28,'flags':0x400}",
    "{'workload':'broadcast','node_count':2,'rate':50,'time_limit':3,'n':3,'seed':21,'flags':0x400}",
    "{'workload':'broadcast','node_count':9,'rate':100,'time_limit':4,'topology':'total','n':5,'seed':17,'flags':0x400}",
    # more than one block of draws per cluster, with long runs
    "{'workload':'broadcast','node_count':25,'rate':400,'time_limit':3,'n':4,'inbox_capacity':6,'seed':35,'flags':0x400}",
]
# j. one case under MSIM_POISON=0xA5
POISONED = ["{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':5,'inbox_capacity':6,'seed':36,'flags':0x400}"]
# d. capacities that stop a cluster: (case, the flag every instance carries)
STOPS = [
    ("{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':3,'inbox_capacity':6,'max_payload_words':400,'seed':31,'flags':0x400}", 0x2),
    ("{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':3,'inbox_capacity':6,'max_rows':300,'seed':31,'flags':0x400}", 0x1),
    ("{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':3,'inbox_capacity':6,'max_values':64,'seed':31,'flags':0x400}", 0x8),
]
# i. a round limit inside a run of reads (see the docstring)
LIMIT_CASE = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':1,'inbox_capacity':6,'seed':37,'flags':0x400}"
LIMITS = list(range(40, 200))
MSIM_FLAG_ROUND_LIMIT = 16


def _config(case):
    from maelstrom_amd import engine as E
    kw = ast.literal_eval(case)
    n, flags = kw.pop("n"), kw.pop("flags")
    return E, E.test_config(seed=kw.pop("seed"), **kw), n, flags


def check_stops():
    """Runs STOPS on whatever library MSIM_LIB names (the device library by default): every instance carries the oracle's flags."""
    import oracle_lib as O
    for case, flag in STOPS:
        E, cfg, n, flags = _config(case)
        ora = O.run(cfg, 0, n)
        with E.Engine(cfg) as eng:
            eng.set_dev_flags(flags)
            eng.run(0, n)
            eng.fetch()
            for i in range(n):
                got, want = eng.meta(i).flags, int(ora.meta[i]["flags"])
                print(f"{case}: instance {i} flags {got:#x} (oracle {want:#x})", flush=True)
                assert want == flag, f"{case}: the oracle flags instance {i} {want:#x}, not {flag:#x}"
                assert got == want, f"{case}: flags of instance {i}: {got:#x}, the oracle {want:#x}"
    print("stops: OK")


def limit_sweep():
    """LIMIT_CASE under every limit of LIMITS on whatever library MSIM_LIB names; the prefix checks against the oracle; returns
    {limit: [digest per instance]} and the number of (limit, instance) pairs at which the limit fell behind the first read of a run"""
    import numpy as np
    import oracle_lib as O
    E, cfg, n, flags = _config(LIMIT_CASE)
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    out, inside, n_rows_at = {}, 0, {}
    for lim in LIMITS:
        os.environ["MSIM_DUO_ROUND_LIMIT"] = str(lim)
        try:
            with E.Engine(cfg) as eng:
                eng.set_dev_flags(flags)
                eng.run(0, n)
                eng.fetch()
                dig = []
                for i in range(n):
                    rows, pay = eng.raw_history(i)
                    orows, opay = ora.history(i)
                    m, st = eng.meta(i), eng.net_stats_raw(i)
                    assert m.flags == MSIM_FLAG_ROUND_LIMIT, f"limit {lim}: flags of instance {i}: {m.flags:#x}"
                    assert m.n_rounds == lim + 1, f"limit {lim}: instance {i} counted {m.n_rounds} rounds"
                    rb, pb = rows.tobytes(), pay.tobytes()
                    assert len(rb) == 16 * m.n_rows and orows.tobytes()[:len(rb)] == rb, f"limit {lim}: the rows of instance {i} are no prefix of the oracle's"
                    assert len(pb) == 4 * m.n_payload_words and opay.tobytes()[:len(pb)] == pb, f"limit {lim}: the payload of instance {i} is no prefix of the oracle's"
                    r = np.frombuffer(rb, dtype=np.uint32).reshape(-1, 4)
                    kinds = [int(w >> 2) & 0x1FF for w in r[0::2, 2]]   # the ops' functions, invocation rows
                    n_rows_at[(lim, i)] = m.n_rows
                    if (len(kinds) >= 3 and kinds[-3] == 2 and kinds[-2] == 2 and   # MSIM_F_READ
                            n_rows_at.get((lim - 1, i)) == m.n_rows - 2 and n_rows_at.get((lim - 2, i)) == m.n_rows - 4):
                        inside += 1
                    dig.append([m.n_rows, m.n_payload_words, m.flags, m.n_rounds, hashlib.sha256(rb + pb).hexdigest()] +
                               [int(getattr(st, f)) for f in ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv")])
                out[str(lim)] = dig
        finally:
            del os.environ["MSIM_DUO_ROUND_LIMIT"]
    return out, inside


def test_no_case_is_flagged():
    """the oracle alone: no instance of CASES or POISONED carries a flag"""
    import oracle_lib as O
    for case in CASES + POISONED:
        _, cfg, n, _ = _config(case)
        ora = O.run(cfg, 0, n)
        assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n, case


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
def test_duo_read_runs_on_the_emulator_equal_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(900)
def test_duo_read_runs_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED, {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_read_runs_on_the_emulator_stopped_by_a_capacity(emu_lib):
    env = dict(os.environ, MSIM_LIB=emu_lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "stops: OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.timeout(1800)
def test_duo_read_runs_on_the_emulator_with_a_round_limit_inside_a_run(emu_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools", "hipemu"))
    import build_emu
    noflood = build_emu.build_variant("noflood", "duo.hip", ["-DDUO_NO_FLOOD"])
    got = {}
    for tag, lib in (("runs", emu_lib), ("noflood", noflood)):
        env = dict(os.environ, MSIM_LIB=lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "limits"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=800)
        assert r.returncode == 0, tag + ": " + r.stdout[-3000:] + r.stderr[-3000:]
        got[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["runs"]["inside"] >= 5, f"only {got['runs']['inside']} limits fell behind the first read of a run"
    assert sorted(got["runs"]["digests"]) == sorted(str(x) for x in LIMITS)
    diff = [k for k in got["runs"]["digests"] if got["runs"]["digests"][k] != got["noflood"]["digests"][k]]
    assert not diff, f"the builds with and without flood mode differ at the limits {diff[:10]}"


if __name__ == "__main__":
    if sys.argv[1:] == ["limits"]:
        d, inside = limit_sweep()
        print(json.dumps({"digests": d, "inside": inside}))
    else:
        check_stops()
