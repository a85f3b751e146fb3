"""Paired op rounds of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, latency 0, at most four neighbours): a half that
is ready for its op waits at the gossip loop's exit test (it is PARKED, for at most DUO_PAIR_WAIT wave-rounds) until its partner's flood
has ended, so that one op wave-round carries the ops of both halves.  Parking changes only the order in which two independent clusters
take their rounds: on the host wavefront emulator (lanes out of lockstep, MSIM_GUARD=3) every unflagged instance equals the oracle bit
for bit: rows, payload, meta (n_rounds included) and the six net-stats counters.  Dev flag 0x400 requires the duo layout.

CASES: the headline shape at a short time limit with 2, 4 and 7 clusters (the odd count has an empty upper half, which never parks); few
ops (rate 1: a cluster ends while its partner is parked, and the reverse); ops that meet clusters that are not quiescent (rate 2000 with
small queues, rate 3000: the partner is in generic mode, GENERAL bodies release a parked half); a line of 24 nodes, whose floods take up
to 25 rounds (the longest waits); two nodes; echo-back; the generic-degree instantiation (9 nodes, `total`), which never parks; several
blocks of draws.  The product's cap is as long as the longest flood of these shapes, so the path on which the wait runs out and the op
goes alone is run with a build of a short cap (-DDUO_PAIR_WAIT=2, emulator only: WAIT_RUNS_OUT, the headline shape and the line).  No instance of CASES or POISONED is flagged by the oracle (test_no_case_is_flagged).  POISONED
runs with every device buffer filled with 0xA5 before the launch.

STOPS: the three capacities of tests/test_duo_op_plan_hipemu.py at 2 and 4 clusters: they stop a cluster while it or its partner is
parked; every instance carries the oracle's flags (a flagged instance is compared by its flags, as everywhere in this project).

PAIR_LIMIT_CASE: two clusters under MSIM_DUO_ROUND_LIMIT = 40 .. 160.  Where a cluster in mid-flood stops depends on its partner (see the
docstring of tests/test_duo_op_plan_hipemu.py), so every instance must carry MSIM_FLAG_ROUND_LIMIT alone, have counted at least L + 1
rounds, and hold rows and a payload that are a prefix of the oracle's; exact round counts are the one-cluster sweep's of that module,
whose digests this build and a -DDUO_NO_FLOOD build must share limit for limit (there, emulator only; both sweeps are also held against
their recorded digests, tests/golden/duo_round_limits.json, by tests/test_duo_trim_hipemu.py).

THE PAIRING HAPPENS (emulator, a -DDUO_PROF build): at the headline shape the wave-rounds with an op are at most 0.65 x the broadcasts
of the wavefront's two clusters (the replay model of tools/duo_pair_estimate.py puts unpaired code at 0.92 .. 0.97 and pairing at 0.50 ..
0.54; the few reads that end a block of draws add about 0.03), there are parks, and no parked half waited longer than DUO_PAIR_WAIT.
Without this check everything above passes with the feature silently off.
tests/test_duo_pair_ops_gpu.py runs the cases on the device."""
import ast
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "hipemu", "_build", "libmaelsim_emu.so")
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HEADLINE = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':%d,'inbox_capacity':6,'seed':2026,'flags':0x400}"
CASES = [
    HEADLINE % 2, HEADLINE % 4, HEADLINE % 7,
    # few ops: a cluster ends while its partner is parked, and the reverse
    "{'workload':'broadcast','node_count':25,'rate':1,'time_limit':12,'n':4,'inbox_capacity':6,'seed':34,'flags':0x400}",
    # ops that meet clusters that are not quiescent
    "{'workload':'broadcast','node_count':25,'rate':2000,'time_limit':2,'n':4,'inbox_capacity':2,'spill_capacity':1,'seed':26,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':3000,'time_limit':2,'n':4,'seed':13,'flags':0x400}",
    # the longest floods
    "{'workload':'broadcast','node_count':24,'rate':100,'time_limit':4,'topology':'line','n':4,'seed':28,'flags':0x400}",
    "{'workload':'broadcast','node_count':2,'rate':50,'time_limit':3,'n':4,'seed':21,'flags':0x400}",
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':25,'rate':100,'time_limit':3,'n':4,'inbox_capacity':2,'spill_capacity':2,'seed':30,'flags':0x400}",
    # the generic-degree instantiation: never parks
    "{'workload':'broadcast','node_count':9,'rate':100,'time_limit':4,'topology':'total','n':4,'seed':17,'flags':0x400}",
    # several blocks of draws
    "{'workload':'broadcast','node_count':25,'rate':400,'time_limit':3,'n':4,'inbox_capacity':6,'seed':35,'flags':0x400}",
]
POISONED = ["{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':4,'inbox_capacity':6,'seed':36,'flags':0x400}"]
_STOP = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':%d,'inbox_capacity':6,%s,'seed':31,'flags':0x400}"
STOPS = [(_STOP % (n, cap), flag) for n in (2, 4) for cap, flag in (("'max_payload_words':400", 0x2), ("'max_rows':300", 0x1), ("'max_values':64", 0x8))]
WAIT_RUNS_OUT = [HEADLINE % 4, CASES[6]]
PAIR_LIMIT_CASE = HEADLINE % 2
PAIR_LIMITS = list(range(40, 161))
PAIRING_CASE = HEADLINE % 2
MSIM_FLAG_ROUND_LIMIT = 16
MSIM_F_BROADCAST = 1


def pair_wait():
    """DUO_PAIR_WAIT of the product build"""
    with open(os.path.join(ROOT, "maelstrom_amd", "csrc", "duo.hip")) as f:
        return int(re.search(r"^#define DUO_PAIR_WAIT (\d+)", f.read(), re.M).group(1))


def _config(case):
    from maelstrom_amd import engine as E
    kw = ast.literal_eval(case)
    n, flags = kw.pop("n"), kw.pop("flags")
    return E, E.test_config(seed=kw.pop("seed"), **kw), n, flags


def check_stops():
    """STOPS on whatever library MSIM_LIB names (the device library by default): every instance carries the oracle's flags"""
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


def check_pair_limits():
    """PAIR_LIMIT_CASE under every limit of PAIR_LIMITS on whatever library MSIM_LIB names"""
    import oracle_lib as O
    E, cfg, n, flags = _config(PAIR_LIMIT_CASE)
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    for lim in PAIR_LIMITS:
        os.environ["MSIM_DUO_ROUND_LIMIT"] = str(lim)
        try:
            with E.Engine(cfg) as eng:
                eng.set_dev_flags(flags)
                eng.run(0, n)
                eng.fetch()
                for i in range(n):
                    rows, pay = eng.raw_history(i)
                    orows, opay = ora.history(i)
                    m = eng.meta(i)
                    assert m.flags == MSIM_FLAG_ROUND_LIMIT, f"limit {lim}: flags of instance {i}: {m.flags:#x}"
                    assert m.n_rounds >= lim + 1, f"limit {lim}: instance {i} counted {m.n_rounds} rounds"
                    rb, pb = rows.tobytes(), pay.tobytes()
                    assert len(rb) == 16 * m.n_rows and orows.tobytes()[:len(rb)] == rb, f"limit {lim}: the rows of instance {i} are no prefix of the oracle's"
                    assert len(pb) == 4 * m.n_payload_words and opay.tobytes()[:len(pb)] == pb, f"limit {lim}: the payload of instance {i} is no prefix of the oracle's"
        finally:
            del os.environ["MSIM_DUO_ROUND_LIMIT"]
    print("pair limits: OK")


def pairing_counts():
    """PAIRING_CASE on the -DDUO_PROF library MSIM_LIB names: the counters of the one wavefront (see the epilogue of sim_kernel_duo) and
    the broadcasts of its two clusters, counted from the oracle's rows"""
    import numpy as np
    import oracle_lib as O
    E, cfg, n, flags = _config(PAIRING_CASE)
    assert n == 2
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    bcasts = 0
    for i in range(n):
        r = np.frombuffer(ora.history(i)[0].tobytes(), dtype=np.uint32).reshape(-1, 4)
        bcasts += sum(1 for w in r[:, 2] if (int(w) & 3) == 0 and ((int(w) >> 2) & 0x1FF) == MSIM_F_BROADCAST)   # invocation rows of broadcasts
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags)
        eng.run(0, n)
        eng.fetch()
        lo, up = eng.meta(0), eng.meta(1)
        for i in range(n):
            assert (eng.meta(i).n_rows, eng.meta(i).n_rounds, eng.meta(i).flags) == (ora.meta[i]["n_rows"], ora.meta[i]["n_rounds"], 0)
        return {"broadcasts": bcasts, "general": lo.n_events & 0xFFFF, "op_rounds": (lo.n_events >> 16) + (up.reserved[0] & 0xFFFF),
                "two_ops": (up.reserved[0] >> 16) & 0xFFF, "wave_rounds": lo.reserved[0] & 0xFFFF, "parks": (lo.reserved[2] >> 16) & 0x7FF,
                "longest_wait": lo.reserved[2] >> 27, "parked_rounds": up.n_events >> 16}


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


def _env(lib, **extra):
    return dict(os.environ, MSIM_LIB=lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3", **extra)


def _compare(emu_lib, cases, extra_env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + cases, cwd=ROOT, env=_env(emu_lib, **extra_env), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(cases), r.stdout
    assert "guard: 0 damaged byte(s)" in r.stdout, r.stdout[-2000:]


def _self(lib, what, timeout=800):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=_env(lib), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.timeout(1800)
def test_duo_paired_ops_on_the_emulator_equal_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(900)
def test_duo_paired_ops_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED, {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_paired_ops_on_the_emulator_when_the_wait_runs_out(emu_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools", "hipemu"))
    import build_emu
    short = build_emu.build_variant("pairw2", "duo.hip", ["-DDUO_PAIR_WAIT=2"])
    _compare(short, WAIT_RUNS_OUT, {})
    prof = build_emu.build_variant("pairw2prof", "duo.hip", ["-DDUO_PAIR_WAIT=2", "-DDUO_PROF"])
    c = json.loads(_self(prof, "pairing").strip().splitlines()[-1])
    assert c["longest_wait"] == 2 and c["op_rounds"] - c["two_ops"] > 20, f"the wait never ran out: {c}"


@pytest.mark.timeout(900)
def test_duo_paired_ops_on_the_emulator_stopped_by_a_capacity(emu_lib):
    assert "stops: OK" in _self(emu_lib, "stops")


@pytest.mark.timeout(900)
def test_duo_paired_ops_on_the_emulator_with_a_round_limit(emu_lib):
    assert "pair limits: OK" in _self(emu_lib, "pair_limits")


@pytest.mark.timeout(900)
def test_duo_op_rounds_are_paired_on_the_emulator(emu_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools", "hipemu"))
    import build_emu
    prof = build_emu.build_variant("pairprof", "duo.hip", ["-DDUO_PROF"])
    c = json.loads(_self(prof, "pairing").strip().splitlines()[-1])
    print(c)
    with_op = c["general"] + c["op_rounds"]
    assert with_op <= 0.65 * c["broadcasts"], f"{with_op} wave-rounds with an op for {c['broadcasts']} broadcasts: {c}"
    assert c["parks"] > 0 and c["parked_rounds"] >= c["parks"], c
    assert pair_wait() < 31, "the DUO_PROF build reports the longest wait in 5 bits"
    assert 1 <= c["longest_wait"] <= pair_wait(), c


if __name__ == "__main__":
    if sys.argv[1:] == ["pairing"]:
        print(json.dumps(pairing_counts()))
    elif sys.argv[1:] == ["pair_limits"]:
        check_pair_limits()
    else:
        check_stops()
