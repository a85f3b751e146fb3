"""The flood stretch of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, latency 0, at most four neighbours, paired op
rounds): the flood gossip rounds of a wavefront run in a loop of their own whose back edge tests only what can end the stretch (a half
with nothing due that is not parked, the count-down of a parked half), and the flood bodies publish fan-out masks instead of envelopes.
Every round, delivery and message is simulated as before, so on the host wavefront emulator (lanes out of lockstep, MSIM_GUARD=3) every
unflagged instance equals the oracle bit for bit: rows, payload, meta (n_rounds included) and the six net-stats counters.  Dev flag
0x400 requires the duo layout.

CASES: the headline shape at a short time limit with 2, 4 and 7 clusters (the odd count has a wavefront with an empty upper half, which
takes its rounds one by one); few ops (rate 1: a cluster ends while its partner is inside a stretch, and the reverse); a line of 24 nodes,
whose floods take up to 25 rounds, more than DUO_PAIR_WAIT = 24, so the count-down runs out inside a stretch (LINE runs again with a
-DDUO_PAIR_WAIT=2 build, emulator only); 31 nodes on the grid (node 30 is the highest bit of a fan-out mask, lane 31 the target of the
unused neighbour slots); `tree3` with 13 nodes (inner nodes use all four neighbour slots); two nodes; echo-back at an inbox capacity that
gives a ring of 8, so that flood mode is on (the fan-out that skips nobody); ops that meet clusters that are not quiescent (rate 2000
with small queues, rate 3000: one half is generic, GENERAL bodies run between stretches); several blocks of draws (rate 400).  No
instance of CASES or POISONED is flagged by the oracle (test_no_case_is_flagged).  POISONED runs with every device buffer filled with 0xA5
before the launch, in a process of its own.

STOPS (those of tests/test_duo_pair_ops_hipemu.py: the three capacities at 2 and 4 clusters) are compared by their flags, as everywhere
in this project.  The round limit: two clusters of the headline shape under MSIM_DUO_ROUND_LIMIT = 40 .. 160 with the conditions of that
module's check_pair_limits.  That the limit is looked at at the same rounds as without the stretch is held by the one-cluster sweep of
tests/test_duo_op_plan_hipemu.py (this build against a -DDUO_NO_FLOOD build, limit for limit) and by the recorded digests of both sweeps
(tests/golden/duo_round_limits.json, tests/test_duo_trim_hipemu.py).

THE STRETCH HAPPENS (emulator, a -DDUO_PROF -DDUO_PROF_STRETCH build): at the headline shape the rounds taken inside stretches are at
least 0.9 x (flood gossip rounds + parked rounds), and there are fewer stretches than such rounds.  Beyond that: a stretch ends when
the flood of one of the two halves has ended (or a count-down has), a flood on the 5 x 5 grid lasts at least 5 rounds (the eccentricity
of its centre is 4), and the two halves' floods start together after a paired op round, so two floods end at most two stretches per 5
rounds: the stretches are at most 0.4 x the rounds taken inside them.  Without these checks everything above passes with the loop
silently dead.  tests/test_duo_stretch_gpu.py runs the cases on the device."""
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

from test_duo_pair_ops_hipemu import STOPS, _config, check_pair_limits, check_stops  # noqa: E402,F401

HEADLINE = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':%d,'inbox_capacity':6,'seed':2026,'flags':0x400}"
LINE = "{'workload':'broadcast','node_count':24,'rate':100,'time_limit':4,'topology':'line','n':4,'seed':28,'flags':0x400}"
CASES = [
    HEADLINE % 2, HEADLINE % 4, HEADLINE % 7,
    # few ops: a cluster ends while its partner is inside a stretch, and the reverse
    "{'workload':'broadcast','node_count':25,'rate':1,'time_limit':12,'n':4,'inbox_capacity':6,'seed':34,'flags':0x400}",
    # floods longer than the wait of a parked half
    LINE,
    # the highest bit of a fan-out mask; all four neighbour slots; two nodes
    "{'workload':'broadcast','node_count':31,'rate':100,'time_limit':4,'n':4,'inbox_capacity':6,'seed':41,'flags':0x400}",
    "{'workload':'broadcast','node_count':13,'rate':100,'time_limit':4,'topology':'tree3','n':4,'inbox_capacity':6,'seed':42,'flags':0x400}",
    "{'workload':'broadcast','node_count':2,'rate':50,'time_limit':3,'n':4,'seed':21,'flags':0x400}",
    # echo-back with a ring of 8: flood mode, the fan-out that skips nobody
    "{'workload':'broadcast','bin':'broadcast-ff-echoback','node_count':25,'rate':100,'time_limit':3,'n':4,'inbox_capacity':6,'seed':43,'flags':0x400}",
    # ops that meet clusters that are not quiescent
    "{'workload':'broadcast','node_count':25,'rate':2000,'time_limit':2,'n':4,'inbox_capacity':2,'spill_capacity':1,'seed':26,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':3000,'time_limit':2,'n':4,'seed':13,'flags':0x400}",
    # several blocks of draws
    "{'workload':'broadcast','node_count':25,'rate':400,'time_limit':3,'n':4,'inbox_capacity':6,'seed':35,'flags':0x400}",
]
POISONED = ["{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':4,'inbox_capacity':6,'seed':44,'flags':0x400}"]
STRETCH_CASE = HEADLINE % 2


def stretch_counts():
    """STRETCH_CASE on the -DDUO_PROF -DDUO_PROF_STRETCH library MSIM_LIB names: the counters of the one wavefront (see the epilogue of
    sim_kernel_duo)"""
    import oracle_lib as O
    E, cfg, n, flags = _config(STRETCH_CASE)
    assert n == 2
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags)
        eng.run(0, n)
        eng.fetch()
        lo, up = eng.meta(0), eng.meta(1)
        for i in range(n):
            assert (eng.meta(i).n_rows, eng.meta(i).n_rounds, eng.meta(i).flags) == (ora.meta[i]["n_rows"], ora.meta[i]["n_rounds"], 0)
        return {"stretches": lo.n_events & 0xFFFF, "stretch_rounds": lo.n_events >> 16, "flood_gossip_rounds": up.n_events & 0xFFFF,
                "parked_rounds": up.n_events >> 16, "generic_gossip_rounds": lo.reserved[1] & 0xFFFF, "wave_rounds": lo.reserved[0] & 0xFFFF}


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


def _variant(tag, flags):
    sys.path.insert(0, os.path.join(ROOT, "tools", "hipemu"))
    import build_emu
    return build_emu.build_variant(tag, "duo.hip", flags)


def _env(lib, **extra):
    return dict(os.environ, MSIM_LIB=lib, HIPEMU_DIVERGENT="1", MSIM_GUARD="3", **extra)


def _compare(lib, cases, extra_env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + cases, cwd=ROOT, env=_env(lib, **extra_env), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(cases), r.stdout
    assert "guard: 0 damaged byte(s)" in r.stdout, r.stdout[-2000:]


def _self(lib, what, timeout=800):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=_env(lib), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.timeout(1800)
def test_duo_stretch_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(900)
def test_duo_stretch_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED, {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_stretch_on_the_emulator_when_the_wait_runs_out(emu_lib):
    _compare(_variant("stretchw2", ["-DDUO_PAIR_WAIT=2"]), [LINE, HEADLINE % 4], {})


@pytest.mark.timeout(900)
def test_duo_stretch_on_the_emulator_stopped_by_a_capacity(emu_lib):
    assert "stops: OK" in _self(emu_lib, "stops")


@pytest.mark.timeout(900)
def test_duo_stretch_on_the_emulator_with_a_round_limit(emu_lib):
    assert "pair limits: OK" in _self(emu_lib, "pair_limits")


@pytest.mark.timeout(900)
def test_duo_flood_rounds_are_taken_in_stretches_on_the_emulator(emu_lib):
    prof = _variant("stretchprof", ["-DDUO_PROF", "-DDUO_PROF_STRETCH"])
    c = json.loads(_self(prof, "stretch").strip().splitlines()[-1])
    print(c)
    flood = c["flood_gossip_rounds"] + c["parked_rounds"]
    assert flood > 500, c
    assert c["stretch_rounds"] >= 0.9 * flood, f"{c['stretch_rounds']} rounds inside stretches of {flood} flood gossip and parked rounds: {c}"
    assert 0 < c["stretches"] < c["stretch_rounds"], c
    assert c["stretches"] <= 0.4 * c["stretch_rounds"], f"{c['stretches']} stretches for {c['stretch_rounds']} rounds: {c}"


if __name__ == "__main__":
    if sys.argv[1:] == ["stretch"]:
        print(json.dumps(stretch_counts()))
    elif sys.argv[1:] == ["pair_limits"]:
        check_pair_limits()
    else:
        check_stops()
