"""The quiet op round of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, the flood instantiation: latency 0, at
most four neighbours): an op wave-round in which every live half acts, from flood mode, takes a body of
its own.  Such a half is quiescent, so the round's gossip part has nothing to do and the exchange would only find what every lane reads
off its own registers: a lane receives the broadcast iff bit `picked` of its own adjacency mask is set (the neighbour relation is
symmetric; the emulator build asserts it), and the poll would take that envelope out of an empty queue.  Every round, delivery and
message is simulated as before, so on the host wavefront emulator (lanes out of lockstep, MSIM_GUARD=3) every unflagged instance equals
the oracle bit for bit: rows, payload, meta (n_rounds included) and the six net-stats counters.  The emulator build also traps when a
half that takes the quiet body is not quiescent.

CASES: those of tests/test_duo_trim_hipemu.py (more than 32 broadcasts per cluster, 7 clusters: an empty upper half, a single cluster, 31
nodes, two nodes, echo-back, rate 2000 / 3000: halves outside flood mode beside flood halves, several blocks of draws, FEW_VALUES), which
hold two of the TOPOLOGIES that exercise the neighbour test already (`tree3` with 13 nodes: four neighbour slots, node numbers that are
not adjacent; a line of 24 nodes), and a partial grid of 7 nodes (side * side != n: the grid's last row is short).  All of them run again
on a -DDUO_PAIR_WAIT=2 build, where many op rounds carry one op: the superset body and the quiet one alternate inside a wavefront.
GPU_CASES are the same shapes at a time limit of at most 1 s (tests/test_duo_quiet_op_gpu.py).  No instance of any of them is flagged by
the oracle (test_no_case_is_flagged).  POISONED + [FEW_VALUES] run with every device buffer filled with 0xA5, in a process of their own;
the three capacity stops are compared by their flags, as everywhere in this project.

ROUND LIMITS.  An unflagged instance never ends with an envelope in flight, so the oracle cannot see a delivery that skips the queue at a stop.
Under MSIM_DUO_ROUND_LIMIT a cluster stops in the middle of a flood; what the kernel gives there, limit for limit, is held by the
one-cluster sweep of tests/test_duo_op_plan_hipemu.py against a -DDUO_NO_FLOOD build and by the recorded digests of that sweep and of two
clusters of the headline shape under the limits 40 .. 160 (tests/golden/duo_round_limits.json, tests/test_duo_trim_hipemu.py).

THE BODY IS TAKEN (a -DDUO_PROF emulator build, two clusters of the headline shape): at least half of the op wave-rounds are quiet ones.
This is a floor against a vacuous pass, not a measurement (the 4096-cluster profile has 1017 of 1046)."""
import ast
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_duo_stretch_hipemu as S  # noqa: E402
import test_duo_trim_hipemu as T  # noqa: E402
from test_duo_stretch_hipemu import HEADLINE, LINE, POISONED, _compare, _config, _variant, check_stops, emu_lib  # noqa: E402,F401
from test_duo_trim_hipemu import FEW_VALUES  # noqa: E402

TREE3 = "{'workload':'broadcast','node_count':13,'rate':100,'time_limit':4,'topology':'tree3','n':4,'inbox_capacity':6,'seed':42,'flags':0x400}"
GRID7 = "{'workload':'broadcast','node_count':7,'rate':100,'time_limit':4,'n':4,'inbox_capacity':6,'seed':61,'flags':0x400}"
TOPOLOGIES = [TREE3, LINE, GRID7]
assert TREE3 in T.CASES and LINE in T.CASES
CASES = T.CASES + [GRID7]
QUIET_CASE = HEADLINE % 2


def _short(case):
    """the case at a time limit of at most 1 s of virtual time"""
    kw = ast.literal_eval(case)
    kw["time_limit"] = min(kw["time_limit"], 1)
    return repr(kw)


GPU_CASES = [_short(c) for c in CASES]
GPU_POISONED = [_short(c) for c in POISONED + [FEW_VALUES]]


def quiet_counts():
    """QUIET_CASE on the -DDUO_PROF library MSIM_LIB names: the op wave-rounds of the one wavefront and how many took the quiet body (see
    the epilogue of sim_kernel_duo)"""
    import oracle_lib as O
    E, cfg, n, flags = _config(QUIET_CASE)
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
        return {"generic_op_rounds": lo.n_events >> 16, "flood_op_rounds": up.reserved[0] & 0xFFFF, "quiet_op_rounds": lo.reserved[1] >> 21,
                "two_ops": (up.reserved[0] >> 16) & 0xFFF}


def test_no_case_is_flagged():
    """the oracle alone: no instance of the added cases, at either length, carries a flag (tests/test_duo_trim_hipemu.py checks its own)"""
    import oracle_lib as O
    for case in [GRID7] + GPU_CASES + GPU_POISONED:
        _, cfg, n, _ = _config(case)
        ora = O.run(cfg, 0, n)
        assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n, case


def _self(lib, what, timeout=800):
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=S._env(lib), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.timeout(1800)
def test_duo_quiet_op_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(1800)
def test_duo_quiet_op_on_the_emulator_beside_one_op_rounds(emu_lib):
    _compare(_variant("quietw2", ["-DDUO_PAIR_WAIT=2"]), CASES, {})


@pytest.mark.timeout(900)
def test_duo_quiet_op_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED + [FEW_VALUES], {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_quiet_op_on_the_emulator_stopped_by_a_capacity(emu_lib):
    assert "stops: OK" in _self(emu_lib, "stops")


@pytest.mark.timeout(900)
def test_duo_op_rounds_take_the_quiet_body_on_the_emulator(emu_lib):
    prof = _variant("quietprof", ["-DDUO_PROF"])
    c = json.loads(_self(prof, "quiet").strip().splitlines()[-1])
    print(c)
    op_rounds = c["generic_op_rounds"] + c["flood_op_rounds"]
    assert op_rounds > 50, c
    assert c["quiet_op_rounds"] <= c["flood_op_rounds"], c
    assert 2 * c["quiet_op_rounds"] >= op_rounds, f"{c['quiet_op_rounds']} quiet op rounds of {op_rounds} op wave-rounds: {c}"


if __name__ == "__main__":
    if sys.argv[1:] == ["quiet"]:
        print(json.dumps(quiet_counts()))
    else:
        check_stops()
