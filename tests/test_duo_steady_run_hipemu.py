"""The steady run of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, the memo instantiation: latency 0, at most four
neighbours; -DDUO_NO_STEADY_RUN compiles it out): the loop of the read runs also takes a broadcast whose flood the wavefront remembers,
as a cluster round of its own (the pick, the two rows, next_value, the set word's bit, the recorded rises of n_arr and rounds, the time
jump and the next round's count), so that a half goes from one block of 32 generator draws to the next inside the loop and the quiet
body, the tail and the head of an op wave-round are paid once per block.  What a cluster computes is what it always computed, so on the
host wavefront emulator (lanes out of lockstep, MSIM_GUARD=3) every unflagged instance equals the oracle bit for bit: rows, payload, meta
(n_rounds included) and the six net-stats counters.

CASES are those of tests/test_duo_flood_memo_hipemu.py, each a handful of clusters at a time limit of at most 1 s of virtual time; the
smallest shapes at which the run can go wrong: 2, 4 and 5 nodes at rate 100 (more than 32 broadcasts per cluster: a broadcast inside a run
crosses a set-word boundary, and a cluster goes through three blocks of draws), MANY_BROADCASTS (two word boundaries), rate 400 (several
blocks), the odd cluster counts (a wavefront with one live half), the line of 24 (halves that drift: one replays while its partner
simulates), rate 2000 and 3000 (halves that are not quiet: the run takes reads only), FEW_OPS (nothing is remembered).  The order of
the sets: a read that follows a broadcast of the same run copies the set from HBM and must see that broadcast's bit;
test_a_read_follows_a_remembered_broadcast_inside_one_block finds, on the oracle alone, such a pair in the 2-node case.  All cases run
again on a -DDUO_PAIR_WAIT=2 build; POISONED run with every device buffer filled with 0xA5, in a process of their own.

CAPACITIES INSIDE A RUN (capacity_sweeps): two clusters of the 2-node case with max_rows, max_payload_words (eight consecutive values
each) and max_values (30 to 34, 62 to 66) chosen, from the oracle's rows of the uncapped run, so that the stop falls behind ops the run
takes; flags are compared as check_stops does, and every unflagged instance equals the oracle in full.

BUILD AGAINST BUILD.  Under MSIM_DUO_ROUND_LIMIT the one-cluster LIMITS sweep and the two-cluster PAIR_LIMITS sweep must give, limit for
limit and at both pair waits, what a -DDUO_NO_STEADY_RUN build gives (which compiles to the previous kernel): rows, payload, meta and
all six counters.  Under such limits the run takes reads only (a half is never FAR from the limit), so the limit is found where it was.

THE PATH IS TAKEN (a -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN emulator build, two clusters of the headline shape).  Per wavefront
    op wave-rounds <= ceil(ops of the busier cluster / 31) + floods recorded + recordings dropped + broadcasts taken outside the quiet body + 2,
a condition, not a tolerance: an op wave-round ends only where a half's run ends, at the last draw of a block or at an op the run does
not take.  The same count on a -DDUO_NO_STEADY_RUN build of the same profile lies above that bound (else the check would say nothing).
The -DDUO_MEMO_VERIFY build, which takes no broadcast into a run and simulates every remembered flood, runs every case without a trap."""
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
from test_duo_flood_memo_hipemu import ADDED, CASES, MSIM_F_BROADCAST, POISONED, limit_sweeps  # noqa: E402,F401
from test_duo_stretch_hipemu import HEADLINE, _compare, _config, _variant, check_stops, emu_lib  # noqa: E402,F401
from test_duo_trim_hipemu import NET, PAIR_LIMITS  # noqa: E402

TWO_NODES = ADDED[0]   # 2 nodes at rate 100
RUN_CASE = HEADLINE % 2
PROF_FLAGS = ["-DDUO_PROF", "-DDUO_PROF_MEMO", "-DDUO_PROF_RUN"]
SWEEP_OP = 40   # the op of the 2-node case at which the swept capacities begin to stop a cluster: inside the second block of draws


def _ops(ora, i, n_nodes):
    """the generator's ops of instance i in order, from the oracle's invocation rows: (is a broadcast, node, payload words of a read's
    completion); the final reads, one per node, are left out"""
    import numpy as np
    rows, _ = ora.history(i)
    r = np.frombuffer(rows.tobytes(), dtype=np.uint32).reshape(-1, 4)
    inv, done = r[(r[:, 2] & 3) == 0], r[(r[:, 2] & 3) != 0]
    assert len(inv) == len(done)
    ops = [(((int(a[2]) >> 2) & 0x1FF) == MSIM_F_BROADCAST, int(a[2]) >> 12, (int(b[1]) >> 16) & 0xFF) for a, b in zip(inv, done)]
    final = ops[len(ops) - n_nodes:]
    assert sorted(o[1] for o in final) == list(range(n_nodes)) and not any(o[0] for o in final)
    return ops[:len(ops) - n_nodes]


def _taken_by_a_run(ops, j):
    """by the oracle's rows alone: op j is not a block's last draw and is a read or a broadcast from an origin seen before"""
    return j % 32 < 31 and (not ops[j][0] or any(o[0] and o[1] == ops[j][1] for o in ops[:j]))


def _equals_the_oracle(eng, ora, i):
    rows, pay = eng.raw_history(i)
    orows, opay = ora.history(i)
    m, st = eng.meta(i), eng.net_stats_raw(i)
    assert rows.tobytes() == orows.tobytes() and pay.tobytes() == opay.tobytes(), f"history of instance {i}"
    assert (m.n_rows, m.n_payload_words, m.n_rounds) == (int(ora.meta[i]["n_rows"]), int(ora.meta[i]["n_payload_words"]), int(ora.meta[i]["n_rounds"])), f"meta of instance {i}"
    for f in NET:
        assert int(getattr(st, f)) == int(ora.stats[i][f]), f"{f} of instance {i}"


def capacity_sweeps():
    """Two clusters of TWO_NODES on whatever library MSIM_LIB names (the device library by default), each capacity swept over values at
    which, by the oracle's rows of the uncapped run, the cluster stops behind ops a run takes; returns the number of flagged instances"""
    import oracle_lib as O
    from maelstrom_amd import engine as E
    kw = ast.literal_eval(TWO_NODES)
    kw["n"] = 2
    flags, seed, n = kw.pop("flags"), kw.pop("seed"), kw.pop("n")
    free = O.run(E.test_config(seed=seed, **kw), 0, n)
    ops = [_ops(free, i, kw["node_count"]) for i in range(n)]
    # rows: two per op; the payload in front of op SWEEP_OP, in words; the ops around the stop are ops a run takes
    for o in ops:
        assert len(o) > SWEEP_OP + 8 and all(_taken_by_a_run(o, j) for j in range(SWEEP_OP - 2, SWEEP_OP + 5)), o[SWEEP_OP - 2:SWEEP_OP + 5]
        assert sum(1 for x in o[:SWEEP_OP - 2] if x[0]) > 2 and any(not x[0] for x in o[SWEEP_OP:SWEEP_OP + 8])
    pay0 = min(sum(x[2] for x in o[:SWEEP_OP]) for o in ops)
    sweeps = [("max_rows", list(range(2 * SWEEP_OP, 2 * SWEEP_OP + 8))), ("max_payload_words", list(range(pay0, pay0 + 8))),
              ("max_values", list(range(30, 35)) + list(range(62, 67)))]
    flagged = {k: 0 for k, _ in sweeps}
    for key, values in sweeps:
        for v in values:
            cfg = E.test_config(seed=seed, **dict(kw, **{key: v}))
            ora = O.run(cfg, 0, n)
            with E.Engine(cfg) as eng:
                eng.set_dev_flags(flags)
                eng.run(0, n)
                eng.fetch()
                for i in range(n):
                    got, want = eng.meta(i).flags, int(ora.meta[i]["flags"])
                    print(f"{key}={v}: instance {i} flags {got:#x} (oracle {want:#x})", flush=True)
                    assert got == want, f"{key}={v}: flags of instance {i}: {got:#x}, the oracle {want:#x}"
                    if want == 0:
                        _equals_the_oracle(eng, ora, i)
                    else:
                        flagged[key] += 1
    # rows and payload stop every instance at every value; the value counts 30 to 34 and 62 to 66 stop the clusters that make more
    assert flagged["max_rows"] == 8 * n and flagged["max_payload_words"] == 8 * n and flagged["max_values"] > 0, flagged
    print("capacities inside a run: OK", flagged)
    return flagged


def run_counts():
    """RUN_CASE on the -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN library MSIM_LIB names, checked against the oracle: the counters of the
    one wavefront (see the epilogue of sim_kernel_duo) and the ops of its busier cluster"""
    import oracle_lib as O
    E, cfg, n, flags = _config(RUN_CASE)
    assert n == 2
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags)
        eng.run(0, n)
        eng.fetch()
        for i in range(n):
            _equals_the_oracle(eng, ora, i)
        lo, up = eng.meta(0), eng.meta(1)
        return {"ops": max(len(_ops(ora, i, int(cfg.n_nodes))) for i in range(n)),
                "op_wave_rounds": (lo.n_events >> 16) + (up.reserved[0] & 0xFFFF), "wave_rounds": lo.reserved[0] & 0xFFFF,
                "reads_in_runs": lo.reserved[0] >> 16, "iterations": lo.reserved[2] & 0xFFFF, "broadcasts_in_runs": lo.reserved[2] >> 16,
                "replayed": (lo.reserved[1] & 0xFFFF) + (up.reserved[1] & 0xFFFF), "recorded": lo.reserved[1] >> 24, "dropped": up.reserved[2],
                "outside_quiet": ((lo.reserved[1] >> 16) & 0xFF) + ((up.reserved[1] >> 16) & 0xFF)}


def _bound(c):
    return -(-c["ops"] // 31) + c["recorded"] + c["dropped"] + c["outside_quiet"] + 2


def _self(lib, what, timeout=800, **extra):
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=S._env(lib, **extra), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_a_read_follows_a_remembered_broadcast_inside_one_block():
    """the oracle alone: in the 2-node case some cluster has a read directly behind a broadcast from an origin seen before, both inside one
    block of 32 draws and the broadcast not the block's last draw (what a run takes as two iterations: the read copies the set from HBM)"""
    import oracle_lib as O
    _, cfg, n, _ = _config(TWO_NODES)
    ora = O.run(cfg, 0, n)
    found = []
    for i in range(n):
        ops = _ops(ora, i, int(cfg.n_nodes))
        found += [(i, j) for j in range(1, len(ops)) if ops[j - 1][0] and not ops[j][0] and _taken_by_a_run(ops, j - 1) and (j - 1) // 32 == j // 32]
    assert found, "no read behind a broadcast from a seen origin inside one block: choose another seed"
    # ... and one such pair whose broadcast opens or closes nothing special, and one behind a set-word boundary (value 32 or later)
    assert any(sum(1 for o in _ops(ora, i, int(cfg.n_nodes))[:j] if o[0]) > 32 for i, j in found), found


@pytest.mark.timeout(900)
def test_duo_steady_run_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(900)
def test_duo_steady_run_on_the_emulator_when_count_downs_run_out(emu_lib):
    _compare(_variant("srunw2", ["-DDUO_PAIR_WAIT=2"]), CASES, {})


@pytest.mark.timeout(900)
def test_duo_steady_run_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED, {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_steady_run_on_the_emulator_stopped_by_a_capacity_inside_a_run(emu_lib):
    assert "capacities inside a run: OK" in _self(emu_lib, "capacities")


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("wait", [[], ["-DDUO_PAIR_WAIT=2"]], ids=["wait24", "wait2"])
def test_duo_steady_run_round_limits_are_those_of_the_build_without_it(emu_lib, wait):
    from test_duo_op_plan_hipemu import LIMITS
    tag = "w2" if wait else ""
    new = _variant("srunw2", wait) if wait else emu_lib
    plain = _variant("nosrun" + tag, ["-DDUO_NO_STEADY_RUN"] + wait)
    got = {t: json.loads(_self(lib, "limits", timeout=1500).strip().splitlines()[-1]) for t, lib in (("new", new), ("plain", plain))}
    for sweep, limits in (("one", LIMITS), ("pair", PAIR_LIMITS)):
        a, b = got["new"][sweep], got["plain"][sweep]
        assert sorted(a) == sorted(str(x) for x in limits)
        if sweep == "pair":
            assert all(len(row) == 5 + len(NET) for d in a.values() for row in d)
        diff = [k for k in a if a[k] != b[k]]
        assert not diff, f"{sweep}: the builds with and without the steady run differ at the limits {diff[:10]}: {a[diff[0]]} != {b[diff[0]]}"


@pytest.mark.timeout(900)
def test_duo_steady_run_verify_build_runs_every_case_without_a_trap(emu_lib):
    verify = _variant("memoverify", ["-DDUO_MEMO_VERIFY"])
    _compare(verify, CASES, {})
    _compare(verify, POISONED, {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_op_wave_rounds_end_where_a_run_ends_on_the_emulator(emu_lib):
    old = json.loads(_self(_variant("nosrunprof", PROF_FLAGS + ["-DDUO_NO_STEADY_RUN"]), "counts").strip().splitlines()[-1])
    new = json.loads(_self(_variant("srunprof", PROF_FLAGS), "counts").strip().splitlines()[-1])
    print(old, new)
    assert old["ops"] == new["ops"] and old["broadcasts_in_runs"] == 0
    assert _bound(new) < old["op_wave_rounds"], f"the bound {_bound(new)} says nothing: the build without the steady run takes {old['op_wave_rounds']} op wave-rounds"
    assert new["op_wave_rounds"] <= _bound(new), f"{new['op_wave_rounds']} op wave-rounds, the bound is {_bound(new)}: {new}"
    assert 0 < new["broadcasts_in_runs"] <= new["replayed"] and new["iterations"] <= new["reads_in_runs"] + new["broadcasts_in_runs"], new


if __name__ == "__main__":
    if sys.argv[1:] == ["limits"]:
        print(json.dumps(limit_sweeps()))
    elif sys.argv[1:] == ["counts"]:
        print(json.dumps(run_counts()))
    elif sys.argv[1:] == ["capacities"]:
        capacity_sweeps()
    else:
        raise SystemExit("limits | counts | capacities")
