"""The block plan of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, the steady-run instantiation: latency 0, at most four
neighbours; -DDUO_NO_BLOCK_PLAN compiles it out): in front of the steady run's loop, lane k of a half plans draw k of the block of 32
generator draws (its time, value count, row index and payload offset by prefix sums), tests on it what the loop tests on its op, and the
longest prefix of ops that all pass is committed at once; a planned read WRITES what its node's set must hold (all ones up to a partial
last word) under facts the kernel checks, and a half for which a fact fails takes the loop.  What a cluster computes is what it always
computed, so on the host wavefront emulator (lanes out of lockstep, MSIM_GUARD=3) every unflagged instance equals the oracle bit for
bit: rows, payload, meta (n_rounds included) and the six net-stats counters.

CASES are those of tests/test_duo_flood_memo_hipemu.py (each a handful of clusters at <= 1 s of virtual time): a cutoff inside a block, odd
cluster counts (one live half), halves that drift (the line of 24), halves that are not quiet (rate 2000 / 3000: the plan declines),
MANY_BROADCASTS (two set-word boundaries).  They run again on a -DDUO_PAIR_WAIT=2 build; POISONED run with every device buffer filled
with 0xA5, in a process of their own.

MID-BLOCK ENTRY (the oracle alone): the 2-node case holds a half that enters a block in mid-block, behind a broadcast from an origin not
yet seen, and reads a plan can take at the value counts 31, 32, 33 (63, 64, 65 in MANY_BROADCASTS): the edges of the partial word.

CAPACITIES INSIDE A PLAN (plan_capacity_sweeps): two clusters of the 2-node case with max_rows and max_payload_words moved over every op
of the second block of draws, and max_values 30 to 34 and 62 to 66; flags are the oracle's, every unflagged instance is equal in full.

BUILD AGAINST BUILD: under MSIM_DUO_ROUND_LIMIT the LIMITS and PAIR_LIMITS sweeps, at both pair waits, give what a -DDUO_NO_BLOCK_PLAN
build gives, limit for limit.

THE FALLBACK: a -DDUO_BLOCK_PLAN_NO_FACTS build (every half's sets treated as not uniform) equals the oracle and takes no plan.

THE PATH IS TAKEN (a -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN -DDUO_PROF_PLAN build, two clusters of the headline shape): the ops taken
by plans are at least plan_bound(), computed from the oracle's rows alone; the same build with -DDUO_NO_BLOCK_PLAN reports 0."""
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
from test_duo_flood_memo_hipemu import CASES, MANY_BROADCASTS, POISONED, limit_sweeps  # noqa: E402
from test_duo_steady_run_hipemu import PROF_FLAGS, RUN_CASE, TWO_NODES, _equals_the_oracle, _ops, _taken_by_a_run  # noqa: E402
from test_duo_stretch_hipemu import _compare, _config, _variant, emu_lib  # noqa: E402,F401
from test_duo_trim_hipemu import NET, PAIR_LIMITS  # noqa: E402

PLAN_PROF = PROF_FLAGS + ["-DDUO_PROF_PLAN"]
SWEEP_BLOCK = 1   # the block of draws the swept capacities stop a cluster in: ops 32 to 63


def plan_bound(ops):
    """by the oracle's rows alone: the ops of one cluster that are not a block's last draw and are a read or a broadcast from an origin
    seen before (_taken_by_a_run), less those that stand at or behind the first op of their block that is not such an op"""
    total = 0
    for b in range(0, len(ops), 32):
        for j in range(b, min(b + 32, len(ops))):
            if not _taken_by_a_run(ops, j):
                break
            total += 1
    return total


def plan_counts():
    """RUN_CASE on the -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN -DDUO_PROF_PLAN library MSIM_LIB names, checked against the oracle: the
    wavefront's plan counters (see the epilogue of sim_kernel_duo) and the bound from the oracle's rows"""
    import oracle_lib as O
    E, cfg, n, flags = _config(RUN_CASE)
    assert n == 2
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    ops = [_ops(ora, i, int(cfg.n_nodes)) for i in range(n)]
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags)
        eng.run(0, n)
        eng.fetch()
        for i in range(n):
            _equals_the_oracle(eng, ora, i)
        lo, up = eng.meta(0), eng.meta(1)
        return {"ops": sum(len(o) for o in ops), "bound": sum(plan_bound(o) for o in ops), "plans": up.reserved[2] & 0xFFFF, "plan_ops": up.reserved[2] >> 16,
                "reads_in_runs": lo.reserved[0] >> 16, "broadcasts_in_runs": lo.reserved[2] >> 16, "iterations": lo.reserved[2] & 0xFFFF}


def plan_capacity_sweeps():
    """Two clusters of TWO_NODES on whatever library MSIM_LIB names (the device library by default): max_rows and max_payload_words moved
    over every op of block SWEEP_BLOCK (from the oracle's rows of the uncapped run), max_values 30 to 34 and 62 to 66"""
    import oracle_lib as O
    from maelstrom_amd import engine as E
    kw = ast.literal_eval(TWO_NODES)
    kw["n"] = 2
    flags, seed, n = kw.pop("flags"), kw.pop("seed"), kw.pop("n")
    free = O.run(E.test_config(seed=seed, **kw), 0, n)
    ops = [_ops(free, i, kw["node_count"]) for i in range(n)]
    b0, b1 = 32 * SWEEP_BLOCK, 32 * SWEEP_BLOCK + 32
    for o in ops:   # the block is there in full, and plans take ops of it: most of its ops are such ops
        assert len(o) > b1 + 4 and sum(1 for j in range(b0, b1) if _taken_by_a_run(o, j)) >= 24, o[b0:b1]
    pay = sorted({sum(x[2] for x in o[:j]) for o in ops for j in range(b0, b1 + 1)})
    sweeps = [("max_rows", list(range(2 * b0, 2 * b1 + 1))), ("max_payload_words", pay), ("max_values", list(range(30, 35)) + list(range(62, 67)))]
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
    assert flagged["max_rows"] == len(sweeps[0][1]) * n and flagged["max_payload_words"] > 0 and flagged["max_values"] > 0, flagged
    print("capacities inside a plan: OK", flagged)
    return flagged


def _self(lib, what, timeout=800, **extra):
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=S._env(lib, **extra), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _value_counts_of_plannable_reads(ops):
    """the value counts (broadcasts before it) of the reads of one cluster that a plan can take"""
    out, v = set(), 0
    for j, o in enumerate(ops):
        if o[0]:
            v += 1
        elif _taken_by_a_run(ops, j):
            out.add(v)
    return out


def test_a_half_enters_a_block_in_mid_block_and_reads_stand_at_the_word_edges():
    """the oracle alone (see MID-BLOCK ENTRY above)"""
    import oracle_lib as O
    _, cfg, n, _ = _config(TWO_NODES)
    ora = O.run(cfg, 0, n)
    ops = [_ops(ora, i, int(cfg.n_nodes)) for i in range(n)]
    # (a) a broadcast from an origin not seen before (the quiet body simulates it), not at the end of its block, with an op a plan takes
    #     right behind it in the same block: the half's next op wave-round begins at that op, k0 > 0
    mid = [(i, j) for i, o in enumerate(ops) for j in range(len(o) - 1)
           if o[j][0] and not any(x[0] and x[1] == o[j][1] for x in o[:j]) and j % 32 < 30 and _taken_by_a_run(o, j + 1)]
    assert mid, "no half enters a block in mid-block behind a broadcast from an unseen origin: choose another seed"
    # (b) the partial-word edges
    seen = set().union(*[_value_counts_of_plannable_reads(o) for o in ops])
    assert {31, 32, 33} <= seen, sorted(seen)
    _, cfg, n, _ = _config(MANY_BROADCASTS)
    ora = O.run(cfg, 0, n)
    seen = set().union(*[_value_counts_of_plannable_reads(_ops(ora, i, int(cfg.n_nodes))) for i in range(n)])
    assert {63, 64, 65} <= seen, sorted(seen)


@pytest.mark.timeout(900)
def test_duo_block_plan_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(900)
def test_duo_block_plan_on_the_emulator_when_count_downs_run_out(emu_lib):
    _compare(_variant("bplanw2", ["-DDUO_PAIR_WAIT=2"]), CASES, {})


@pytest.mark.timeout(900)
def test_duo_block_plan_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED, {"MSIM_POISON": "0xA5"})
    _compare(_variant("bplanw2", ["-DDUO_PAIR_WAIT=2"]), POISONED, {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(1800)
def test_duo_block_plan_on_the_emulator_stopped_by_a_capacity_inside_a_plan(emu_lib):
    assert "capacities inside a plan: OK" in _self(emu_lib, "capacities", timeout=1500)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("wait", [[], ["-DDUO_PAIR_WAIT=2"]], ids=["wait24", "wait2"])
def test_duo_block_plan_round_limits_are_those_of_the_build_without_it(emu_lib, wait):
    from test_duo_op_plan_hipemu import LIMITS
    tag = "w2" if wait else ""
    new = _variant("bplanw2", wait) if wait else emu_lib
    plain = _variant("nobplan" + tag, ["-DDUO_NO_BLOCK_PLAN"] + wait)
    got = {t: json.loads(_self(lib, "limits", timeout=1500).strip().splitlines()[-1]) for t, lib in (("new", new), ("plain", plain))}
    for sweep, limits in (("one", LIMITS), ("pair", PAIR_LIMITS)):
        a, b = got["new"][sweep], got["plain"][sweep]
        assert sorted(a) == sorted(str(x) for x in limits)
        if sweep == "pair":
            assert all(len(row) == 5 + len(NET) for d in a.values() for row in d)
        diff = [k for k in a if a[k] != b[k]]
        assert not diff, f"{sweep}: the builds with and without the block plan differ at the limits {diff[:10]}: {a[diff[0]]} != {b[diff[0]]}"


@pytest.mark.timeout(900)
def test_duo_block_plan_without_its_facts_takes_the_loop_and_equals_the_oracle(emu_lib):
    _compare(_variant("bplannofacts", ["-DDUO_BLOCK_PLAN_NO_FACTS"]), CASES, {})
    c = json.loads(_self(_variant("bplannofactsprof", PLAN_PROF + ["-DDUO_BLOCK_PLAN_NO_FACTS"]), "counts").strip().splitlines()[-1])
    print(c)
    assert c["plans"] == 0 and c["plan_ops"] == 0 and c["broadcasts_in_runs"] > 0, c


@pytest.mark.timeout(900)
def test_duo_steady_ops_are_taken_by_block_plans_on_the_emulator(emu_lib):
    old = json.loads(_self(_variant("nobplanprof", PLAN_PROF + ["-DDUO_NO_BLOCK_PLAN"]), "counts").strip().splitlines()[-1])
    new = json.loads(_self(_variant("bplanprof", PLAN_PROF), "counts").strip().splitlines()[-1])
    print(old, new)
    assert old["plans"] == 0 and old["plan_ops"] == 0, old   # the bound says something: the build without the plan does not meet it
    assert old["ops"] == new["ops"] and old["bound"] == new["bound"] and new["bound"] > new["ops"] // 2, new
    assert new["plan_ops"] >= new["bound"], f"{new['plan_ops']} ops taken by plans, the bound is {new['bound']}: {new}"
    assert 0 < new["plans"] <= new["plan_ops"] <= new["reads_in_runs"] + new["broadcasts_in_runs"], new
    # what the loop still took: an iteration of it takes at least one op
    assert new["iterations"] <= new["reads_in_runs"] + new["broadcasts_in_runs"] - new["plan_ops"], new


if __name__ == "__main__":
    if sys.argv[1:] == ["limits"]:
        print(json.dumps(limit_sweeps()))
    elif sys.argv[1:] == ["counts"]:
        print(json.dumps(plan_counts()))
    elif sys.argv[1:] == ["capacities"]:
        plan_capacity_sweeps()
    else:
        raise SystemExit("limits | counts | capacities")
