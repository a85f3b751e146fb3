"""The flood table of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, "FLOOD TABLE"; the memo instantiation: latency 0, at
most four neighbours; -DDUO_NO_FLOOD_TABLE compiles it out): what the flood of a broadcast does to a cluster is a function of the
topology, the fan-out rule and the picked node alone, so the memo tables that every wavefront of every launch used to fill for itself
are one table.  One wavefront makes it before a context's first launch (two clusters of the context's configuration on slabs of their
own, the kernel's own recording path), every later wavefront starts from a copy of it, and an origin the table lacks is recorded by the
wavefront that meets it, as before.  What a cluster computes is what it always computed: on the host wavefront emulator (lanes out of
lockstep, MSIM_GUARD=3, which fences the table and the table wavefront's slabs like every slab) every case equals the oracle bit for
bit: rows, payload, meta with n_rounds, the six net-stats counters.

THE MEMO CASES: CASES of tests/test_duo_flood_memo_hipemu.py, again at -DDUO_PAIR_WAIT=2, and on the -DDUO_MEMO_VERIFY build, which
takes the table, simulates every flood the table remembers all the same and traps where it differs from the record.
A FULL TABLE (FULL_CASE: 5 nodes, rate 100, 1 s, 4 clusters, none of which ends on a broadcast), on a profile build that takes the table (-DDUO_PROF -DDUO_PROF_MEMO
-DDUO_PROF_RUN -DDUO_PROF_TABLE: the op wave-round bound below is the steady run's, which a -DDUO_PROF build has with -DDUO_PROF_RUN
alone): the table names all 5 origins, no wavefront records or drops anything, every cluster replays at least its broadcasts less those
taken outside the quiet body, and a wavefront's op wave-rounds stay within ceil(ops of its busier cluster / 31) + its broadcasts outside
the quiet body + 2: the bound of tests/test_duo_steady_run_hipemu.py with its two recording terms gone.
A PARTIAL TABLE (PARTIAL_CASE: the 25-node grid, 0.2 s, 5 clusters): the table wavefront's two clusters broadcast from fewer than 25
origins, so some replays come from the table and some from a wavefront's own recording, and the lone fifth cluster, which could never
record, replays.  AN EMPTY TABLE (FEW_OPS): every output byte is that of the -DDUO_NO_FLOOD_TABLE build.
THE TABLE'S INSTANCES DO NOT MATTER: one case under two values of MSIM_DUO_TABLE_FIRST gives the same bytes.  ONE TABLE PER CONTEXT: one
engine, three runs with other first instances and sizes (4, 1, 7: the slabs are regrown), makes one table; two engines with other
topologies make one each.  LAUNCH PATHS: three contexts in flight (run_async + check, 6 clusters each); poisoned slabs (MSIM_POISON fills
the context's slabs before every launch and the table wavefront's own, never the table).  CAPACITIES: the sweeps of
tests/test_duo_block_plan_hipemu.py against the oracle (flags equal, every unflagged instance in full).  ROUND LIMITS: the one-cluster
and the pair sweep under MSIM_DUO_ROUND_LIMIT, build against build with -DDUO_NO_FLOOD_TABLE, at both waits: every instance's flags are
equal and every unflagged instance is equal in full, with the table read under the limits (MSIM_DUO_TABLE_UNDER_LIMIT=1) and, as a
launch under a limit runs by default, without it (test_duo_flood_table_round_limits says why, and prints where stopped instances differ)."""
import ast
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_duo_stretch_hipemu as S  # noqa: E402
from test_duo_flood_memo_hipemu import ADDED, CASES, FEW_OPS, MSIM_F_BROADCAST, POISONED, limit_sweeps  # noqa: E402,F401
from test_duo_steady_run_hipemu import PROF_FLAGS, _equals_the_oracle, _ops  # noqa: E402
from test_duo_stretch_hipemu import _compare, _config, _variant, emu_lib  # noqa: E402,F401
from test_duo_trim_hipemu import NET  # noqa: E402

# (seed 71: by the oracle's rows the last op every one of the four generators makes is a read.  A cluster's LAST generated op is never
#  replayed: gen_next < cutoff is a condition of the replay, since the half's own scheduler acts next, and by the oracle alone the case
#  is one in which that op is no broadcast, so that "every broadcast inside the quiet body is replayed" can be asked without a term for it)
FULL_CASE = "{'workload':'broadcast','node_count':5,'rate':100,'time_limit':1,'n':4,'inbox_capacity':6,'seed':71,'flags':0x400}"
PARTIAL_CASE = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':0.2,'n':5,'inbox_capacity':6,'seed':2026,'flags':0x400}"
FIRST_CASE = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':1,'n':5,'inbox_capacity':6,'seed':2027,'flags':0x400}"
IN_FLIGHT = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':1,'n':6,'inbox_capacity':6,'seed':%d,'flags':0x400}"
LINE5 = "{'workload':'broadcast','node_count':5,'rate':100,'time_limit':1,'topology':'line','n':4,'inbox_capacity':6,'seed':65,'flags':0x400}"
TABLE_PROF = PROF_FLAGS + ["-DDUO_PROF_TABLE"]
TRACE = re.compile(r"\[duo\] flood table: (\d+) of (\d+) origins")
assert ast.literal_eval(FULL_CASE)["node_count"] == 5 and ast.literal_eval(FULL_CASE)["n"] == 4


def table_counts(case):
    """`case` on the -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN -DDUO_PROF_TABLE library MSIM_LIB names, checked against the oracle: per
    cluster its ops and broadcasts (the oracle's rows), the floods it replayed and the broadcasts it took outside the quiet body; per
    wavefront its op wave-rounds and the floods it recorded itself (see the epilogue of sim_kernel_duo; a lone cluster's wavefront has no
    upper instance: its flood op rounds are not carried)"""
    import oracle_lib as O
    E, cfg, n, flags = _config(case)
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags | 0x1000)
        eng.run(0, n)
        eng.fetch()
        out = {"nodes": int(cfg.n_nodes), "clusters": [], "wavefronts": []}
        for i in range(n):
            _equals_the_oracle(eng, ora, i)
            ops, m = _ops(ora, i, int(cfg.n_nodes)), eng.meta(i)
            out["clusters"].append({"ops": len(ops), "broadcasts": sum(1 for o in ops if o[0]), "origins": len({o[1] for o in ops if o[0]}),
                                    "replayed": m.reserved[1] & 0xFFFF, "outside_quiet": (m.reserved[1] >> 16) & 0xFF, "recorded_by_wavefront": m.reserved[1] >> 24})
        for w in range(0, n - 1, 2):
            lo, up = eng.meta(w), eng.meta(w + 1)
            out["wavefronts"].append({"op_wave_rounds": (lo.n_events >> 16) + (up.reserved[0] & 0xFFFF), "recorded": lo.reserved[1] >> 24})
        return out


def digests(case, first=0, n=None):
    """every output byte of `case` on the library MSIM_LIB names, per instance: meta, the digest of rows and payload, the net stats"""
    E, cfg, n0, flags = _config(case)
    n = n or n0
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags | 0x1000)
        eng.run(first, n)
        eng.fetch()
        out = []
        for i in range(n):
            rows, pay = eng.raw_history(i)
            m, st = eng.meta(i), eng.net_stats_raw(i)
            out.append([m.n_rows, m.n_payload_words, m.flags, m.n_rounds, hashlib.sha256(rows.tobytes() + pay.tobytes()).hexdigest()] + [int(getattr(st, f)) for f in NET])
        return out


def _against_the_oracle(eng, cfg, first, n):
    import oracle_lib as O
    ora = O.run(cfg, first, n)
    eng.fetch()
    for i in range(n):
        assert int(ora.meta[i]["flags"]) == 0 and eng.meta(i).flags == 0
        _equals_the_oracle(eng, ora, i)


def one_engine_three_runs():
    """one context, three launches with other first instances and sizes (the slabs are regrown for the third): each equals the oracle"""
    E, cfg, _, flags = _config(FIRST_CASE)
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags | 0x1000)
        for first, n in ((0, 4), (100, 1), (7, 7)):
            eng.run(first, n)
            _against_the_oracle(eng, cfg, first, n)
    print("one engine: OK")


def two_engines():
    """two contexts with other topologies in one process, launched in turn: each equals the oracle (each from its own table)"""
    E, cfg_a, n_a, flags = _config(FULL_CASE)
    _, cfg_b, n_b, _ = _config(LINE5)
    with E.Engine(cfg_a) as a, E.Engine(cfg_b) as b:
        for eng in (a, b):
            eng.set_dev_flags(flags | 0x1000)
        for _ in range(2):
            a.run(0, n_a)
            b.run(0, n_b)
            _against_the_oracle(a, cfg_a, 0, n_a)
            _against_the_oracle(b, cfg_b, 0, n_b)
    print("two engines: OK")


def three_in_flight(streams=(None, None, None)):
    """three contexts in flight, run_async + check, 6 clusters each, two rounds of launches: every batch equals the oracle and is valid"""
    E = None
    cfgs = []
    for k in range(3):
        E, cfg, n, flags = _config(IN_FLIGHT % (70 + k))
        cfgs.append(cfg)
    engs = [E.Engine(c) for c in cfgs]
    try:
        for e in engs:
            e.set_dev_flags(flags | 0x1000)
        for rnd in range(2):
            for e, st in zip(engs, streams):
                e.run_async(rnd * n, n, st)
            for e, c in zip(engs, cfgs):
                e.check()
                assert all(bool(r["valid"]) for r in e.check_results())
                _against_the_oracle(e, c, rnd * n, n)
    finally:
        for e in engs:
            e.close()
    print("in flight: OK")


def _child(lib, what, timeout=800, **extra):
    """this file as a script on `lib` (None: the library the environment names), in a process of its own: (stdout, stderr)"""
    env = S._env(lib, **extra) if lib else dict(os.environ, **extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + what, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, " ".join(what) + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout, r.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def check_full_table(lib):
    out, err = _child(lib, ["counts", FULL_CASE])
    c = _last_json(out)
    print(c, TRACE.findall(err))
    assert TRACE.findall(err) == [("5", "5")], err[-2000:]
    for cl in c["clusters"]:
        assert cl["recorded_by_wavefront"] == 0, c
        assert cl["broadcasts"] > 2 * c["nodes"] and cl["origins"] == c["nodes"], c   # (the case has the ops for it)
        assert cl["replayed"] >= cl["broadcasts"] - cl["outside_quiet"], c
    for w, wf in enumerate(c["wavefronts"]):
        pair = c["clusters"][2 * w:2 * w + 2]
        assert wf["op_wave_rounds"] <= -(-max(p["ops"] for p in pair) // 31) + sum(p["outside_quiet"] for p in pair) + 2, (w, c)


def check_partial_table(lib):
    out, err = _child(lib, ["counts", PARTIAL_CASE])
    c = _last_json(out)
    print(c, TRACE.findall(err))
    (known, nodes), = TRACE.findall(err)
    assert 0 < int(known) < int(nodes) == 25, err[-2000:]
    own = sum(w["recorded"] for w in c["wavefronts"])
    assert own > 0, c   # some replays come from a wavefront's own recording ...
    # ... and some from the table: the first wavefront runs the very clusters that made the table (instances 0 and 1), so it ends no recording
    # of its own (what the table wavefront recorded it finds there, what that one dropped it drops), and yet it replays
    assert c["wavefronts"][0]["recorded"] == 0 and c["clusters"][0]["replayed"] + c["clusters"][1]["replayed"] > 0, c
    assert c["clusters"][4]["replayed"] > 0, c   # the lone fifth cluster cannot record: what it replays it has from the table


def check_round_limits(table, plain, **table_env):
    """the two sweeps on both builds (`table_env`: the environment of the first): flags equal, unflagged instances equal in full; returns
    the limits at which flagged instances differ"""
    from test_duo_op_plan_hipemu import LIMITS
    from test_duo_trim_hipemu import PAIR_LIMITS
    got = {"table": _last_json(_child(table, ["limits"], timeout=1500, **table_env)[0]), "plain": _last_json(_child(plain, ["limits"], timeout=1500)[0])}
    differ = {}
    for sweep, limits in (("one", LIMITS), ("pair", PAIR_LIMITS)):
        a, b = got["table"][sweep], got["plain"][sweep]
        assert sorted(a) == sorted(str(x) for x in limits) == sorted(b)
        for k in a:
            assert [r[2] for r in a[k]] == [r[2] for r in b[k]], f"{sweep}: flags differ at the limit {k}: {a[k]} != {b[k]}"
            for ra, rb in zip(a[k], b[k]):
                assert ra[2] != 0 or ra == rb, f"{sweep}: an unflagged instance differs at the limit {k}: {ra} != {rb}"
        differ[sweep] = sorted(int(k) for k in a if a[k] != b[k])
    return differ


def test_the_cases_have_the_ops_for_it():
    """the oracle alone: no instance of the added cases is flagged; FULL_CASE's clusters broadcast from all 5 origins, more than 10 times;
    the first two clusters of PARTIAL_CASE (instances 0 and 1: the table wavefront's by default) broadcast from fewer than 25 origins, and
    its later clusters from origins those two lack"""
    import oracle_lib as O
    for case in (FULL_CASE, PARTIAL_CASE, FIRST_CASE, LINE5, IN_FLIGHT % 70):
        _, cfg, n, _ = _config(case)
        assert ast.literal_eval(case)["time_limit"] <= 1
        ora = O.run(cfg, 0, n)
        assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n, case
        org = [{o[1] for o in _ops(ora, i, int(cfg.n_nodes)) if o[0]} for i in range(n)]
        if case == FULL_CASE:
            assert all(len(s) == 5 for s in org) and all(sum(1 for o in _ops(ora, i, 5) if o[0]) > 10 for i in range(n))
            assert not any(_ops(ora, i, 5)[-1][0] for i in range(n))   # (no generator ends on a broadcast, see FULL_CASE)
        if case == PARTIAL_CASE:
            assert len(org[0] | org[1]) < 25 and any(s - (org[0] | org[1]) for s in org[2:]) and org[4] & (org[0] | org[1])


@pytest.mark.timeout(900)
def test_duo_flood_table_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES + [PARTIAL_CASE, FIRST_CASE, LINE5], {})


@pytest.mark.timeout(900)
def test_duo_flood_table_on_the_emulator_when_count_downs_run_out(emu_lib):
    _compare(_variant("memow2", ["-DDUO_PAIR_WAIT=2"]), CASES + [PARTIAL_CASE], {})


@pytest.mark.timeout(900)
def test_duo_flood_table_verify_build_simulates_every_flood_of_the_table_without_a_trap(emu_lib):
    _compare(_variant("memoverify", ["-DDUO_MEMO_VERIFY"]), CASES + [PARTIAL_CASE, LINE5], {})


@pytest.mark.timeout(900)
def test_duo_flood_table_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED + [PARTIAL_CASE], {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_full_flood_table_leaves_nothing_to_record_on_the_emulator(emu_lib):
    check_full_table(_variant("tableprof", TABLE_PROF))


@pytest.mark.timeout(900)
def test_duo_partial_flood_table_is_completed_by_the_wavefronts_on_the_emulator(emu_lib):
    check_partial_table(_variant("tableprof", TABLE_PROF))


@pytest.mark.timeout(900)
def test_duo_empty_flood_table_gives_the_bytes_of_the_build_without_it(emu_lib):
    plain = _variant("notable", ["-DDUO_NO_FLOOD_TABLE"])
    out, err = _child(emu_lib, ["digests", FEW_OPS])
    assert TRACE.findall(err) == [("0", "25")], err[-2000:]
    out_p, err_p = _child(plain, ["digests", FEW_OPS])
    assert not TRACE.findall(err_p) and _last_json(out) == _last_json(out_p)


@pytest.mark.timeout(900)
def test_duo_flood_table_does_not_depend_on_the_instances_that_made_it(emu_lib):
    got = [_last_json(_child(emu_lib, ["digests", FIRST_CASE], MSIM_DUO_TABLE_FIRST=first)[0]) for first in ("0", "1000001")]
    assert got[0] == got[1]


@pytest.mark.timeout(900)
def test_duo_flood_table_is_made_once_per_context_on_the_emulator(emu_lib):
    out, err = _child(emu_lib, ["one_engine"])
    assert "one engine: OK" in out and len(TRACE.findall(err)) == 1 and err.count("[layout] duo") == 3, err[-2000:]
    out, err = _child(emu_lib, ["two_engines"])
    assert "two engines: OK" in out and len(TRACE.findall(err)) == 2 and err.count("[layout] duo") == 4, err[-2000:]


@pytest.mark.timeout(900)
def test_duo_flood_table_with_three_contexts_in_flight_on_the_emulator(emu_lib):
    out, err = _child(emu_lib, ["in_flight"])
    assert "in flight: OK" in out and len(TRACE.findall(err)) == 3, err[-2000:]


@pytest.mark.timeout(900)
def test_duo_flood_table_on_the_emulator_stopped_by_a_capacity(emu_lib):
    out, _ = _child(emu_lib, ["capacities"])
    assert "capacities inside a plan: OK" in out


@pytest.mark.timeout(3000)
@pytest.mark.parametrize("wait", [[], ["-DDUO_PAIR_WAIT=2"]], ids=["wait24", "wait2"])
def test_duo_flood_table_round_limits(emu_lib, wait):
    """A launch under MSIM_DUO_ROUND_LIMIT starts from empty tables unless MSIM_DUO_TABLE_UNDER_LIMIT=1 is given (msim_launch_duo).
    WITH THE TABLE READ (that switch), both sweeps against the -DDUO_NO_FLOOD_TABLE build: every instance's flags are equal and every
    unflagged instance is equal in full (check_round_limits), so a replay from the table's record near a limit changes no result; the
    one-cluster sweep, where a lone cluster now replays from its first op, is equal in full, stopped instances included: there is no
    partner, and the replay's own precondition (rounds + the record + the leaving round below the limit) keeps the limit where it was.
    In the pair sweep an instance the limit stops may be stopped elsewhere: a half's limit is looked at where R0's block is entered, and
    when that happens follows the alignment of the two halves' rounds ("Not built": a replaying half's dry point
    comes at once); a half that replays its first floods from the table is aligned with its partner otherwise than one that records
    them.  The limits at which stopped instances differ are printed: measured, none at the default wait, 37 of the 121 at
    -DDUO_PAIR_WAIT=2, all from 119 on (at 119 the upper cluster is stopped at round 123 instead of 120, one op further on).
    WITHOUT THE SWITCH no launch under a limit reads a table, and both sweeps give the other build's bytes limit for limit, stopped
    instances included: what the sweeps of tests/test_duo_flood_memo_hipemu.py, which hold this build against -DDUO_NO_MEMO, need."""
    tag = "w2" if wait else ""
    table = _variant("memow2", wait) if wait else emu_lib
    plain = _variant("notable" + tag, ["-DDUO_NO_FLOOD_TABLE"] + wait)
    differ = check_round_limits(table, plain, MSIM_DUO_TABLE_UNDER_LIMIT="1")
    print("with the table read under the limits, stopped instances differ at the limits:", differ)
    assert differ["one"] == [], differ
    assert check_round_limits(table, plain) == {"one": [], "pair": []}


if __name__ == "__main__":
    what = sys.argv[1:]
    if what[:1] == ["counts"]:
        print(json.dumps(table_counts(what[1])))
    elif what[:1] == ["digests"]:
        print(json.dumps(digests(what[1])))
    elif what == ["limits"]:
        print(json.dumps(limit_sweeps()))
    elif what == ["one_engine"]:
        one_engine_three_runs()
    elif what == ["two_engines"]:
        two_engines()
    elif what == ["in_flight"]:
        three_in_flight()
    elif what == ["capacities"]:
        from test_duo_block_plan_hipemu import plan_capacity_sweeps
        plan_capacity_sweeps()
    else:
        raise SystemExit("unknown: " + " ".join(what))
