"""The flood memo of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, the steady instantiation: latency 0, at most four
neighbours; -DDUO_NO_MEMO compiles it out): a wavefront simulates the flood of a broadcast once per origin, records per lane what that
simulation did (the rise of n_arr, the value's bit in the set word, the rise of rounds), and a later broadcast from that origin by a
steady half applies the record in the quiet op round instead of simulating the flood again; two halves that leave an op round with
nothing in flight go straight to their next op round (the direct way on).  What a cluster computes is what it always computed, so on the
host wavefront emulator (lanes out of lockstep, MSIM_GUARD=3) every unflagged instance equals the oracle bit for bit: rows, payload, meta
(n_rounds included) and the six net-stats counters.

CASES, each a few clusters at a time limit of at most 1 s of virtual time: the shapes of tests/test_duo_quiet_op_hipemu.py at that length
(the 25-node grid with 2, 4 and 7 clusters: some origins repeat, some are seen once, the odd count leaves a wavefront with one live
cluster; 31 nodes: the highest bit of the origin mask and the last row of the table; `tree3`: all four neighbour slots; the line of 24:
floods of very different length, so that one half replays while its partner simulates and is parked; two nodes at rate 50; echo-back with a ring of
8: the fan-out that skips nobody; rate 2000 / 3000: ops that meet a half that is not quiet, GENERAL bodies in mid-run; rate 400: several
blocks of 32 draws; FEW_VALUES: the max_values stop; the partial grid of 7) and ADDED: 2, 4 and 5 nodes at rate 100, where every origin
repeats many times within the second and a cluster makes more than 32 broadcasts (with two nodes a flood lasts a round or two, so replays,
steady leaves and the direct way on follow each other most closely, and replays cross a set-word boundary); rate 200, more than 64 broadcasts per cluster, so that
replays cross two set-word boundaries (val & 31 == 0); FEW_OPS, five ops per cluster: every flood is a first one, and a cluster whose
generator has ended forces GENERAL bodies on a partner that is still recording: the profile build counts recordings DROPPED there, and none
that ended (test_duo_recordings_are_dropped_when_a_cluster_ends_beside_a_recording_partner).  No instance of any of them is flagged by the oracle (test_no_case_is_flagged).  All of them run again on
a -DDUO_PAIR_WAIT=2 build, where a replaying half goes on alone after two rounds, and on a -DDUO_MEMO_VERIFY build, which simulates
every remembered flood all the same and traps if the rise of n_arr in any lane, the rise of rounds or the end state (in_n, deliver_at,
sw) is not the record's.  POISONED run with every device buffer filled with 0xA5, in a process of their own; the three capacity stops
are compared by their flags, as everywhere in this project.

BUILD AGAINST BUILD.  An unflagged instance never stops inside a flood, so the oracle cannot see whether a replay moves the place where
the round limit is found.  Under MSIM_DUO_ROUND_LIMIT the one-cluster sweep of tests/test_duo_op_plan_hipemu.py (LIMITS) and two
clusters of the headline shape under PAIR_LIMITS, limits that fall before, inside and just behind floods that are replayed when the
limit is far, must give, limit for limit, what a -DDUO_NO_MEMO build gives (which compiles to the previous kernel): rows, payload, meta
and all six net-stats counters.  The same with -DDUO_PAIR_WAIT=2 on both sides.  The one-cluster sweep can only show that the memo is
inert there: a recording ends in the steady leave, which wants both halves alive, so a wavefront with one live cluster never remembers a
flood.  The pair sweep is the one that replays: the profile build, run under the highest of PAIR_LIMITS, must have replayed floods in both
clusters before the limit stopped them (with floods replayed below the highest limit, the lower limits fall before, inside and behind them).

THE PATH IS TAKEN (a -DDUO_PROF -DDUO_PROF_MEMO emulator build, two clusters of the headline shape): the wavefront records at most N
floods, and each cluster replays at least its broadcasts less N less the broadcasts taken outside the quiet body.  A condition, not a
tolerance: a quiet broadcast that is not replayed has an origin the wavefront does not remember yet."""
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
from test_duo_quiet_op_hipemu import GPU_CASES as QUIET_SHORT, GPU_POISONED  # noqa: E402
from test_duo_stretch_hipemu import HEADLINE, _compare, _config, _variant, check_stops, emu_lib  # noqa: E402,F401
from test_duo_trim_hipemu import NET, PAIR_LIMITS, pair_limit_sweep  # noqa: E402

_NODES = "{'workload':'broadcast','node_count':%d,'rate':100,'time_limit':1,'n':4,'inbox_capacity':6,'seed':%d,'flags':0x400}"
MANY_BROADCASTS = "{'workload':'broadcast','node_count':25,'rate':200,'time_limit':1,'n':3,'inbox_capacity':6,'seed':62,'flags':0x400}"
FEW_OPS = "{'workload':'broadcast','node_count':25,'rate':5,'time_limit':1,'n':4,'inbox_capacity':6,'seed':63,'flags':0x400}"
ADDED = [_NODES % (2, 64), _NODES % (4, 60), _NODES % (5, 61), MANY_BROADCASTS, FEW_OPS]
CASES = QUIET_SHORT + ADDED
POISONED = GPU_POISONED
MEMO_CASE = HEADLINE % 2
MSIM_F_BROADCAST = 1


def memo_counts(case=None, limit=None):
    """`case` (MEMO_CASE by default; an even number of clusters) on the -DDUO_PROF -DDUO_PROF_MEMO library MSIM_LIB names: per cluster its
    broadcasts (from its rows), the floods it replayed and the broadcasts it took outside the quiet body, and per wavefront the floods it
    recorded and the recordings it dropped (see the epilogue of sim_kernel_duo).  Without a limit the run is checked against the oracle;
    with one it runs under MSIM_DUO_ROUND_LIMIT and every cluster must have been stopped by it."""
    import numpy as np
    import oracle_lib as O
    E, cfg, n, flags = _config(case or MEMO_CASE)
    assert n % 2 == 0
    ora = O.run(cfg, 0, n)
    assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n
    if limit is not None:
        os.environ["MSIM_DUO_ROUND_LIMIT"] = str(limit)
    try:
        with E.Engine(cfg) as eng:
            eng.set_dev_flags(flags)
            eng.run(0, n)
            eng.fetch()
            out = {"nodes": int(cfg.n_nodes), "clusters": []}
            for i in range(n):
                m = eng.meta(i)
                if limit is None:
                    assert (m.n_rows, m.n_rounds, m.flags) == (ora.meta[i]["n_rows"], ora.meta[i]["n_rounds"], 0)
                else:
                    assert m.flags == 16 and m.n_rounds <= limit + 64, (m.flags, m.n_rounds)   # MSIM_FLAG_ROUND_LIMIT
                rows, _ = eng.raw_history(i)
                r = np.frombuffer(rows.tobytes(), dtype=np.uint32).reshape(-1, 4)
                inv = r[(r[:, 2] & 3) == 0]   # MSIM_T_INVOKE
                out["clusters"].append({"broadcasts": int((((inv[:, 2] >> 2) & 0x1FF) == MSIM_F_BROADCAST).sum()), "replayed": m.reserved[1] & 0xFFFF,
                                        "outside_quiet": (m.reserved[1] >> 16) & 0xFF, "recorded_by_wavefront": m.reserved[1] >> 24,
                                        "dropped_by_wavefront": eng.meta(i | 1).reserved[2]})
            return out
    finally:
        os.environ.pop("MSIM_DUO_ROUND_LIMIT", None)


def limit_sweeps():
    from test_duo_op_plan_hipemu import limit_sweep
    return {"one": limit_sweep()[0], "pair": pair_limit_sweep()}


def test_no_case_is_flagged():
    """the oracle alone: no instance of the cases carries a flag, and MANY_BROADCASTS makes more than 64 broadcasts per cluster"""
    import oracle_lib as O
    for case in CASES + POISONED:
        _, cfg, n, _ = _config(case)
        assert ast.literal_eval(case)["time_limit"] <= 1
        ora = O.run(cfg, 0, n)
        assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n, case
        if case in (MANY_BROADCASTS, ADDED[0], ADDED[1], ADDED[2]):
            least = 64 if case == MANY_BROADCASTS else 32
            assert all(int(ora.meta[i]["n_rows"]) - 2 * _reads(ora, i) > 2 * least for i in range(n)), case


def _reads(ora, i):
    import numpy as np
    rows, _ = ora.history(i)
    r = np.frombuffer(rows.tobytes(), dtype=np.uint32).reshape(-1, 4)
    return int(((r[:, 2] & 3) == 0).sum() - ((((r[:, 2] >> 2) & 0x1FF) == MSIM_F_BROADCAST) & ((r[:, 2] & 3) == 0)).sum())


def _self(lib, what, timeout=800, **extra):
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=S._env(lib, **extra), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def verify_lib(emu_lib):
    return _variant("memoverify", ["-DDUO_MEMO_VERIFY"])


@pytest.mark.timeout(900)
def test_duo_flood_memo_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(900)
def test_duo_flood_memo_on_the_emulator_when_count_downs_run_out(emu_lib):
    _compare(_variant("memow2", ["-DDUO_PAIR_WAIT=2"]), CASES, {})


@pytest.mark.timeout(900)
def test_duo_flood_memo_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED, {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_flood_memo_on_the_emulator_stopped_by_a_capacity(emu_lib):
    assert "stops: OK" in _self(emu_lib, "stops")


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("wait", [[], ["-DDUO_PAIR_WAIT=2"]], ids=["wait24", "wait2"])
def test_duo_flood_memo_round_limits_are_those_of_the_build_without_it(emu_lib, wait):
    from test_duo_op_plan_hipemu import LIMITS
    tag = "w2" if wait else ""
    memo = _variant("memow2", wait) if wait else emu_lib
    plain = _variant("nomemo" + tag, ["-DDUO_NO_MEMO"] + wait)
    got = {t: json.loads(_self(lib, "limits", timeout=1500).strip().splitlines()[-1]) for t, lib in (("memo", memo), ("plain", plain))}
    for sweep, limits in (("one", LIMITS), ("pair", PAIR_LIMITS)):
        a, b = got["memo"][sweep], got["plain"][sweep]
        assert sorted(a) == sorted(str(x) for x in limits)
        if sweep == "pair":
            assert all(len(row) == 5 + len(NET) for d in a.values() for row in d)
        diff = [k for k in a if a[k] != b[k]]
        assert not diff, f"{sweep}: the builds with and without the flood memo differ at the limits {diff[:10]}: {a[diff[0]]} != {b[diff[0]]}"
    # the pair sweep does stop clusters with envelopes in flight: servers_recv < servers_send somewhere
    assert any(row[-1] < row[-2] for d in got["memo"]["pair"].values() for row in d)


@pytest.mark.timeout(900)
def test_duo_flood_memo_verify_build_runs_every_case_without_a_trap(verify_lib):
    _compare(verify_lib, CASES, {})
    _compare(verify_lib, POISONED, {"MSIM_POISON": "0xA5"})
    assert "stops: OK" in _self(verify_lib, "stops")


@pytest.mark.timeout(900)
def test_duo_flood_memo_verify_build_when_count_downs_run_out(emu_lib):
    _compare(_variant("memoverifyw2", ["-DDUO_MEMO_VERIFY", "-DDUO_PAIR_WAIT=2"]), CASES, {})


@pytest.mark.timeout(1800)
def test_duo_flood_memo_verify_build_under_round_limits(verify_lib):
    """the sweeps of the build-against-build test on the verifying build: no remembered flood that a limit cuts short differs from its record"""
    from test_duo_op_plan_hipemu import LIMITS
    got = json.loads(_self(verify_lib, "limits", timeout=1500).strip().splitlines()[-1])
    assert sorted(got["one"]) == sorted(str(x) for x in LIMITS) and sorted(got["pair"]) == sorted(str(x) for x in PAIR_LIMITS)


@pytest.mark.timeout(900)
def test_duo_floods_are_recorded_once_and_replayed_on_the_emulator(emu_lib):
    prof = _variant("memoprof", ["-DDUO_PROF", "-DDUO_PROF_MEMO"])
    c = json.loads(_self(prof, "memo").strip().splitlines()[-1])
    print(c)
    n = c["nodes"]
    assert c["clusters"][0]["recorded_by_wavefront"] == c["clusters"][1]["recorded_by_wavefront"] <= n, c
    assert c["clusters"][0]["recorded_by_wavefront"] > 0, c
    for cl in c["clusters"]:
        assert cl["broadcasts"] > 2 * n, c   # (else the condition below holds with nothing replayed)
        assert cl["replayed"] >= cl["broadcasts"] - n - cl["outside_quiet"], c


@pytest.mark.timeout(900)
def test_duo_floods_are_replayed_below_the_swept_pair_limits(emu_lib):
    """the pair sweep of the build-against-build test is not vacuous: under its highest limit both clusters have replayed floods"""
    prof = _variant("memoprof", ["-DDUO_PROF", "-DDUO_PROF_MEMO"])
    c = json.loads(_self(prof, "memo_under_the_highest_pair_limit").strip().splitlines()[-1])
    print(c)
    assert len(c["clusters"]) == 2 and all(cl["replayed"] > 0 for cl in c["clusters"]), c
    assert c["clusters"][0]["recorded_by_wavefront"] > 0, c


@pytest.mark.timeout(900)
def test_duo_recordings_are_dropped_when_a_cluster_ends_beside_a_recording_partner(emu_lib):
    """FEW_OPS on the profile build (checked against the oracle in memo_counts): recordings begin and are dropped, in every wavefront"""
    prof = _variant("memoprof", ["-DDUO_PROF", "-DDUO_PROF_MEMO"])
    c = json.loads(_self(prof, "memo_few_ops").strip().splitlines()[-1])
    print(c)
    assert len(c["clusters"]) == 4 and all(cl["dropped_by_wavefront"] > 0 for cl in c["clusters"]), c
    assert all(cl["replayed"] <= cl["broadcasts"] for cl in c["clusters"]), c


if __name__ == "__main__":
    if sys.argv[1:] == ["limits"]:
        print(json.dumps(limit_sweeps()))
    elif sys.argv[1:] == ["memo"]:
        print(json.dumps(memo_counts()))
    elif sys.argv[1:] == ["memo_under_the_highest_pair_limit"]:
        print(json.dumps(memo_counts(limit=max(PAIR_LIMITS))))
    elif sys.argv[1:] == ["memo_few_ops"]:
        print(json.dumps(memo_counts(case=FEW_OPS)))
    else:
        check_stops()
