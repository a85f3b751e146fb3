"""The steady leave of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, the flood instantiation: latency 0, at most four
neighbours): when a flood stretch ends because a half has run out of due envelopes, and that half's last
op round left it in the state R0's block and the exit test would only find again (its bit of sd_m), the half is parked, or both halves go
to their op round, straight from the stretch's exit: the same time jump, round count and count-down at the same round, without a pass
through the loop's head.  Every round, delivery and message is simulated as before, so on the host wavefront emulator (lanes out of
lockstep, MSIM_GUARD=3) every unflagged instance equals the oracle bit for bit: rows, payload, meta (n_rounds included) and the six
net-stats counters.  The emulator build also traps when a half taken by the fast path is not what the slow path would have found:
something held, queued or busy, sched_at not ahead of T, a special envelope due at the partner, one of st_m's compares false.

CASES: those of tests/test_duo_quiet_op_hipemu.py (7 clusters: an empty upper half, a single cluster, 31 nodes, two nodes, echo-back,
rate 2000 / 3000: halves that leave flood mode and ops that fall at gen_next == T, several blocks of draws, FEW_VALUES, whose clusters stop
being steady at the max_values stop, tree3, the line of 24, the partial grid of 7).  All of them run again on a -DDUO_PAIR_WAIT=2 build,
where count-downs run out and fast and slow leaves alternate inside a wavefront.  GPU_CASES are the same shapes at a time limit of at
most 1 s (tests/test_duo_steady_leave_gpu.py).  No instance of any of them is flagged by the oracle (test_no_case_is_flagged).
POISONED + [FEW_VALUES] run with every device buffer filled with 0xA5, in a process of their own; the three capacity stops are compared by
their flags, as everywhere in this project.

ROUND LIMITS.  An unflagged instance never ends with an envelope in flight, so the oracle cannot see whether the fast path looks at the round
limit where R0's block does.
Under MSIM_DUO_ROUND_LIMIT a cluster stops in the middle of a flood; what the kernel gives there, limit for limit, is held by the
one-cluster sweep of tests/test_duo_op_plan_hipemu.py against a -DDUO_NO_FLOOD build and by the recorded digests of that sweep and of two
clusters of the headline shape under the limits 40 .. 160 (tests/golden/duo_round_limits.json, tests/test_duo_trim_hipemu.py).

THE PATH IS TAKEN (a -DDUO_PROF -DDUO_PROF_STEADY emulator build, two clusters of the headline shape): steady parks plus steady leaves are
at least half of the rounds that leave the gossip loop or park a half.  This is a floor against a vacuous pass, not a measurement."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_duo_stretch_hipemu as S  # noqa: E402
from test_duo_quiet_op_hipemu import CASES, GPU_CASES, GPU_POISONED  # noqa: E402,F401
from test_duo_stretch_hipemu import HEADLINE, POISONED, _compare, _config, _variant, check_stops, emu_lib  # noqa: E402,F401
from test_duo_trim_hipemu import FEW_VALUES  # noqa: E402

STEADY_CASE = HEADLINE % 2


def steady_counts():
    """STEADY_CASE on the -DDUO_PROF -DDUO_PROF_STEADY library MSIM_LIB names: the rounds of the one wavefront that leave the gossip loop
    or park a half, and how many of them the steady leave took (see the epilogue of sim_kernel_duo)"""
    import oracle_lib as O
    E, cfg, n, flags = _config(STEADY_CASE)
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
        return {"general_bodies": lo.n_events & 0xFFFF, "generic_op_rounds": lo.n_events >> 16, "flood_op_rounds": up.reserved[0] & 0xFFFF,
                "parks": (lo.reserved[2] >> 16) & 0x7FF, "steady_parks": lo.reserved[1] & 0x7FF, "steady_leaves": (lo.reserved[1] >> 11) & 0x7FF}


def test_no_case_is_flagged():
    """the oracle alone: no instance of the cases, at either length, carries a flag"""
    import oracle_lib as O
    for case in CASES + POISONED + GPU_CASES + GPU_POISONED:
        _, cfg, n, _ = _config(case)
        ora = O.run(cfg, 0, n)
        assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n, case


def _self(lib, what, timeout=800):
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=S._env(lib), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.timeout(1800)
def test_duo_steady_leave_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(1800)
def test_duo_steady_leave_on_the_emulator_when_count_downs_run_out(emu_lib):
    _compare(_variant("steadyw2", ["-DDUO_PAIR_WAIT=2"]), CASES, {})


@pytest.mark.timeout(900)
def test_duo_steady_leave_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED + [FEW_VALUES], {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_steady_leave_on_the_emulator_stopped_by_a_capacity(emu_lib):
    assert "stops: OK" in _self(emu_lib, "stops")


@pytest.mark.timeout(900)
def test_duo_leaving_rounds_take_the_steady_path_on_the_emulator(emu_lib):
    prof = _variant("steadyprof", ["-DDUO_PROF", "-DDUO_PROF_STEADY"])
    c = json.loads(_self(prof, "steady").strip().splitlines()[-1])
    print(c)
    leaving = c["general_bodies"] + c["generic_op_rounds"] + c["flood_op_rounds"] + c["parks"]
    steady = c["steady_parks"] + c["steady_leaves"]
    assert leaving > 50, c
    assert c["steady_parks"] <= c["parks"] and c["steady_leaves"] <= c["flood_op_rounds"], c
    assert c["steady_parks"] > 0 and c["steady_leaves"] > 0, c
    assert 2 * steady >= leaving, f"{steady} steady parks and leaves of {leaving} leaving rounds: {c}"


if __name__ == "__main__":
    if sys.argv[1:] == ["steady"]:
        print(json.dumps(steady_counts()))
    else:
        check_stops()
