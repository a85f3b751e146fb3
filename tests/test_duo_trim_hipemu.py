"""The trims of the stretch instantiation of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip, the flood instantiation: latency 0, at most
four neighbours):
  (A) no body counts the delivered server envelopes: servers_recv = servers_send - what is queued or held when the cluster stops;
  (B) the flood bodies do not store the node's set word: a half in flood mode writes it back once, at the head of an op round in which it
      acts and when it leaves flood mode, and an acting half takes the op's word from the register;
  (C) an op wave-round derives its half's offsets once; rows and payload are addressed by 32-bit byte offsets.
Every round, delivery and message is simulated as before, so on the host wavefront emulator (lanes out of lockstep, MSIM_GUARD=3) every
unflagged instance equals the oracle bit for bit: rows, payload, meta (n_rounds included) and the six net-stats counters.

CASES: those of tests/test_duo_stretch_hipemu.py (more than 32 broadcasts per cluster: the flood's word changes; an empty upper half at 7
clusters; rate 2000 / 3000: materialisation, generic halves beside flood halves; 31 nodes, two nodes, echo-back, several blocks of draws),
a single cluster, and a shape of 64 values at most whose clusters broadcast 33 to 63 of them: the values end shortly after the word
boundary (test_no_case_is_flagged checks both, on the oracle alone; a shape that RUNS OUT of its 64 values, at the boundary, is among the
stops).  POISONED runs with every device buffer filled with 0xA5 before the launch, in a process of its own: a read that finds a set word
the deferred store has not written copies poison.  The three capacity stops are compared by their flags, as everywhere in this project.

THE RECORDED ROUND LIMITS.  An unflagged instance never ends with an envelope in flight, so the oracle cannot see a wrong servers_recv, a
late write-back, a delivery that skips the queue or a look at the limit in another round at a stop.  Under MSIM_DUO_ROUND_LIMIT a cluster
stops in the middle of a flood: the one-cluster sweep of tests/test_duo_op_plan_hipemu.py (LIMITS) and two clusters of the headline shape
under the limits 40 .. 160 (PAIR_LIMITS) must give, limit for limit, what tests/golden/duo_round_limits.json holds: rows, payload, meta
and all six net-stats counters.  The file is what `python tests/test_duo_trim_hipemu.py limits` printed at commit f51b6dc, the last one
whose duo.hip could be built with each of its optimisation levels switched off: "one" from the -DDUO_NO_FLOOD emulator build, "pair" from
the -DDUO_NO_STRETCH emulator build (the oldest level with paired op rounds: pairing changes which rounds a cluster takes beside its
partner).  At that commit the product build and the builds without the trims, the quiet op round, the steady leave, the memo, the steady
run, the block plan and the flood table gave the same two sweeps, and every build the same one-cluster sweep.  The one-cluster sweep is
also held against a live -DDUO_NO_FLOOD build (tests/test_duo_op_plan_hipemu.py).  A deliberate change of these outputs is recorded again
from the then-current product build, in the commit that makes it, and reviewed as such.
tests/test_duo_trim_gpu.py runs the cases on the device."""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_duo_stretch_hipemu as S  # noqa: E402
from test_duo_stretch_hipemu import HEADLINE, POISONED, _compare, _config, _variant, check_stops, emu_lib  # noqa: E402,F401

ONE_CLUSTER = HEADLINE % 1
# at most 64 values; the clusters broadcast 33 .. 63 of them
FEW_VALUES = "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':0.8,'n':4,'inbox_capacity':6,'max_values':64,'seed':51,'flags':0x400}"
ADDED = [ONE_CLUSTER, FEW_VALUES]
CASES = S.CASES + ADDED
PAIR_LIMITS = list(range(40, 161))
GOLDEN = os.path.join(ROOT, "tests", "golden", "duo_round_limits.json")
NET = ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv")


def pair_limit_sweep():
    """Two clusters of the headline shape under every limit of PAIR_LIMITS on whatever library MSIM_LIB names: {limit: [per instance:
    n_rows, n_payload_words, flags, n_rounds, the digest of rows and payload, the six net-stats counters]}"""
    E, cfg, n, flags = _config(HEADLINE % 2)
    out = {}
    for lim in PAIR_LIMITS:
        os.environ["MSIM_DUO_ROUND_LIMIT"] = str(lim)
        try:
            with E.Engine(cfg) as eng:
                eng.set_dev_flags(flags)
                eng.run(0, n)
                eng.fetch()
                dig = []
                for i in range(n):
                    rows, pay = eng.raw_history(i)
                    m, st = eng.meta(i), eng.net_stats_raw(i)
                    dig.append([m.n_rows, m.n_payload_words, m.flags, m.n_rounds, hashlib.sha256(rows.tobytes() + pay.tobytes()).hexdigest()] +
                               [int(getattr(st, f)) for f in NET])
                out[str(lim)] = dig
        finally:
            del os.environ["MSIM_DUO_ROUND_LIMIT"]
    return out


def test_no_case_is_flagged():
    """the oracle alone: no instance of CASES or POISONED carries a flag; FEW_VALUES ends between the word boundary and its 64 values"""
    import numpy as np
    import oracle_lib as O
    for case in CASES + POISONED:
        _, cfg, n, _ = _config(case)
        ora = O.run(cfg, 0, n)
        assert [int(ora.meta[i]["flags"]) for i in range(n)] == [0] * n, case
        if case == FEW_VALUES:
            for i in range(n):
                rows = np.frombuffer(ora.history(i)[0].tobytes(), dtype=np.uint32).reshape(-1, 4)
                bcasts = sum(1 for w in rows[:, 2] if int(w) & 0x7FF == (1 << 2))   # MSIM_T_INVOKE rows of MSIM_F_BROADCAST
                assert 33 <= bcasts <= 63, f"instance {i} broadcasts {bcasts} values"


def _self(lib, what, timeout=800):
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, env=S._env(lib), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, what + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.timeout(1800)
def test_duo_trim_on_the_emulator_equals_the_oracle(emu_lib):
    _compare(emu_lib, CASES, {})


@pytest.mark.timeout(900)
def test_duo_trim_on_the_emulator_with_poisoned_buffers(emu_lib):
    _compare(emu_lib, POISONED + [FEW_VALUES], {"MSIM_POISON": "0xA5"})


@pytest.mark.timeout(900)
def test_duo_trim_on_the_emulator_stopped_by_a_capacity(emu_lib):
    assert "stops: OK" in _self(emu_lib, "stops")


@pytest.mark.timeout(1800)
def test_duo_round_limits_are_the_recorded_ones(emu_lib):
    """both sweeps of the product emulator build against tests/golden/duo_round_limits.json (see THE RECORDED ROUND LIMITS above)"""
    from test_duo_op_plan_hipemu import LIMITS
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(_self(emu_lib, "limits").strip().splitlines()[-1])
    assert sorted(got) == sorted(want) == ["one", "pair"]
    for sweep, limits in (("one", LIMITS), ("pair", PAIR_LIMITS)):
        a, b = got[sweep], want[sweep]
        assert sorted(a) == sorted(b) == sorted(str(x) for x in limits)
        assert all(len(row) == 5 + len(NET) for d in a.values() for row in d)
        diff = [k for k in a if a[k] != b[k]]
        assert not diff, f"{sweep}: the build and the recorded sweep differ at the limits {diff[:10]}: {a[diff[0]]} != {b[diff[0]]}"
    # the pair sweep does stop clusters with envelopes in flight: servers_recv < servers_send somewhere
    assert any(row[-1] < row[-2] for d in got["pair"].values() for row in d)


if __name__ == "__main__":
    if sys.argv[1:] == ["limits"]:
        from test_duo_op_plan_hipemu import limit_sweep
        print(json.dumps({"one": limit_sweep()[0], "pair": pair_limit_sweep()}))
    else:
        check_stops()
