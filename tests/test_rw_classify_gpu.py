"""The device classification of rw-register dependency cycles (csrc/rw_check_dev.hip, rw_classify_kernel) against the host analysis
(msim_check_rw_rows = check_rw + finish + classify + judge of csrc/txn_check.cpp), every field of CHECK_DT, under all five models.

Two entries reach the kernel:
  * E.classify_rw_batch (msim_classify_rw_batch) and Engine.check(classify=True): EVERY record is the host's, byte for byte;
  * E.check_rw_batch (msim_check_rw_batch) and Engine.check(): a history that the first pass (rw_check_kernel) proves valid keeps that
    pass's record (verdict and counts of the host, the non-cycle anomalies it saw, the edges IT built: tests/test_rw_check_gpu.py::_agree);
    every other record — every invalid history among them — is the host's, byte for byte.
Neither hands a history to the host (n_host == 0) unless the history is beyond a device capacity; MSIM_DEV_FLAGS bit 0x2000 makes the
classification's capacity 16 transactions per strongly connected component, so that the host fallback is reached (CAPACITY)."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import oracle_lib as O

pytestmark = pytest.mark.gpu

MODELS = ["read-uncommitted", "read-committed", "snapshot-isolation", "serializable", "strict-serializable"]
BITS = {name: bit for bit, name in A.ANOMALIES.items()}
TINY = bool(int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0) & 0x2000)   # the classification's capacity is 16 transactions: CAPACITY's child
R, W = ":r", ":w"
_HOST = {}


def _host(hs, model):
    """msim_check_rw_rows' records of the histories `hs` (a tuple, kept: computed once per set and model)"""
    key = (id(hs), model)
    if key not in _HOST:
        lib = A.load()
        out = np.zeros(len(hs), dtype=E.CHECK_DT)
        for i, (rows, pay) in enumerate(hs):
            rows = np.ascontiguousarray(rows); pay = np.ascontiguousarray(pay, dtype=np.uint32)
            res = A.CheckResult()
            rc = lib.msim_check_rw_rows(rows.ctypes.data_as(C.c_void_p), len(rows), pay.ctypes.data_as(C.c_void_p), len(pay), E.CONSISTENCY_MODELS[model], C.byref(res))
            assert rc == 0, (i, rc)
            out[i] = np.frombuffer(bytes(res), dtype=E.CHECK_DT)[0]
        _HOST[key] = (hs, out)
    return _HOST[key][1]


def _same(got, host, what):
    for i in range(len(host)):
        assert got[i].tobytes() == host[i].tobytes(), (what, i, got[i], host[i])


def _both_entries(hs, expect_host=False):
    """classify_rw_batch: the host's records; check_rw_batch: the host's records but for the histories the first pass proves valid"""
    for model in MODELS:
        host = _host(hs, model)
        full, n_host = E.classify_rw_batch(list(hs), model)
        _same(full, host, ("classify", model))
        res, n_host2 = E.check_rw_batch(list(hs), model)
        for i in range(len(hs)):
            g, h = res[i], host[i]
            if g.tobytes() == h.tobytes():
                continue
            # the first pass's own record: only of a history it proved valid
            assert int(g["valid"]) == int(h["valid"]) and int(h["valid"]) != 0, (model, i, g, h)
            assert int(g["error_count"]) & ~int(h["error_count"]) == 0 and int(g["stale_count"]) == 0, (model, i, g, h)
            for f in ("attempt_count", "stable_count", "op_count", "ok_count", "fail_count", "info_count"):
                assert int(g[f]) == int(h[f]), (model, i, f, g, h)
        if expect_host:
            assert n_host > 0 and n_host2 <= n_host, (model, n_host, n_host2)
        else:
            assert n_host == 0 and n_host2 == 0, (model, n_host, n_host2)


def _cfg(**kw):
    args = dict(workload="txn-rw-register", node_count=2, rate=100.0, time_limit=6.0, seed=11)
    args.update(kw)
    return E.test_config(**args)


SHAPES = [
    dict(),                                                                    # 16 of 16 G2 under serializable
    dict(rate=50.0, time_limit=2.0),                                           # 9 G2, 7 valid under serializable (G-single + realtime)
    dict(rate=30.0, time_limit=1.0, nemesis=("partition",), nemesis_interval=0.5),
    dict(node_count=3, nemesis=("partition",), nemesis_interval=2.0, latency=20, latency_dist="exponential", p_loss=0.02),   # :info transactions
    dict(node_count=5, latency=10, latency_dist="uniform"),                    # the largest cycles
    dict(node_count=3, concurrency=18, time_limit=3.0, latency=5),             # six workers per node
]


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_engine_histories_are_classified_on_the_device(lib, shape):
    o = O.run(_cfg(**SHAPES[shape]), 0, 16)
    hs = tuple(o.history(i) for i in range(16))
    host = _host(hs, "serializable")
    res, n_host = E.check_rw_batch(list(hs), "serializable")
    assert n_host == 0
    if shape == 0:
        assert (res["valid"] == 0).all() and (host["error_count"] & BITS["G2"] != 0).all()
    for i in range(16):
        if int(host[i]["valid"]) == 0:
            assert res[i].tobytes() == host[i].tobytes(), (i, res[i], host[i])
    _both_entries(hs)


def _ops(*txns):
    """[(process, type, request, completed)] one after the other (type None: never completes)"""
    ops = []
    for p, typ, req, done in txns:
        ops.append({"type": ":invoke", "process": p, "f": ":txn", "value": req})
        if typ:
            ops.append({"type": typ, "process": p, "f": ":txn", "value": done})
    return ops


def _concurrent(*txns):
    """every transaction invoked before any completes: no realtime edges"""
    return ([{"type": ":invoke", "process": p, "f": ":txn", "value": req} for p, typ, req, done in txns] +
            [{"type": typ, "process": p, "f": ":txn", "value": done} for p, typ, req, done in txns if typ])


def _w(k, v):
    return [W, k, v]


HAND = {
    "G0": (_concurrent((0, ":ok", [[R, 1, None], _w(1, 2), _w(2, 1)], [[R, 1, 1], _w(1, 2), _w(2, 1)]),
                       (1, ":ok", [[R, 2, None], _w(2, 2), _w(1, 1)], [[R, 2, 1], _w(2, 2), _w(1, 1)])), {"G0"}),
    "G1c": (_concurrent((0, ":ok", [_w(1, 1), [R, 2, None]], [_w(1, 1), [R, 2, 1]]), (1, ":ok", [_w(2, 1), [R, 1, None]], [_w(2, 1), [R, 1, 1]])), {"G1c"}),
    "G-single": (_concurrent((0, ":ok", [[R, 1, None], [R, 2, None]], [[R, 1, None], [R, 2, 1]]), (1, ":ok", [_w(1, 1), _w(2, 1)], [_w(1, 1), _w(2, 1)])), {"G-single"}),
    "G2": (_concurrent((0, ":ok", [[R, 1, None], _w(2, 1)], [[R, 1, None], _w(2, 1)]), (1, ":ok", [[R, 2, None], _w(1, 1)], [[R, 2, None], _w(1, 1)])), {"G2"}),
    "G-single-realtime": (_ops((0, ":ok", [_w(1, 1)], [_w(1, 1)]), (1, ":ok", [[R, 1, None]], [[R, 1, None]])), {"G-single", "realtime"}),
    # A -rw-> B -rw-> C, and C completed before A began; B overlaps both
    "G2-realtime": ([{"type": ":invoke", "process": 1, "f": ":txn", "value": [_w(1, 1), [R, 2, None]]},
                     {"type": ":invoke", "process": 2, "f": ":txn", "value": [_w(2, 1)]}, {"type": ":ok", "process": 2, "f": ":txn", "value": [_w(2, 1)]},
                     {"type": ":invoke", "process": 0, "f": ":txn", "value": [[R, 1, None]]}, {"type": ":ok", "process": 0, "f": ":txn", "value": [[R, 1, None]]},
                     {"type": ":ok", "process": 1, "f": ":txn", "value": [_w(1, 1), [R, 2, None]]}], {"G2", "realtime"}),
    "internal": (_ops((0, ":ok", [_w(1, 1), [R, 1, None]], [_w(1, 1), [R, 1, None]])), {"internal"}),
    "G1a": (_ops((0, ":fail", [_w(1, 1)], [_w(1, 1)]), (1, ":ok", [[R, 1, None]], [[R, 1, 1]])), {"G1a"}),
    "G1b": (_concurrent((0, ":ok", [_w(1, 1), _w(1, 2)], [_w(1, 1), _w(1, 2)]), (1, ":ok", [[R, 1, None]], [[R, 1, 1]])), {"G1b"}),
    # key 1's version order is cyclic (it contributes no edges); keys 2 and 3 carry a write skew
    "cyclic-versions": (_concurrent((0, ":ok", [[R, 1, None], _w(1, 1)], [[R, 1, 2], _w(1, 1)]), (1, ":ok", [[R, 1, None], _w(1, 2)], [[R, 1, 1], _w(1, 2)]),
                                    (2, ":ok", [[R, 2, None], _w(3, 1)], [[R, 2, None], _w(3, 1)]), (3, ":ok", [[R, 3, None], _w(2, 1)], [[R, 3, None], _w(2, 1)])),
                        {"cyclic-versions", "G1c"}),   # (the two reads of key 1 are a wr cycle; the skew's two transactions count in stale_count)
    "no-ok": (_ops((0, ":fail", [_w(1, 1)], [_w(1, 1)]), (1, None, [[R, 1, None]], None)), set()),
}
HAND_HS = tuple(E.encode_txn_history(ops, rw=True) for ops, _ in HAND.values())


def test_hand_made_histories_one_per_class(lib):
    host = _host(HAND_HS, "strict-serializable")
    for i, (name, (_, want)) in enumerate(HAND.items()):
        got = {n for b, n in A.ANOMALIES.items() if int(host[i]["error_count"]) & b}
        assert got == want, (name, got, want)
    assert int(host[len(HAND) - 1]["valid"]) == 2
    _both_entries(HAND_HS)


def synth(seed, n_txn, P=4, K=3, window=3, p_future=0.3, p_fail=0.05, p_info=0.05):
    """a history whose reads may return values written up to `window` transactions LATER: G0, G1c and plain G-single, which the
    engine's histories never show"""
    rng = random.Random(seed); nextv = [1] * K; plan = []
    for t in range(n_txn):                       # shapes and writes: unique values per key, < 63
        mops = []
        for _ in range(rng.randint(1, 4)):
            k = rng.randrange(K)
            if rng.random() < 0.5 and nextv[k] < 63:
                mops.append([":w", k, nextv[k]]); nextv[k] += 1
            else:
                mops.append([":r", k, None])
        plan.append(mops)
    wrote = [[(t, m[2]) for t, ms in enumerate(plan) for m in ms if m[0] == ":w" and m[1] == k] for k in range(K)]
    done = []
    for t, mops in enumerate(plan):              # reads: own last micro-op on the key, else nil or a value written nearby
        d = []
        for f, k, v in mops:
            if f == ":r":
                mine = [m for m in d if m[1] == k]
                if mine:
                    v = mine[-1][2]
                else:
                    hi = t + window if rng.random() < p_future else t - 1
                    c = [x for tt, x in wrote[k] if t - window <= tt <= hi and tt != t]
                    v = rng.choice(c) if c and rng.random() < 0.85 else None
            d.append([f, k, v])
        done.append(d)
    ops, open_, t = [], {}, 0
    while t < n_txn or open_:                    # interleave P processes
        p = rng.randrange(P)
        if p in open_:
            i, typ = open_.pop(p)
            ops.append({"type": typ, "process": p, "f": ":txn", "value": done[i] if typ == ":ok" else plan[i]})
        elif t < n_txn:
            typ = ":fail" if rng.random() < p_fail else ":info" if rng.random() < p_info else ":ok"
            ops.append({"type": ":invoke", "process": p, "f": ":txn", "value": plan[t]}); open_[p] = (t, typ); t += 1
    return ops


def _case(seed):
    return synth(seed, n_txn=[6, 20, 60, 130][seed % 4], P=[2, 4, 8][seed % 3], K=[2, 3, 5][(seed // 3) % 3], window=[1, 3, 8][(seed // 7) % 3],
                 p_future=[0, .2, .5][(seed // 5) % 3])


_RANDOM = []


def _random_hs():
    if not _RANDOM:
        _RANDOM.append(tuple(E.encode_txn_history(_case(s), rw=True) for s in range(240)))
    return _RANDOM[0]


def test_random_histories_with_reads_from_the_future(lib):
    """seeds 0-239: every cycle class, up to 130 transactions (three 64-wide chunks), components past one 64-bit word of a matrix row.
    Under MSIM_DEV_FLAGS bit 0x2000 (test_capacity_fallback's child) some components exceed the capacity and the host finishes them."""
    hs = _random_hs()
    host = _host(hs, "strict-serializable")
    e = host["error_count"]
    count = lambda name: int((e & BITS[name] != 0).sum())
    assert count("G0") >= 1 and count("G1c") >= 10 and count("G-single") >= 10 and count("G2") >= 10, [(n, count(n)) for n in BITS]
    assert count("realtime") >= 5 and count("cyclic-versions") >= 1 and int((e == 0).sum()) >= 10, [(n, count(n)) for n in BITS]
    assert int(host["stale_count"].max()) > 64 and int(host["attempt_count"].max()) > 128
    _both_entries(hs, expect_host=TINY)


def test_capacity_fallback(lib):
    """The random set again in a process of its own under MSIM_DEV_FLAGS=0x2000 (the batch entries read the switch from the environment,
    once per process): n_host > 0, and the records are still the host's."""
    assert not TINY
    env = dict(os.environ, MSIM_DEV_FLAGS="0x2000")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "test_random_histories"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_engine_check_classify(lib):
    cfg = _cfg(node_count=3, rate=80.0, time_limit=5.0, latency=5)
    with E.Engine(cfg) as eng:
        eng.run(0, 16)
        eng.check(classify=True)
        assert eng.check_host_rechecks() == 0
        res = eng.check_results().copy()
        eng.set_dev_flags(0x10000)       # at most 7 histories per launch: three launches of the classification
        eng.check(classify=True)
        assert eng.check_results().tobytes() == res.tobytes()
        eng.set_dev_flags(0)
        eng.fetch()
        hs = tuple((eng.raw_history(i)[0].copy(), eng.raw_history(i)[1].copy()) for i in range(16))
        _same(res, _host(hs, "read-committed"), "Engine.check(classify=True)")
        census = E.anomaly_census(res)
        assert set(census) == set(A.ANOMALIES.values()) | {"clean"}
        assert census["clean"] + int((res["error_count"] != 0).sum()) == 16 and all(0 <= v <= 16 for v in census.values())
        assert census == E.anomaly_census(_host(hs, "read-committed"))
        assert (res["valid"] == 1).all() and census["G2"] + census["G-single"] > 0    # read-committed allows what these histories show
        eng.check()                      # and back: the first pass's records, no cycle classes
        plain = eng.check_results()
        assert eng.check_host_rechecks() == 0 and (plain["valid"] == 1).all() and (plain["stale_count"] == 0).all()
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        assert A.load().msim_set_check_classify(eng._ctx, 1) == A.E_UNSUPPORTED
