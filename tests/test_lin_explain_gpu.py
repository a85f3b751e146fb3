"""The explaining lin-kv check on the device (csrc/lin_check_dev.hip: lin_check_explain_kernel / lin_check_wg_explain_kernel)
through E.explain_lin_kv_batch (msim_explain_lin_kv_batch) and Engine.explain_lin_kv() (msim_explain_lin_kv): every byte of every key
record — Knossos' :op and :previous-ok rows, the register values of the :configs, the open calls — and every field of the check record
must be what the host entry (msim_explain_lin_kv_rows, csrc/lin_check.cpp) writes, at every level the search has: the registers, the HBM
pools of pass 1, the LDS pool of pass 2, the large HBM slots, the host search behind them.  With MSIM_DEV_FLAGS 0x2000 the pools are
small enough that every level is reached; the batch entry reads the switch once per process, so those cases run this file's tests again
in a child process (0x3000: with the developer trace, from which the child asserts that histories reached each level; the trace keeps
its timings in the check record, so a traced run compares ROUTE_FIELDS of it and the key records whole).  A last child runs under
MSIM_POISON.  tests/test_lin_explain_hipemu.py runs this file on the host wavefront emulator in the CPU suite."""
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import oracle_lib as O

import lin_explain_cases as K
from test_lin_check_gpu import DEV_FLAGS, FIELDS, ROUTE_FIELDS, TINY, TRACED, _histories, _routes, _with_one_read_changed

pytestmark = pytest.mark.gpu
_HOST = {}


def _host_of(hs):
    """the host entry's (check record, key records) of the histories `hs` (a tuple, kept: computed once per set)"""
    if id(hs) not in _HOST:
        _HOST[id(hs)] = (hs, [E.explain_lin_kv_history(h) for h in hs])
    return _HOST[id(hs)][1]


def _same(dev, host, what):
    assert len(dev) == len(host)
    for i, ((drec, dkeys), (hrec, hkeys)) in enumerate(zip(dev, host)):
        for f in (ROUTE_FIELDS if TRACED else FIELDS):
            assert int(drec[f]) == int(hrec[f]), (what, i, f, int(drec[f]), int(hrec[f]))
        assert len(dkeys) == len(hkeys) == int(hrec["attempt_count"]), (what, i, len(dkeys), len(hkeys))
        assert dkeys.tobytes() == hkeys.tobytes(), (what, i, [k for k in zip(dkeys, hkeys) if k[0] != k[1]][:3])


def _in_child(test, **env):
    """this file's `test` (a node id's tail) in a process of its own with `env` set before the library is loaded"""
    assert DEV_FLAGS == 0 and "MSIM_POISON" not in os.environ
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__) + "::" + test],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


HAND = tuple(K.encode(ops) for ops, _ in K.HAND.values()) + tuple(K.encode(K.with_nemesis(ops)) for ops, _ in K.HAND.values())


def test_hand_written_histories_device_equals_host(lib):
    host = _host_of(HAND)
    _same(E.explain_lin_kv_batch(list(HAND)), host, "hand-written")
    for (ops, want), (rec, keys) in zip(K.HAND.values(), host):   # (the host's records are the ones written out by hand: tests/test_lin_explain.py)
        assert [int(k["valid"]) for k in keys] == [w["valid"] for _, w in sorted(want.items())]
    # a slab of one record per history: the true key count, the first record only
    res = E.explain_lin_kv_batch(list(HAND), max_keys=1)
    for (rec, keys), (hrec, hkeys) in zip(res, host):
        assert int(rec["attempt_count"]) == len(hkeys) and len(keys) == 1 and keys.tobytes() == hkeys[:1].tobytes()


def _synthetic_set():
    hs = []
    for i, n_rows in enumerate((63, 64, 65, 129, 127, 128, 200, 300, 400, 333)):
        for j in range(3):
            hs.append(K.encode(K.synthetic(100 * i + j, n_rows, keys=((0,), (0, 1, 2), (5, 9, 200, 254))[j], workers=(2, 6, 10)[j], p_overlap=(0.05, 0.3, 0.5)[j],
                                           p_wrong=(0.0, 0.02, 0.05)[j], p_info=(0.0, 0.03, 0.06)[j], odd=(0.0, 0.0, 0.03)[j])))
    for n_open in (20, 63, 64, 70):   # up to 64 calls of one key open at once; beyond: "unknown" (and the pairing table of 64: the host's)
        hs.append(K.encode(K.many_open_calls(n_open, tail_reads=(1, 3, 3, 2))))
        hs.append(K.encode(K.many_open_calls(n_open, tail_reads=(1, 3, 1))))
    for n_writes, done, read_value, n_info in ((9, 3, 99, 0), (8, 3, 99, 1), (8, 1, 99, 0), (7, 2, 12, 2), (9, 4, 13, 0)):   # closures that start in a pool
        hs.append(K.encode(K.wide_then_bad_read(n_writes, done, read_value, n_info)))
    return tuple(hs)


SYNTHETIC = _synthetic_set()


def test_synthetic_histories_device_equals_host(lib):
    """63 / 64 / 65 / 129 rows (the 64-row chunks of the pairing pass and of the key walk), a few hundred rows with overlaps, wrong results,
    :fail, :info and rows no client produces, and 20 to 70 calls open at once"""
    host = _host_of(SYNTHETIC)
    res, n_host = E.explain_lin_kv_batch(list(SYNTHETIC), with_n_host=True)
    _same(res, host, "synthetic")
    valid = [int(k["valid"]) for _, keys in host for k in keys]
    assert {0, 1, 2} <= set(valid) and valid.count(0) >= 10, valid
    assert any(int(k["n_pending"]) > 0 for _, keys in host for k in keys) and any(int(k["n_values"]) > 1 for _, keys in host for k in keys)
    assert n_host >= 2   # more than 64 open calls
    assert sum(int(k["valid"]) == 0 and int(k["n_values"]) == 3 and int(k["n_pending"]) >= 5 for _, keys in host for k in keys) >= 2   # (wide_then_bad_read)


_WIDE = []


def _wide():
    """20 oracle histories of Raft under partitions and copies with one read changed"""
    if not _WIDE:
        rng = np.random.default_rng(5)
        good = _histories(20)
        _WIDE.append(tuple(good + [_with_one_read_changed(h, rng) for h in good]))
    return _WIDE[0]


@pytest.mark.parametrize("flags", [0, 0x2000, 0x3000])
def test_wide_keys_device_equals_host(lib, flags, capfd):
    """[0]: under the switches this process has.  [8192] (0x2000): case [0] in a child with the small pools: every level down to the host
    search; [12288] (0x3000): the same with the trace, which must show histories at every level."""
    if flags:
        return _in_child("test_wide_keys_device_equals_host[0]", MSIM_DEV_FLAGS=hex(flags))
    hs = _wide()
    host = _host_of(hs)
    n_good = len(hs) // 2
    assert all(int(rec["valid"]) == 1 for rec, _ in host[:n_good])
    assert sum(int(rec["valid"]) == 0 for rec, _ in host[n_good:]) >= n_good // 2   # (the seed: at least half the changed copies have an invalid key)
    capfd.readouterr()
    res, n_host = E.explain_lin_kv_batch(list(hs), with_n_host=True)
    err = capfd.readouterr().err
    _same(res, host, "wide keys")
    assert TRACED == ("[lin-check]" in err), err
    if TRACED:
        routes = _routes(err)
        print("lin-kv routes of the 40 wide-key histories, explained:", routes)
        assert routes["n"] == len(hs) and routes["open1"] > 0 and routes["host"] == n_host, routes
        if TINY:
            assert routes["grown"] > 0 and routes["open2"] > 0 and routes["host"] > 0, routes
    # the plain entry: the same check records, untouched by the explaining one
    plain = E.check_lin_kv_batch(list(hs))
    for i, (rec, _) in enumerate(host):
        for f in (ROUTE_FIELDS if TRACED else FIELDS):
            assert int(plain[i][f]) == int(rec[f]), (i, f)


def _proxy_cfg():
    # the proxy over a sequentially consistent service is not linearizable: stale reads in every instance (chosen on the CPU oracle)
    return E.test_config("lin-kv", bin="lin-kv-proxy", proxy_service="seq-kv", node_count=3, concurrency=6, rate=40, time_limit=4, latency=5, seed=1)


def test_engine_explain_lin_kv(lib):
    """Engine.explain_lin_kv() over the histories of a run where they lie in HBM: the host entry's records on the fetched histories, and
    check_results() as a plain Engine.check() leaves it"""
    n = 64
    with E.Engine(_proxy_cfg()) as eng:
        eng.run(0, n)
        res = eng.explain_lin_kv()
        after = eng.check_results()
        eng.check()
        plain = eng.check_results()
        eng.fetch()
        hs = [eng.raw_history(i)[0].copy() for i in range(n)]
        small = eng.explain_lin_kv(max_keys=1)
    host = [E.explain_lin_kv_history(h) for h in hs]
    assert sum(int(rec["error_count"]) > 0 for rec, _ in host) >= n // 4
    _same(res, host, "engine")
    for f in (ROUTE_FIELDS if TRACED else FIELDS):
        assert (after[f] == plain[f]).all() and all(int(rec[f]) == int(p[f]) for (rec, _), p in zip(res, plain)), f
    assert all(keys.tobytes() == hkeys[:1].tobytes() for (_, keys), (_, hkeys) in zip(small, host))
    a = E.lin_kv_analysis(hs[0], res[0][1])
    k = a["failures"][0]
    assert a["valid?"] is False and a["results"][k]["linearizable"]["op"]["type"] == ":ok"
    with E.Engine(E.test_config("echo", node_count=1, time_limit=1)) as eng:   # a context of another workload
        eng.run(0, 1)
        with pytest.raises(E.EngineError, match=r"\(-6\)"):
            eng.explain_lin_kv()


@pytest.mark.parametrize("test", ["test_hand_written_histories_device_equals_host", "test_synthetic_histories_device_equals_host", "test_engine_explain_lin_kv"])
def test_records_do_not_change_under_poison(lib, test):
    """every device allocation of a context poisoned before each launch (MSIM_POISON): the device still equals the host"""
    _in_child(test, MSIM_POISON="0xA5")
