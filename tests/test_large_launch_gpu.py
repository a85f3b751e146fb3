"""Every kernel at the launch size and options the benchmarks use (tools/bench_configs.py, seed 99), bit-compared with the CPU oracle where a
launch goes wrong quietly: its END (a partial last wavefront, instances whose row / payload offsets lie past 4 GiB), instance ids that cross
2^32 in the middle of a launch (every packed kernel keys its RNG on first_instance + inst), and a one-cluster launch just below the packed
layout's threshold on the scratch the packed kernel left behind — three launches in one Engine context.  The device checker's verdicts on
the first launch are held, field by field, against the host checkers on the same histories.

Which kernel a launch took is read from its `[layout] <kernel> <n>` line (MSIM_DEV_FLAGS bit 12, set only around run(): the same bit makes
the checkers time their passes), so a moved threshold cannot quietly move a case onto another kernel."""
import concurrent.futures as cf
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
from launch_digests import digest_engine, digest_oracle
import oracle_lib as O
import setfull_ref as R
from test_set_full_batch_gpu import _compare as _compare_set_full

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bench_configs", os.path.join(ROOT, "tools", "bench_configs.py"))
BC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(BC)
GIB4 = 1 << 32
TRACE = 0x1000


def _headline():
    import bench
    return bench.headline_config(E, 99), 4096


def _bench(name):
    kw, n = BC.CONFIGS[name]
    return E.test_config(seed=99, **kw), n


# (id, config, expected kernel at the bench batch, the batch from which that kernel is taken or None, expected one-cluster kernel below it,
#  the slabs in which the last instances of launch 1 lie past 4 GiB: rows of 22714 x 16 B per unique-ids instance, payload words of the
#  transactional and kafka shapes)
CASES = [
    ("cfg2-headline", _headline, "duo", None, None, ()),
    ("cfg1-echo", lambda: _bench("cfg1 echo n=3"), "uid8", 4096, "general_a", ()),
    ("cfg3-gset-n100", lambda: _bench("cfg3 g-set n=100 lat100 exponential p_loss 0.05"), "wide_gset", None, None, ()),
    ("cfg4-raft-partitions", lambda: _bench("cfg4 lin-kv raft + partitions lat10"), "raft4", None, None, ()),
    ("cfg5-single-root", lambda: _bench("cfg5 txn-list-append n=5 rate100 30s lat5 + partitions"), "txn8", None, None, ("payload",)),
    ("cfg5-multi-key", lambda: _bench("cfg5-mk txn-list-append multi-key n=5 rate100 30s lat5 + partitions"), "mk8", None, None, ("payload",)),
    ("cfg5-datomic", lambda: _bench("cfg5-datomic txn-list-append datomic n=5 rate100 30s lat5 + partitions"), "dt8", 12288, "dt1", ("payload",)),
    ("datomic-n1-c10", lambda: _bench("txn-list-append datomic n=1 c=10 rate100 30s lat0"), "dtg4", 16384, "dtg", ("payload",)),
    ("single-root-n1-c10", lambda: _bench("txn-list-append n=1 c=10 rate100 30s lat5 (single-root node)"), "txng4", 8192, "txng", ("payload",)),
    ("single-root-n5-c10", lambda: _bench("txn-list-append n=5 c=10 rate100 30s lat5 + partitions (single-root node)"), "txng4", 8192, "txng", ("payload",)),
    ("lin-kv-proxy", lambda: _bench("lin-kv proxy n=5 c=10 rate30 60s lat5"), "svc4", 4096, "svc1", ()),
    ("unique-ids-tso", lambda: _bench("unique-ids over lin-tso n=3 rate1000 10s lat5 + partitions"), "svc4<TSO>", 4096, "svc1", ("rows",)),
    ("unique-ids-n3", lambda: _bench("unique-ids n=3 rate1000 10s lat5 + partitions"), "uid8", 4096, "general_a", ("rows",)),
    ("pn-counter-n5", lambda: _bench("pn-counter n=5 rate100 20s lat100 exponential"), "crdt8", 4096, "general_a", ()),
    ("kafka-n5", lambda: _bench("kafka n=5 rate100 20s lat5 + partitions"), "kafka8", 8192, "kafka1", ("payload",)),
    ("hat-n2", lambda: _bench("txn-rw-register hat n=2 rate100 30s + partitions"), "hat8", 3200 * 2, "hat1", ()),
    ("bcast-n100-wide", lambda: _bench("broadcast n=100 grid lat100 exponential"), "wide_bcast", None, None, ()),
]


def _oracle(cfg, first, idx):
    """Oracle digests of launch-relative instances `idx` of a launch that began at `first`: the contiguous runs of idx, split over threads
    (the oracle is C, the GIL is released during the call)."""
    groups, start = [], idx[0]
    for a, b in zip(idx, idx[1:] + [None]):
        if b != a + 1:
            for s in range(start, a + 1, 4):
                groups.append((s, min(4, a + 1 - s)))
            start = b
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        runs = list(ex.map(lambda g: (g[0], O.run(cfg, first + g[0], g[1])), groups))
    out = {}
    for s, ora in runs:
        for k in range(ora.n):
            out[s + k] = (digest_oracle(ora, k), ora)
    return out


def _launch(eng, capfd, first, n, kernel):
    eng.set_dev_flags(TRACE)
    try:
        eng.run(first, n)
    finally:
        eng.set_dev_flags(0)
    err = capfd.readouterr().err
    got = re.findall(r"^\[layout\] (\S+) (\d+)$", err, re.M)
    assert got == [(kernel, str(n))], (kernel, n, err[-2000:])


def _compare(eng, cfg, first, idx, what):
    ref = _oracle(cfg, first, idx)
    bad = [i for i in idx if digest_engine(eng, i) != ref[i][0]]
    assert not bad, f"{what}: {len(bad)} of {len(idx)} instances differ from the oracle, launch-relative: {bad[:8]} (first_instance {first})"
    assert all(eng.meta(i).flags == 0 for i in idx), what


FIELDS = {
    A.WL_TXN_LIST_APPEND: ("valid", "attempt_count", "stable_count", "lost_count", "stale_count", "error_count", "op_count", "ok_count", "fail_count", "info_count"),
    A.WL_LIN_KV: ("valid", "attempt_count", "error_count", "op_count", "ok_count", "fail_count", "info_count", "stable_count", "lost_count", "stale_count",
                  "never_read_count", "duplicated_count"),
    A.WL_KAFKA: ("valid", "attempt_count", "stable_count", "lost_count", "never_read_count", "duplicated_count", "error_count", "op_count", "ok_count",
                 "fail_count", "info_count"),
    A.WL_PN_COUNTER: ("valid", "attempt_count", "error_count", "stable_count", "op_count", "ok_count", "fail_count", "info_count"),
    A.WL_UNIQUE_IDS: ("valid", "attempt_count", "duplicated_count", "op_count", "ok_count", "fail_count", "info_count"),
}


def _host(cfg, rows, pay):
    """The host checker of cfg's workload on one history (the CheckResult msim_check_*_rows fills)."""
    lib, res = A.load(), A.CheckResult()
    rows = np.ascontiguousarray(rows); pay = np.ascontiguousarray(pay, dtype=np.uint32)
    r, p = rows.ctypes.data_as(C.c_void_p), pay.ctypes.data_as(C.c_void_p)
    wl = cfg.workload
    if wl == A.WL_TXN_LIST_APPEND:
        rc = lib.msim_check_txn_rows(r, len(rows), p, len(pay), C.byref(res))
    elif wl == A.WL_TXN_RW_REGISTER:
        rc = lib.msim_check_rw_rows(r, len(rows), p, len(pay), cfg.consistency_model, C.byref(res))
    elif wl == A.WL_LIN_KV:
        rc = lib.msim_check_lin_kv_rows(r, len(rows), C.byref(res))
    elif wl == A.WL_KAFKA:
        rc = lib.msim_check_kafka_rows(r, len(rows), p, len(pay), C.byref(res))
    elif wl == A.WL_PN_COUNTER:
        rc = lib.msim_check_pn_rows(r, len(rows), C.byref(res), None, 0, None)
    elif wl == A.WL_UNIQUE_IDS:
        rc = lib.msim_check_unique_rows(r, len(rows), C.byref(res))
    else:
        raise AssertionError(f"no host checker for workload {wl}")
    assert rc == 0
    return res


def _verdicts(eng, cfg, idx):
    """eng.check() on the whole launch; the compared instances' records against the host checker / the Python restatements."""
    eng.check()
    res = eng.check_results()
    assert len(res) == eng.n
    assert (res["valid"] == 1).all(), f"{int((res['valid'] != 1).sum())} of {eng.n} histories not valid"   # every bench shape is valid
    _records(eng, cfg, res, idx)


def _records(eng, cfg, res, idx):
    """The records `res` of the fetched launch's instances `idx` against the host checker / the Python restatements (shared with
    tests/pipeline_cases.py)."""
    wl = cfg.workload
    for i in idx:
        rows, pay = eng.raw_history(i)
        g = res[i]
        if wl in (A.WL_BROADCAST, A.WL_G_SET):
            _compare_set_full(cfg, [(rows, pay)], wl, res[i:i + 1])
        elif wl == A.WL_ECHO:
            ref = R.echo_check(E.decode_history(rows, pay, cfg.n_nodes, wl))
            assert (int(g["valid"]) == 1) == ref["valid?"] and int(g["error_count"]) == len(ref["errors"]), (i, g, ref)
        elif wl == A.WL_TXN_RW_REGISTER:
            # the device pass proves a history free of what the model proscribes; where it decides, its anomaly bits / edge count are its
            # own subgraph's (a subset of the host's: tests/test_rw_check_gpu.py::_agree), everything else is the host's record
            h = _host(cfg, rows, pay)
            for f in ("valid", "attempt_count", "op_count", "ok_count", "fail_count", "info_count", "stable_count"):
                assert int(g[f]) == int(getattr(h, f)), (i, f, int(g[f]), int(getattr(h, f)))
            assert int(g["error_count"]) & ~int(h.error_count) == 0, (i, g, h.error_count)
        else:
            h = _host(cfg, rows, pay)
            for f in FIELDS[wl]:
                assert int(g[f]) == int(getattr(h, f)), (i, f, int(g[f]), int(getattr(h, f)))
            if wl == A.WL_UNIQUE_IDS:
                assert [int(x) for x in g["stable_latency_ms"][:2]] == [int(h.stable_latency_ms[0]), int(h.stable_latency_ms[1])], i


@pytest.mark.timeout(240)
@pytest.mark.parametrize("name,make,kernel,threshold,below,past4g", CASES, ids=[c[0] for c in CASES])
def test_bench_size_launch_end_and_crossings(lib, capfd, name, make, kernel, threshold, below, past4g):
    cfg, batch = make()
    slab_rows, slab_pay = cfg.max_rows * 16, cfg.max_payload_words * 4
    with E.Engine(cfg) as eng:
        # 1. a partial last wavefront: the first 8, 8 from the middle, the last 24 (the partial wavefront and full ones before it)
        n1 = batch + 3
        _launch(eng, capfd, 0, n1, kernel)
        idx = list(range(8)) + list(range(n1 // 2 - 4, n1 // 2 + 4)) + list(range(n1 - 24, n1))
        eng.fetch()
        _compare(eng, cfg, 0, idx, f"{name} launch 1 (0, {n1})")
        _verdicts(eng, cfg, idx)
        last = idx[-1]
        crossed = tuple(s for s, per in (("rows", slab_rows), ("payload", slab_pay)) if last * per >= GIB4)
        assert crossed == past4g, (name, crossed, past4g)   # (the slab sizes of the bench options, so that the case keeps covering what it claims)
        with capfd.disabled():
            print(f"[large-launch] {name}: {kernel} x {n1}, last compared instance {last}: row offset {last * slab_rows / 2**30:.2f} GiB, "
                  f"payload offset {last * slab_pay / 2**30:.2f} GiB; past 4 GiB: {', '.join(crossed) or 'none'}")

        # 2. instance ids crossing 2^32 in the middle of the launch: 16 on each side of the crossing and the last 8
        f2 = GIB4 - batch // 2
        _launch(eng, capfd, f2, batch, kernel)
        eng.fetch()
        mid = batch // 2
        _compare(eng, cfg, f2, list(range(mid - 16, mid + 16)) + list(range(batch - 8, batch)), f"{name} launch 2 ({f2}, {batch})")

        # 3. one below the threshold: the one-cluster kernel on the scratch the packed kernel wrote
        if threshold:
            n3 = threshold - 1
            _launch(eng, capfd, 5, n3, below)
            eng.fetch()
            _compare(eng, cfg, 5, list(range(8)) + list(range(n3 - 8, n3)), f"{name} launch 3 (5, {n3})")

