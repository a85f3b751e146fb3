"""The asynchronous, pipelined launch path — what bench.py's headline number, its fetch-inclusive leg and tools/bench_configs.py,
tools/overlap_configs.py and tools/cfg2_overlap.py are measured on — against the oracle and the reference checkers:

  a. the benchmark's own step / retire / drain loop, three engine contexts in flight, check() straight after run_async(), every instance
     of every step against the oracle and every record against the host checker / the Python restatements; seven configurations and one
     run with three different configurations in flight together;
  b. check() straight after run_async() for the checkers that copy the instance meta to the host to size what they hand to the host
     analysis (txn-rw-register, lin-kv with small pools, txn-list-append and kafka on truncated histories): a stale copy changes op_count;
  c. the split fetch (fetch_begin / fetch) in the order of bench.py's fetch_inclusive, two contexts alternating, a launch straight over
     a pending fetch, the accessors in between, rows / payload / stats / meta / journal against the oracle of the context's own batch;
  d. two asynchronous launches back to back on one context, and a launch on the caller's own stream;
  e. the five sums bench.py accumulates from its device views, against the same sums from the oracle and the reference checkers.

No run of the engine serves as a reference; every comparison is exact; nothing here asserts a time.  tests/test_pipeline_hipemu.py runs
this file on the host wavefront emulator (synchronous: the state machine, the regrown mirrors and the compaction kernels; the ordering
itself needs the device)."""
import time

import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import pipeline_cases as P
from test_large_launch_gpu import _host

pytestmark = pytest.mark.gpu

_RUNS = {}


def _pipeline(names, steps, capfd):
    key = (tuple(names), steps)
    if key not in _RUNS:
        _RUNS[key] = P.Pipeline(names, capfd).run(steps)
    return _RUNS[key]


# ---- a. the benchmark's pipeline ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(P.CONFIGS))
def test_three_contexts_in_flight_equal_the_oracle(lib, capfd, name):
    """Depth 3, 7 steps: contexts are reused, the last round is partial, a context's batch grows and shrinks while the others' launches
    are in flight."""
    p = _pipeline([name] * 3, 7, capfd)
    with capfd.disabled():
        print("\n" + p.line(f"{name} ({P.CONFIGS[name][1]})"))


@pytest.mark.timeout(300)
def test_three_different_configurations_in_flight_equal_the_oracle(lib, capfd):
    names = ["headline", "gset100", "txn-partitions"]
    p = _pipeline(names, 7, capfd)
    with capfd.disabled():
        print("\n" + p.line("duo + wide_gset + txn8"))


# ---- e. the benchmark's bookkeeping -------------------------------------------------------------------------------------------------------
def test_benchmark_sums_equal_the_oracle_and_the_reference_checkers(lib, capfd):
    """bench.py's acc — stats[:, 0], check[:, 0] == 1, meta[:, 2] != 0, meta[:, 0], meta[:, 1] summed over its views of device_buffers()
    straight after every pipelined check() — over the headline pipeline (the run of test a; each step's sums are held against the oracle
    there, the totals here)."""
    p = _pipeline(["headline"] * 3, 7, capfd)
    assert p.acc == p.want
    assert p.acc[1] == sum(n for _, n, _, _ in p.ms) and p.acc[2] == 0   # the headline shape: every history valid, no instance flagged
    assert p.acc[0] > 0 and p.acc[3] > 0 and p.acc[4] > 0
    with capfd.disabled():
        print(f"\n[pipeline] bench sums (msgs, valid, flagged, rows, payload words): {p.acc}; " + p.line("headline"))


# ---- b. check straight after an asynchronous launch ---------------------------------------------------------------------------------------
def _check_after_async(capfd, title, cfg, n, flags, compare=True):
    """A fresh context; a blocking run WITHOUT a check (the meta slab holds sane sizes of other instances, no check record exists);
    then run_async and check at once.  Returns (engine-side records, host rechecks, the oracle batch) after the comparisons."""
    t0 = time.perf_counter()
    P.oracle(cfg, 0, n)
    with E.Engine(cfg) as eng:
        eng.run(100, n)
        eng.set_dev_flags(flags)
        eng.run_async(0, n)
        eng.check()
        rechecks = eng.check_host_rechecks()
        res = eng.check_results()
        sim, chk = P.finite_ms(eng, title)
        eng.fetch()
        if compare:
            ref = P.compare_batch(eng, cfg, 0, n, title)
            P.compare_records(eng, cfg, res, title)
            # (a condition of the test: the warm-up left another n_rows in every instance's meta, so a stale copy of it shows in op_count)
            warm = P.oracle(cfg, 100, n)
            assert all(int(warm.meta(i)["n_rows"]) != int(ref.meta(i)["n_rows"]) for i in range(n)), title
        else:
            ref = P.oracle(cfg, 0, n)
            got = [eng.meta(i).flags for i in range(n)]
            assert got == [int(ref.meta(i)["flags"]) for i in range(n)], title
        hist = [tuple(x.copy() for x in eng.raw_history(i)) for i in range(n)]
    with capfd.disabled():
        print(f"\n[pipeline] {title}: n {n}, kernel_ms sim {sim:.2f} check {chk:.2f}, host rechecks {rechecks}; wall {time.perf_counter() - t0:.1f} s")
    return res, rechecks, ref, hist


def test_rw_register_check_straight_after_async_launch(lib, capfd):
    """7 of the 8 histories go to the host analysis, which is sized by the host copy of the meta: every count equals msim_check_rw_rows on
    the fetched history."""
    cfg = E.test_config("txn-rw-register", node_count=5, rate=100, time_limit=6, latency=5, nemesis=["partition"], nemesis_interval=2,
                        consistency_model="serializable", seed=21)
    res, rechecks, _, hist = _check_after_async(capfd, "txn-rw-register, dev flag 0x2000", cfg, 8, 0x2000)
    assert rechecks >= 1   # (a condition of the test: without a host recheck the path is not taken)
    for i, (rows, pay) in enumerate(hist):
        h = _host(cfg, rows, pay)
        for f in ("valid", "op_count", "ok_count", "fail_count", "info_count", "attempt_count", "stable_count"):
            assert int(res[i][f]) == int(getattr(h, f)), (i, f, int(res[i][f]), int(getattr(h, f)))
        assert int(res[i]["error_count"]) & ~int(h.error_count) == 0, (i, res[i], h.error_count)


def test_lin_kv_check_straight_after_async_launch(lib, capfd):
    """The lin-kv twin: the small pools of dev flag 0x2000, a partition every second (timed-out writes and cas stay pending on their
    keys), so that histories reach the host search — all 8 on the emulator (tests/test_lin_check_gpu.py's shape at rate 30 with a
    partition every 10 s sends 1 of 16 there)."""
    cfg = E.test_config("lin-kv", bin="raft", node_count=5, rate=100, time_limit=10, latency=10, nemesis=["partition"], nemesis_interval=1, seed=99)
    res, rechecks, _, hist = _check_after_async(capfd, "lin-kv, dev flag 0x2000", cfg, 8, 0x2000)
    assert rechecks >= 1   # (a condition of the test, as above)


@pytest.mark.parametrize("workload", ["txn-list-append", "kafka"])
def test_truncated_histories_check_straight_after_async_launch(lib, capfd, workload):
    """max_rows = 128: every instance stops at the capacity, so none is valid, and the flags are the oracle's."""
    cfg = E.test_config(workload, node_count=5, rate=100, time_limit=6, latency=5, nemesis=["partition"], nemesis_interval=2, seed=21, max_rows=128)
    n = 8
    res, _, ref, _ = _check_after_async(capfd, f"{workload}, max_rows 128", cfg, n, 0, compare=False)
    assert all(int(ref.meta(i)["flags"]) & A.FLAG_ROWS_OVERFLOW for i in range(n))
    assert (res["valid"] == 0).all(), res["valid"]


# ---- c. the split fetch -----------------------------------------------------------------------------------------------------------------
SPLIT_SIZES = (5, 9, 2, 12, 7)
SPLIT = {
    "ack-retry-journal": lambda: E.test_config("broadcast", bin="broadcast-ack-retry", node_count=5, rate=20, time_limit=4, latency=10, seed=P.SEED,
                                               journal_capacity=60000),
    "txn-list-append": lambda: E.test_config("txn-list-append", node_count=5, rate=60, time_limit=4, latency=5, seed=P.SEED),   # payload prefixes off 16 bytes: compact_words_kernel
    "unique-ids-1000": lambda: E.test_config("unique-ids", node_count=3, rate=1000, time_limit=2, latency=5, seed=P.SEED),       # > 1024 rows per instance: the compaction grid's second dimension
    "echo-rate-0": lambda: E.test_config("echo", node_count=3, rate=0, time_limit=2, seed=P.SEED),                               # every history empty: nothing to compact
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(SPLIT))
def test_split_fetch_returns_the_contexts_own_batch(lib, capfd, name):
    """bench.py's fetch_inclusive on two contexts: run, check, fetch_begin on one while the other's copies cross; fetch before the context
    is used again — except at step 3, where the next run is launched straight over the pending fetch."""
    cfg = SPLIT[name]()
    journal = cfg.journal_capacity > 0
    skip_fetch_before = 3
    batches = [(500 * k + 11, n) for k, n in enumerate(SPLIT_SIZES)]
    t0 = time.perf_counter()
    for first, n in batches:
        P.oracle(cfg, first, n)
    if name == "unique-ids-1000":
        assert all(int(P.oracle(cfg, f, n).meta(i)["n_rows"]) > 1024 for f, n in batches for i in range(n))
        assert sum(int(P.oracle(cfg, *batches[3]).meta(i)["n_rows"]) for i in range(12)) // 12 + 1 > 1024
    if name == "txn-list-append":
        assert any(int(P.oracle(cfg, f, n).meta(i)["n_payload_words"]) % 4 for f, n in batches for i in range(n))
    if name == "echo-rate-0":
        assert all(int(P.oracle(cfg, f, n).meta(i)["n_rows"]) == 0 for f, n in batches for i in range(n))
    ms, verified = [], []

    def fetched(e, k):
        first, n = batches[k]
        what = f"{name} step {k} (first {first}, n {n})"
        e.fetch()
        P.compare_batch(e, cfg, first, n, what, journal)
        e.fetch_begin()   # a second fetch_begin and a second fetch change nothing
        e.fetch()
        P.compare_batch(e, cfg, first, n, what + ", fetched twice", journal)
        verified.append(k)

    engs = [E.Engine(cfg) for _ in range(2)]
    try:
        holds = [None, None]
        for k, (first, n) in enumerate(batches):
            e = engs[k % 2]
            if holds[k % 2] is not None and k != skip_fetch_before:
                fetched(e, holds[k % 2])
            e.run(first, n)
            e.check()
            res = e.check_results()
            ms.append((k, n) + e.kernel_ms())
            e.fetch_begin()
            holds[k % 2] = k
            for get in (e.raw_history, e.meta, e.net_stats_raw) + ((e.raw_journal,) if journal else ()):
                with pytest.raises(E.EngineError):
                    get(0)
            e.fetch_begin()   # a second one while the first is pending
            if name == "echo-rate-0":
                assert (res["valid"] == 1).all() and len(res) == n
        for j, e in enumerate(engs):
            fetched(e, holds[j])
            P.compare_records(e, cfg, e.check_results(), f"{name} step {holds[j]}")
    finally:
        for e in engs:
            e.close()
    assert verified == [0, 2, 4, 3]   # (step 1's batch was launched over)
    per = ", ".join(f"{k}:{n}x{a:.2f}+{b:.2f}" for k, n, a, b in ms)
    with capfd.disabled():
        print(f"\n[pipeline] split fetch {name}: step:n x kernel_ms sim+check {per}; wall {time.perf_counter() - t0:.1f} s")


# ---- d. back to back, and a caller's stream ---------------------------------------------------------------------------------------------
def test_two_async_launches_back_to_back(lib, capfd):
    """No check between them: the context holds the second launch's results."""
    cfg = P.config("headline")
    n1, n2 = P.sizes("headline")[1], P.sizes("headline")[2]
    t0 = time.perf_counter()
    P.oracle(cfg, 40, n2)
    with E.Engine(cfg) as eng:
        P.launch_async(eng, capfd, 3, n1, "duo")
        P.launch_async(eng, capfd, 40, n2, "duo")
        eng.check()
        res = eng.check_results()
        sim, chk = P.finite_ms(eng, "back to back")
        eng.fetch()
        P.compare_batch(eng, cfg, 40, n2, "the second of two launches back to back")
        P.compare_records(eng, cfg, res, "the second of two launches back to back")
    with capfd.disabled():
        print(f"\n[pipeline] back to back: n {n1} then {n2}, kernel_ms sim {sim:.2f} check {chk:.2f}; wall {time.perf_counter() - t0:.1f} s")


@pytest.mark.skipif(P.EMU, reason="the emulator has no streams")
def test_async_launch_on_the_callers_stream(lib, capfd):
    """The contract of msim_run_async for a caller's stream: the caller synchronises it, then check() and fetch() see the launch."""
    torch = P.torch
    cfg = P.config("headline")
    n = P.sizes("headline")[2]
    t0 = time.perf_counter()
    P.oracle(cfg, 77, n)
    stream = torch.cuda.Stream()
    with E.Engine(cfg) as eng:
        P.launch_async(eng, capfd, 77, n, "duo", stream=stream.cuda_stream)
        stream.synchronize()
        eng.check()
        res = eng.check_results()
        sim, chk = P.finite_ms(eng, "caller's stream")
        eng.fetch()
        P.compare_batch(eng, cfg, 77, n, "a launch on the caller's stream")
        P.compare_records(eng, cfg, res, "a launch on the caller's stream")
    with capfd.disabled():
        print(f"\n[pipeline] caller's stream: n {n}, kernel_ms sim {sim:.2f} check {chk:.2f}; wall {time.perf_counter() - t0:.1f} s")
