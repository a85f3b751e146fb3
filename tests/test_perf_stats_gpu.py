"""perf_check_kernel (csrc/perf_check_dev.hip): :stats :by-f and the :perf latency records on the device, held field by field to the
host twin msim_check_perf_rows (and, for everything but the one large history, to tests/perf_ref.py as well):
  (a) Engine.check_perf on the histories of engine runs of four workloads, windows off and 1 s x 8,
  (b) called at once behind run_async on the context's stream, before check(),
  (c) synthetic histories through msim_check_perf_batch: the smallest shapes at which the kernel can go wrong — chunk edges of 64
      rows, the floor(n * q) edges, ties, saturation, open and unpaired rows, processes that move on after an :info, 1 and 128 worker
      threads, window boundaries, and one history of 65534 rows beside one of 3 (the LDS capacity and the slab stride),
  (d) once with every device buffer of the context poisoned, in a process of its own.
tests/test_perf_stats_hipemu.py runs this file on the host wavefront emulator in the CPU suite."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from maelstrom_amd import engine as E
import perf_cases as PC
import perf_ref as R

pytestmark = pytest.mark.gpu
N_INSTANCES = 64
MS = 1_000_000


# ---- (a) engine runs ----
@pytest.mark.parametrize("name", sorted(PC.CONFIGS))
def test_engine_histories(lib, name):
    cfg = PC.CONFIGS[name]()
    with E.Engine(cfg) as eng:
        eng.run(0, N_INSTANCES)
        eng.fetch()
        rows = [eng.raw_history(i)[0].copy() for i in range(N_INSTANCES)]
        for window_s, n_windows in PC.WINDOWS:
            dev = eng.check_perf(window_s, n_windows)
            assert len(dev) == N_INSTANCES
            for i in range(N_INSTANCES):
                assert dev[i] == E.check_perf_rows(rows[i], cfg.concurrency, window_s, n_windows), (name, i, n_windows)
                if n_windows:
                    R.assert_windows_sum(dev[i])
    assert sum(r["count"] for r in dev) > 10 * N_INSTANCES
    census = E.perf_census(dev)
    assert census and all(c["count"] == sum(r["by-f"][f]["latency"][t]["count"] for r in dev if f in r["by-f"]) for (f, t), c in census.items())


# ---- (b) the pipelined path ----
def test_check_perf_straight_after_run_async(lib):
    cfg = PC.CONFIGS["broadcast"]()
    with E.Engine(cfg) as blocking:
        blocking.run(0, N_INSTANCES)
        blocking.check()
        want_check = blocking.check_results()
        want = blocking.check_perf(1.0, 8)
    with E.Engine(cfg) as eng:
        eng.run_async(0, N_INSTANCES)
        got = eng.check_perf(1.0, 8)      # at once: the pass queues behind the launch on the context's stream
        eng.check()
        assert got == want
        assert eng.check_results().tobytes() == want_check.tobytes()   # the workload checker's records are what they are without the pass


# ---- (c) synthetic histories ----
def op(typ, f, process, time):
    return {"type": typ, "f": f, "process": process, "time": time}


def synth(seed, n_ops, workers, fs=(":read", ":write", ":cas"), p_fail=0.1, p_info=0.05, p_never=0.0, overtake=True, max_gap_ns=3 * MS):
    """`n_ops` operations by `workers` worker threads as [upstream] jepsen's interpreter hands them out: a thread has one operation open;
    after an :info its next process is process + workers; a thread whose operation never completes (`p_never`) is not used again.
    Completions are drawn from the open operations at random (`overtake`) or oldest first."""
    rnd = random.Random(seed)
    ops, open_ops, free = [], [], list(range(workers))
    proc_of = {w: w for w in range(workers)}
    t, left = 0, n_ops
    while left or open_ops:
        t += rnd.randrange(1, max_gap_ns)
        if free and left and (not open_ops or rnd.random() < 0.55):
            w = free.pop(rnd.randrange(len(free)))
            f = rnd.choice(fs)
            ops.append(op(":invoke", f, proc_of[w], t))
            left -= 1
            if rnd.random() >= p_never:
                open_ops.append((w, f))
            continue
        if not open_ops:
            if not free:
                break   # every thread is stuck behind an operation that never completes
            continue
        w, f = open_ops.pop(rnd.randrange(len(open_ops)) if overtake else 0)
        x = rnd.random()
        typ = ":fail" if x < p_fail else (":info" if x < p_fail + p_info else ":ok")
        ops.append(op(typ, f, proc_of[w], t))
        if typ == ":info":
            proc_of[w] += workers
        free.append(w)
    return ops


def sequential(latencies_us, f=":echo", typ=":ok", start_ns=0, gap_ns=1000, rnd=None):
    """one worker thread, one operation after the other with the given latencies (+ a remainder below a microsecond)"""
    ops, t = [], start_ns
    for l in latencies_us:
        ops.append(op(":invoke", f, 0, t))
        t += l * 1000 + (rnd.randrange(1000) if rnd else 0)
        ops.append(op(typ, f, 0, t))
        t += gap_ns
    return ops


def compare(histories, workers, window_s=None, n_windows=0, max_rows=None, ref=True):
    rows = [h if isinstance(h, np.ndarray) else R.rows_of(h) for h in histories]
    got = E.check_perf_batch(rows, workers, window_s, n_windows, max_rows=max_rows)
    assert len(got) == len(histories)
    for i, (h, r, g) in enumerate(zip(histories, rows, got)):
        assert g == E.check_perf_rows(r, workers, window_s, n_windows), (i, workers, n_windows)
        if ref and not isinstance(h, np.ndarray):
            assert g == R.perf(h, window_s, n_windows), (i, workers, n_windows)
        if n_windows:
            R.assert_windows_sum(g)
    return got


def test_empty_nemesis_only_and_single_op_histories(lib):
    nemesis = [op(":info", ":start-partition", ":nemesis", 10), op(":info", ":stop-partition", ":nemesis", 20)]
    one = [op(":invoke", ":echo", 0, 1000), op(":ok", ":echo", 0, 3500)]
    for window_s, n_windows in ((None, 0), (1.0, 1), (0.001, 16)):
        got = compare([[], nemesis, one, nemesis + one], 3, window_s, n_windows)
        assert got[0] == got[1] and got[0]["count"] == 0 and got[0]["valid?"] is True
        assert got[2] == got[3] and got[2]["by-f"][":echo"]["latency"][":ok"] == {"count": 1, "sum-us": 2, "quantiles-us": {q: 2 for q in R.QUANTILES}}


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_completions_that_fill_a_chunk_of_rows_exactly(lib, n):
    for workers in (1, 5):   # one thread: every completion next to its invocation; five: pairs that straddle the chunks
        hs = [synth(1000 + n + s, n, workers, p_fail=0.1 * s, p_info=0.05 * s) for s in range(3)]
        got = compare(hs, workers, 0.05, 8)
        assert all(g["count"] == n and g["open-count"] == 0 for g in got)


@pytest.mark.parametrize("n", [1, 2, 20, 100, 101, 200])
def test_one_group_of_n_samples(lib, n):
    """the floor(n * q) edges: 0.95 * 20 = 19 exactly, 0.99 * 100 = 99, 0.99 * 101 = 99.99, 0.95 * 200 = 190 (and the serial / wavefront selection on either side of 128)"""
    rnd = random.Random(n)
    distinct = list(range(10, 10 + n)); rnd.shuffle(distinct)
    hs = [sequential(distinct, rnd=rnd), sequential([rnd.randrange(1, 5000) for _ in range(n)], rnd=rnd),
          sequential([7] * n), sequential([rnd.choice((3, 4)) for _ in range(n)])]
    got = compare(hs, 1, 0.01, 4)
    asc = sorted(distinct)
    assert got[0]["by-f"][":echo"]["latency"][":ok"]["quantiles-us"] == {q: asc[min(n - 1, int(n * q))] for q in R.QUANTILES}
    assert got[2]["by-f"][":echo"]["latency"][":ok"] == {"count": n, "sum-us": 7 * n, "quantiles-us": {q: 7 for q in R.QUANTILES}}


def test_latencies_tied_around_the_quantile_indices(lib):
    # 100 and 200 samples: the median index 50 / 100 is the first, the last, or inside a run of equal values; likewise 0.95 and 0.99
    hs = []
    for n in (100, 200):
        h = n // 2
        for lat in ([10] * h + [20] * (n - h), [10] * (h + 1) + [20] * (n - h - 1), [10] * (h - 1) + [15, 15, 15] + [20] * (n - h - 2),
                    [5] * (n * 95 // 100) + [9] * (n - n * 95 // 100), [5] * (n * 95 // 100 + 1) + [9] * (n - n * 95 // 100 - 1),
                    [5] * (n * 99 // 100) + [9] * (n - n * 99 // 100), [5] * (n - 1) + [4_000_000_000]):
            random.Random(n).shuffle(lat)
            hs.append(sequential(lat))
    compare(hs, 1)
    compare(hs, 1, 0.002, 16)


def test_saturation_open_and_unpaired_rows(lib):
    h = [op(":ok", ":echo", 1, 500),                                                             # a completion before any invocation
         op(":invoke", ":echo", 0, 1_000_000_123), op(":info", ":echo", 0, 6_000_000_999),       # 5 s: more than 2^32 ns
         op(":invoke", ":echo", 2, 8_000_000_000), op(":invoke", ":echo", 4, 8_000_000_500),     # process 4 = thread 1: never completes
         op(":ok", ":echo", 2, 8_000_000_000 + 80 * 60 * 10**9),                                 # 80 min: saturates at 2^32 - 1 us
         op(":invoke", ":echo", 3, 5_000_000_000_000), op(":fail", ":echo", 3, 5_000_000_000_999)]   # process 3 after the :info of 0
    for window_s, n_windows in ((None, 0), (5.0, 2), (1.0, 16)):
        got = compare([h, h[1:], h[:5]], 3, window_s, n_windows)
        e = got[0]["by-f"][":echo"]
        assert e["unpaired"] == 1 and got[0]["open-count"] == 1 and got[0]["count"] == 4
        assert e["latency"][":info"]["quantiles-us"][0.5] == 5_000_000 and e["latency"][":ok"]["quantiles-us"][1] == 0xFFFFFFFF
        assert got[2]["open-count"] == 2 and got[1]["by-f"][":echo"]["unpaired"] == 0
    h = synth(77, 300, 6, p_never=0.02, p_info=0.2)   # processes move on after :info; some threads get stuck
    got = compare([h], 6, 0.1, 8)
    assert got[0]["open-count"] > 0 and got[0]["info-count"] > 20 and max(o["process"] for o in h) >= 12


@pytest.mark.parametrize("workers", [1, 128])
def test_one_and_128_worker_threads(lib, workers):
    hs = [synth(500 + s, 400, workers, p_info=0.1, overtake=bool(s)) for s in range(3)]
    got = compare(hs, workers, 0.2, 8)
    assert all(g["count"] == 400 for g in got)
    if workers == 128:   # completions overtake one another: a block of invocations, completed in reverse
        h = [op(":invoke", ":add", p, 1000 * p) for p in range(128)] + [op(":ok", ":add", p, MS + 777 * (128 - p)) for p in reversed(range(128))]
        assert compare([h], 128)[0]["by-f"][":add"]["latency"][":ok"]["count"] == 128


def test_window_boundaries_and_ops_beyond_the_last_window(lib):
    w = 250 * MS
    starts = [0, w - 1, w, w + 1, 2 * w - 1, 2 * w, 7 * w, 8 * w - 1, 8 * w, 100 * w]   # on, just before and after boundaries; far beyond
    h = [op(":invoke", ":write", k, t0) for k, t0 in enumerate(starts)] + [op(":ok", ":write", k, 101 * w + 1000 * k) for k in range(10)]
    long_op = [op(":invoke", ":read", 0, w - 5), op(":ok", ":read", 0, 3 * w)]   # the window is the invocation's
    for n_windows in (1, 2, 8, 16):
        got = compare([h, long_op], 10, 0.25, n_windows)
        counts = [x[":write"][":ok"]["count"] for x in got[0]["windows"]]
        assert counts == {1: [10], 2: [2, 8], 8: [2, 3, 1, 0, 0, 0, 0, 4], 16: [2, 3, 1, 0, 0, 0, 0, 2, 1] + [0] * 6 + [1]}[n_windows]
        assert [x[":read"][":ok"]["count"] for x in got[1]["windows"]][0] == 1


def large_history(n_ops=32767, workers=128, seed=9):
    """65534 rows = 32767 paired operations (the most a device checker accepts): blocks of `workers` invocations, completed in a random
    order; three :f, all three completion types; as rows (built with numpy)"""
    rnd = np.random.default_rng(seed)
    rows = np.zeros(2 * n_ops, dtype=E.OP_DT)
    t, at, proc = 0, 0, np.arange(workers)
    for first in range(0, n_ops, workers):
        k = min(workers, n_ops - first)
        f = rnd.choice([2, 6, 7], size=k)
        typ = rnd.choice([1, 1, 1, 2, 3], size=k)
        ti = t + np.cumsum(rnd.integers(1, 50_000, size=k))
        order = rnd.permutation(k)
        tc = ti[-1] + np.cumsum(rnd.integers(1, 900_000, size=k))
        rows["time_len"][at:at + k] = ti
        rows["packed"][at:at + k] = (f << 2) | (proc[:k] << 12)
        rows["time_len"][at + k:at + 2 * k] = tc
        rows["packed"][at + k:at + 2 * k] = typ[order] | (f[order] << 2) | (proc[:k][order] << 12)
        proc[:k][typ == 3] += workers   # after an :info the thread's next process
        t, at = int(tc[-1]), at + 2 * k
    return rows


def test_a_history_at_the_row_limit_beside_one_of_three_rows(lib):
    big = large_history()
    small = [op(":invoke", ":read", 5, 10), op(":info", ":start-partition", ":nemesis", 20), op(":ok", ":read", 5, 9010)]
    assert len(big) == 65534
    for window_s, n_windows in ((None, 0), (0.5, 16)):
        got = compare([big, R.rows_of(small), big[:4001]], 128, window_s, n_windows, max_rows=65534)
        assert got[0]["count"] == 32767 and got[0]["open-count"] == 0 and sum(fs["unpaired"] for fs in got[0]["by-f"].values()) == 0
        assert got[1] == R.perf(small, window_s, n_windows)


def test_random_shapes(lib):
    rnd = random.Random(2026)
    for k in range(40):
        workers = rnd.choice([1, 2, 3, 5, 8, 13, 25, 60, 128])
        fs = rnd.choice([(":echo",), (":read", ":write", ":cas"), (":send", ":poll", ":assign", ":crash"), (":broadcast", ":read"), (0, 5, 9, 13, 31)])
        h = synth(7000 + k, rnd.randrange(1, 700), workers, fs=fs, p_fail=rnd.choice([0.0, 0.05, 0.5]), p_info=rnd.choice([0.0, 0.05, 0.3]),
                  p_never=rnd.choice([0.0, 0.0, 0.01]), overtake=rnd.random() < 0.7, max_gap_ns=rnd.choice([2000, 3 * MS, 200 * MS]))
        n_windows = rnd.choice([0, 1, 3, 8, 16])
        compare([h], workers, rnd.choice([0.001, 0.05, 1.0]) if n_windows else None, n_windows)


# ---- (d) poisoned buffers ----
def poisoned_run():
    """under MSIM_POISON (read once per process): two runs on one context — the second launch poisons the perf pass's own cached block too"""
    cfg = PC.CONFIGS["raft-partitions"]()
    with E.Engine(cfg) as eng:
        for first in (0, 8):
            eng.run(first, 8)
            dev = eng.check_perf(1.0, 8)
            eng.fetch()
            for i in range(8):
                assert dev[i] == E.check_perf_rows(eng.raw_history(i)[0], cfg.concurrency, 1.0, 8), (first, i)
    print("poisoned: OK")


def test_records_do_not_depend_on_what_the_buffers_held(lib):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "poisoned"], cwd=ROOT, env=dict(os.environ, MSIM_POISON="0xA5"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poisoned: OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    assert sys.argv[1:] == ["poisoned"] and os.environ.get("MSIM_POISON")
    poisoned_run()
