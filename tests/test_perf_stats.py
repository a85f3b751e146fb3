"""[upstream] jepsen.checker/stats :by-f and the :perf latency records on the host (msim_check_perf_rows: the twin the device kernel is
held to in the GPU tier) against tests/perf_ref.py, the plain-Python restatement of their definitions: on oracle histories of four
workloads, windows off and 1 s x 8, and on hand-made histories for the verdicts and the edges."""
import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import oracle_lib as O
import perf_cases as PC
import perf_ref as R


def op(typ, f, process, time):
    return {"type": typ, "f": f, "process": process, "time": time}


def both(history, concurrency, window_s=None, n_windows=0):
    got = E.check_perf_rows(R.rows_of(history), concurrency, window_s, n_windows)
    assert got == R.perf(history, window_s, n_windows)
    if n_windows:
        R.assert_windows_sum(got)
    return got


@pytest.mark.parametrize("name", sorted(PC.CONFIGS))
def test_oracle_histories(name):
    cfg = PC.CONFIGS[name]()
    ora = O.run(cfg, 0, 3)
    seen = {"types": set(), "fs": set()}
    for i in range(3):
        rows, pay = ora.history(i)
        hist = E.decode_history(rows, pay, cfg.n_nodes, cfg.workload)
        for window_s, n_windows in PC.WINDOWS:
            got = E.check_perf_rows(rows, cfg.concurrency, window_s, n_windows)
            assert got == R.perf(hist, window_s, n_windows), (name, i, n_windows)
            if n_windows:
                R.assert_windows_sum(got)
        assert got["count"] >= 10
        for f, fs in got["by-f"].items():
            seen["fs"].add(f)
            seen["types"] |= {t for t in R.TYPES if fs["latency"][t]["count"]}
    if name == "echo-lossy":
        assert ":info" in seen["types"]
    if name == "raft-partitions":
        assert seen["fs"] == {":read", ":write", ":cas"} and {":fail", ":info"} <= seen["types"]
    if name == "kafka":
        assert ":crash" in seen["fs"] and len(seen["fs"]) == 4


def test_a_cas_that_never_succeeds_makes_stats_invalid():
    h, t = [], 0
    for k in range(6):
        f = (":read", ":write", ":cas")[k % 3]
        t += 1_000_000; h.append(op(":invoke", f, k % 2, t))
        t += 2_000_000; h.append(op(":fail" if f == ":cas" else ":ok", f, k % 2, t))
    got = both(h, 2)
    assert got["valid?"] is False and got["count"] == 6 and got["fail-count"] == 2
    assert [got["by-f"][f]["valid?"] for f in (":read", ":write", ":cas")] == [True, True, False]
    assert got["by-f"][":cas"]["latency"][":fail"] == {"count": 2, "sum-us": 4000, "quantiles-us": {q: 2000 for q in R.QUANTILES}}


def test_kafka_crashes_are_forgiven():
    h = [op(":invoke", ":send", 0, 1000), op(":ok", ":send", 0, 5000), op(":invoke", ":crash", 1, 6000), op(":info", ":crash", 1, 9000),
         op(":invoke", ":poll", 0, 10_000), op(":ok", ":poll", 0, 12_000), op(":invoke", ":crash", 3, 13_000), op(":info", ":crash", 3, 14_000)]
    got = both(h, 2)
    assert got["valid?"] is True and got["by-f"][":crash"]["valid?"] is False and got["by-f"][":crash"]["info-count"] == 2


def test_stats_map_of_an_all_ok_echo_history_has_the_documented_shape():
    h = []
    for k in range(12):
        h += [op(":invoke", ":echo", k % 3, 1000 * k), op(":ok", ":echo", k % 3, 1000 * k + 500)]
    h.insert(5, op(":info", ":start-partition", ":nemesis", 4999))   # nemesis rows are ignored
    stats = E.stats_map(both(h, 3))
    assert stats == {"valid?": True, "count": 12, "ok-count": 12, "fail-count": 0, "info-count": 0,
                     "by-f": {":echo": {"valid?": True, "count": 12, "ok-count": 12, "fail-count": 0, "info-count": 0}}}
    assert list(stats) == ["valid?", "count", "ok-count", "fail-count", "info-count", "by-f"]


def test_empty_history_and_one_of_nemesis_rows_only():
    empty = {"valid?": True, "count": 0, "ok-count": 0, "fail-count": 0, "info-count": 0, "open-count": 0, "complete?": True, "by-f": {}}
    assert E.check_perf_rows(np.zeros(0, dtype=E.OP_DT), 1) == empty
    assert both([op(":info", ":start-partition", ":nemesis", 5), op(":info", ":stop-partition", ":nemesis", 9)], 4) == empty
    assert both([], 4, 1.0, 2)["windows"] == [{}, {}]


def test_five_distinct_f_set_the_incomplete_flag():
    h = []
    for k, f in enumerate((":echo", ":read", ":add", ":write", ":cas")):
        h += [op(":invoke", f, 0, 1000 * k), op(":ok" if k else ":fail", f, 0, 1000 * k + 400)]
    got = both(h, 1)
    assert got["complete?"] is False and list(got["by-f"]) == [":echo", ":read", ":add", ":write"] and got["count"] == 5
    assert got["valid?"] is False   # :echo never succeeded
    h[-1]["type"] = ":fail"; h[1]["type"] = ":ok"   # ... now only the :f beyond the four slots never does: the verdict covers it too
    assert both(h, 1)["valid?"] is False


def test_a_latency_beyond_2_to_the_32_ns_and_one_beyond_2_to_the_32_us():
    h = [op(":invoke", ":echo", 0, 1_000_000_123), op(":info", ":echo", 0, 6_000_000_999),      # 5 s
         op(":invoke", ":echo", 1, 7_000_000_000), op(":ok", ":echo", 4, 7_000_001_000),        # no invocation of process 4
         op(":invoke", ":echo", 2, 8_000_000_000), op(":ok", ":echo", 2, 8_000_000_000 + 80 * 60 * 10**9)]   # 80 min: saturates
    got = both(h, 3, 5.0, 2)
    e = got["by-f"][":echo"]
    assert e["latency"][":info"]["quantiles-us"][1] == 5_000_000 and e["latency"][":ok"]["quantiles-us"][1] == 0xFFFFFFFF
    assert e["unpaired"] == 1 and got["open-count"] == 1 and got["count"] == 3
    assert got["windows"][0][":echo"][":info"]["count"] == 1 and got["windows"][1][":echo"][":ok"]["count"] == 1


def test_bad_arguments_are_rejected():
    rows = R.rows_of([op(":invoke", ":echo", 0, 1), op(":ok", ":echo", 0, 2)])
    with pytest.raises(E.EngineError):
        E.check_perf_rows(rows, 0)                 # no worker thread
    with pytest.raises(E.EngineError):
        E.check_perf_rows(rows, 1, 1.0, 17)        # more than MSIM_PERF_MAX_WINDOWS
    with pytest.raises(E.EngineError):
        E.check_perf_rows(rows, 1, None, 4)        # windows without a width
    lib, out, win = A.load(), np.zeros(1, dtype=E.PERF_DT), np.zeros((4, 4, 3), dtype=E.LATENCY_DT)
    assert lib.msim_check_perf_rows(rows.ctypes.data, 2, 1, 0, 4, out.ctypes.data, win.ctypes.data) == A.E_INVALID
    assert lib.msim_check_perf_rows(rows.ctypes.data, 2, 1, 1000, 17, out.ctypes.data, win.ctypes.data) == A.E_INVALID
    assert lib.msim_check_perf_rows(None, 2, 1, 0, 0, out.ctypes.data, None) == A.E_INVALID
    assert lib.msim_check_perf_rows(rows.ctypes.data, 2, 1, 0, 0, None, None) == A.E_INVALID
    assert lib.msim_check_perf_rows(rows.ctypes.data, 2, 1, 0, 4, out.ctypes.data, None) == A.OK   # no window buffer: whole-history records only
