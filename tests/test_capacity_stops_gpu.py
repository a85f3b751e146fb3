"""Capacity stops in every kernel layout, and the checkers behind them, in launches where flagged and unflagged
clusters sit side by side: the engine against the oracle run at the same lowered capacity (tests/capacity_stop_cases.py derives the
capacity from an ample oracle run, and asserts on the oracle alone that the first lane group mixes).

What is pinned, per instance:
  * flags bitwise the oracle's; n_rows <= max_rows, n_payload_words <= max_payload_words; every row's payload slice inside the payload written;
  * an unflagged instance — a live cluster beside stopped ones in its wavefront — is the oracle's in full (rows, payload, counts, rounds,
    events, net stats: what test_parity_gpu._compare compares);
  * a rows stop keeps whole rounds: the engine's rows are a byte prefix of the capped oracle's (which drops row by row and runs on to
    max_rows), and short of max_rows by less than one round's rows (two nemesis rows, an invocation and a completion per worker);
  * a payload stop equals the capped oracle's rows and payload in full, except where the case table gives the reason it does not (kafka);
  * a values stop: the flags and bounds, and for the broadcast / g-set kernels the rows prefix.
And the checkers on the same launches: the device records equal the host records, a flagged history is never valid, an unflagged one's
record is the one it has in the ample-capacity launch; the availability checker on one echo and one lin-kv launch.

tests/test_capacity_stops_hipemu.py runs this file on the host emulator."""
import re

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import capacity_stop_cases as K

pytestmark = pytest.mark.gpu

CASES = K.cases()
_RUNS = {}
_AMPLE_RECORDS = {}


class _Run:
    pass


def _layout(err):
    return re.findall(r"\[layout\] (\S+) (\d+)", err)


def _run(case, capfd):
    """One engine launch of the case at the lowered capacity (kept for the tests that share it): histories, metas, net stats, and the
    checker's records from the device and from the host."""
    cid, sid, cap, flags, kernel = case
    if cid in _RUNS:
        return _RUNS[cid]
    cfg, ora, value = K.capped(sid, cap)
    n = ora.n
    r = _Run()
    r.cfg, r.ora, r.n = cfg, ora, n
    capfd.readouterr()
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags | 0x1000)
        eng.run(0, n)
        r.layout = _layout(capfd.readouterr().err)
        r.records = {}
        if cap != "values":
            # list-append and unique-ids: both device kernels (bit 13: the HBM-table ones)
            both = cfg.workload in (A.WL_TXN_LIST_APPEND, A.WL_UNIQUE_IDS)
            for name, fl in (("device", 0), ("device-hbm", 0x2000), ("host", 0x800)):
                if name == "device-hbm" and not both:
                    continue
                eng.set_dev_flags(flags | fl)
                eng.check()
                r.records[name] = eng.check_results()
            r.host_rechecks = eng.check_host_rechecks() if cfg.workload == A.WL_LIN_KV else 0
            if cid in AVAILABILITY_CASES:
                r.availability = {a: eng.check_availability(a) for a in (None, "total", 0.9)}
        eng.fetch()
        r.meta = [eng.meta(i) for i in range(n)]
        r.hist = [tuple(x.copy() for x in eng.raw_history(i)) for i in range(n)]
        r.stats = [tuple(int(getattr(eng.net_stats_raw(i), f)) for f, _ in A.NetStats._fields_) for i in range(n)]
    _RUNS[cid] = r
    return r


def _ample_records(sid, flags):
    """the device checker's records of the shape's ample-capacity launch in the same layout"""
    if (sid, flags) not in _AMPLE_RECORDS:
        cfg, ora = K.ample(sid)
        with E.Engine(cfg) as eng:
            eng.set_dev_flags(flags)
            eng.run(0, ora.n)
            eng.check()
            rec = eng.check_results()
            eng.fetch()
            assert all(eng.meta(i).flags == 0 for i in range(ora.n))
        _AMPLE_RECORDS[(sid, flags)] = rec
    return _AMPLE_RECORDS[(sid, flags)]


AVAILABILITY_CASES = ("echo-rows-packed", "raft4-rows-packed")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stop_beside_running_clusters_equals_the_oracle(lib, capfd, case):
    """(The flags of a rows stop: the oracle runs on after it, the kernels do not.  txn-rw-register's transaction table, max_rows / 2
    entries, fills up around the same time: the oracle mirrors that engine capacity, ARENA_OVERRUN, up to the end of the round whose rows
    did not fit and not in later rounds — hatg's instance 5 meets the 411th request one round after the stop and ends 0x1 on both sides,
    instances 2, 3, 4 and 7 meet it in the stop round and end 0x41.)"""
    cid, sid, cap, flags, kernel = case
    r = _run(case, capfd)
    cfg, ora, n = r.cfg, r.ora, r.n
    assert r.layout == [(kernel, str(n))], f"the launch took {r.layout}, not {kernel}"
    stopped, flag_diffs = 0, []
    for i in range(n):
        m, om = r.meta[i], ora.meta[i]
        rows, pay = r.hist[i]
        orows, opay = ora.history(i)
        print(f"{cid}[{i}]: flags {m.flags:#x}/{int(om['flags']):#x} rows {m.n_rows}/{int(om['n_rows'])} of {cfg.max_rows} payload {m.n_payload_words}/{int(om['n_payload_words'])} "
              f"of {cfg.max_payload_words} rounds {m.n_rounds}/{int(om['n_rounds'])}")
        if m.flags != int(om["flags"]):   # (asserted after the loop, so that every instance is looked at in full)
            flag_diffs.append(f"instance {i}: engine {m.flags:#x} oracle {int(om['flags']):#x}")
        assert m.n_rows <= cfg.max_rows and m.n_payload_words <= cfg.max_payload_words, f"instance {i} counts past a capacity"
        assert len(rows) == m.n_rows and len(pay) == m.n_payload_words
        ln = (rows["time_len"] >> np.uint64(48)).astype(np.int64)
        off = rows["value"].astype(np.int64)[ln > 0]
        assert (off + ln[ln > 0] <= m.n_payload_words).all(), f"instance {i}: a row's payload slice ends past the {m.n_payload_words} words written"
        if m.flags == 0:   # a live cluster beside stopped ones: the oracle's in full
            assert (m.n_rows, m.n_payload_words, m.n_rounds, m.n_events) == (om["n_rows"], om["n_payload_words"], om["n_rounds"], om["n_events"]), f"meta differs for unflagged instance {i}"
            assert rows.tobytes() == orows.tobytes(), f"history rows differ for unflagged instance {i}"
            assert pay.tobytes() == opay.tobytes(), f"payload differs for unflagged instance {i}"
            assert r.stats[i] == tuple(int(x) for x in ora.stats[i]), f"net stats differ for unflagged instance {i}"
            continue
        stopped += 1
        prefix = rows.tobytes() == orows[:m.n_rows].tobytes() and m.n_rows <= int(om["n_rows"])
        if m.flags & A.FLAG_ROWS_OVERFLOW:
            assert int(om["n_rows"]) == cfg.max_rows
            assert prefix, f"instance {i}: the engine's {m.n_rows} rows are no prefix of the oracle's"
            assert cfg.max_rows - m.n_rows < 2 + 2 * K.workers(cfg), f"instance {i} stopped early: {m.n_rows} rows of {cfg.max_rows}"
        if m.flags & A.FLAG_PAYLOAD_OVERFLOW and K.SHAPE[sid].get("payload_exact", True):
            assert (m.n_rows, m.n_payload_words) == (om["n_rows"], om["n_payload_words"]), f"counts differ for instance {i} at its payload stop"
            assert rows.tobytes() == orows.tobytes(), f"history rows differ for instance {i} at its payload stop"
            assert pay.tobytes() == opay.tobytes(), f"payload differs for instance {i} at its payload stop"
        if m.flags & A.FLAG_VALUES_OVERFLOW and cfg.workload in (A.WL_BROADCAST, A.WL_G_SET):
            assert prefix, f"instance {i}: the engine's {m.n_rows} rows are no prefix of the oracle's"
    assert 0 < stopped < n or cap == "values"
    assert not flag_diffs, f"flags differ: {flag_diffs}"


def _same_records(cfg, dev, host, i):
    if cfg.workload != A.WL_TXN_RW_REGISTER:
        return dev[i].tobytes() == host[i].tobytes()
    # txn-rw-register: allowed cycle classes are not searched on the device — what tests/test_rw_check_gpu.py compares
    return (int(dev[i]["valid"]), int(dev[i]["ok_count"]), int(dev[i]["attempt_count"])) == (int(host[i]["valid"]), int(host[i]["ok_count"]), int(host[i]["attempt_count"])) \
        and int(dev[i]["error_count"]) & ~int(host[i]["error_count"]) == 0


CHECKED = [c for c in CASES if c[2] != "values"]


@pytest.mark.parametrize("case", CHECKED, ids=[c[0] for c in CHECKED])
def test_checkers_on_truncated_and_whole_histories_side_by_side(lib, capfd, case):
    cid, sid, cap, flags, kernel = case
    r = _run(case, capfd)
    cfg, n = r.cfg, r.n
    ample = _ample_records(sid, flags)
    host = r.records["host"]
    assert len(host) == n
    for name, dev in r.records.items():
        assert len(dev) == n
        for i in range(n):
            assert _same_records(cfg, dev, host, i), f"{name} record of instance {i} differs from the host's: {dev[i]} / {host[i]}"
            if r.meta[i].flags:
                assert int(dev[i]["valid"]) == 0, f"{name}: truncated history {i} (flags {r.meta[i].flags:#x}) is reported {int(dev[i]['valid'])}"
            elif name != "host" or cfg.workload != A.WL_TXN_RW_REGISTER:
                assert dev[i].tobytes() == ample[i].tobytes(), f"{name} record of unflagged instance {i} is not its ample-capacity record: {dev[i]} / {ample[i]}"
    if cid in AVAILABILITY_CASES:
        for a, got in r.availability.items():
            for i in range(n):
                assert got[i] == E.check_availability_rows(r.hist[i][0], a), f"availability {a!r} of instance {i}"
