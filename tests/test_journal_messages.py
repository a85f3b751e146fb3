"""The net journal's messages on the host (msim_journal_messages_rows, csrc/journal.cpp; the contract: include/maelsim_journal.h)
against tests/journal_ref.py — the contract restated in pure Python — on the journals of tests/journal_cases.py, and on journals of
the CPU oracle against the counters the oracle keeps while it runs.  Needs no device; tests/test_journal_messages_gpu.py holds the
device entries against this host entry byte for byte."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import journal_cases as K
import journal_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5A5A5A5
CASES = K.all_cases()

# the configurations whose journals the oracle writes: name -> (options, instances)
ACK_RETRY = dict(workload="broadcast", bin="broadcast-ack-retry", node_count=5, topology="tree4", rate=10, time_limit=20, nemesis=["partition"], nemesis_interval=5,
                 latency=10, seed=13)
ORACLE = {"ack-retry": (ACK_RETRY, 4),
          "echo": (dict(workload="echo", node_count=2, rate=10, time_limit=10, seed=3), 2),
          "lin-kv proxy": (dict(workload="lin-kv", bin="lin-kv-proxy", node_count=3, rate=10, time_limit=10, seed=4), 2),
          "broadcast": (dict(workload="broadcast", node_count=5, rate=10, time_limit=10, seed=5), 2)}


def host(events, cap, n_nodes=K.N, slots=K.SLOTS):
    """the host entry over poisoned arrays -> (summary, the whole slab of `cap` records): the entry clears what it does not write"""
    events = np.ascontiguousarray(events)
    summ = np.full(E.JOURNAL_SUMMARY_DT.itemsize // 4, POISON, dtype=np.uint32).view(E.JOURNAL_SUMMARY_DT)
    slab = np.full(max(cap, 1) * 8, POISON, dtype=np.uint32).view(E.JOURNAL_MSG_DT)
    rc = A.load().msim_journal_messages_rows(events.ctypes.data, len(events), n_nodes, slots, summ.ctypes.data, slab.ctypes.data if cap else None, cap)
    assert rc == 0, rc
    return summ[0], slab[:cap]


_oracle_runs = {}


def oracle_journals(name, capacity=100000):
    """-> (cfg, the oracle's run) of one of ORACLE, made once"""
    if (name, capacity) not in _oracle_runs:
        kw, n = ORACLE[name]
        cfg = E.test_config(**kw, journal_capacity=capacity)
        _oracle_runs[name, capacity] = (cfg, O.run(cfg, 0, n))
    return _oracle_runs[name, capacity]


def slots_of(cfg):
    return max(cfg.concurrency, cfg.n_nodes)


@pytest.mark.parametrize("name", list(CASES))
def test_host_entry_equals_the_restatement(lib, name):
    events, handed = CASES[name]
    n_msgs = R.messages(events, K.N, K.SLOTS)[0]["n_msgs"]
    roomy = None
    for cap in sorted({n_msgs + 3, 0, 1, max(n_msgs - 1, 0)}, reverse=True):
        got, want = host(events, cap), R.packed(events, K.N, K.SLOTS, cap)
        assert got[0].tobytes() == want[0].tobytes(), (name, cap, got[0], want[0])
        assert got[1].tobytes() == want[1].tobytes(), (name, cap)
        assert int(got[0]["valid"]) == 1 - handed
        assert bool(int(got[0]["flags"]) & A.JOURNAL_TABLE_TRUNCATED) == (n_msgs > cap)
        # the capacity changes the flag and nothing else of the summary
        plain = got[0].copy()
        plain["flags"] = 0
        roomy = plain.tobytes() if roomy is None else roomy
        assert plain.tobytes() == roomy, (name, cap)


def test_what_the_cases_cover():
    w = K.W
    lens = {len(v[0]) for v in K.well_formed().values()}
    assert {0, 1, 2, w - 1, w, w + 1, 2 * w + 1} <= lens
    counts = {int(host(v[0], 0)[0]["latency"][c]["count"]) for v in K.well_formed().values() for c in (0, 1)}
    assert {0, 1, 2, 20, 100, 101, 200} <= counts
    bad = [host(v[0], 0)[0] for v in K.malformed().values()]
    assert all(int(s["valid"]) == 0 for s in bad)
    assert any(int(s["dup_sends"]) for s in bad) and any(int(s["orphan_recvs"]) for s in bad) and any(int(s["extra_recvs"]) for s in bad)
    assert any(not (int(s["dup_sends"]) or int(s["orphan_recvs"]) or int(s["extra_recvs"])) for s in bad)   # an id beyond the events alone
    s = host(K.well_formed()["endpoints 0 and 255"][0], 0)[0]
    assert int(s["endpoints"][0]) & 1 and int(s["endpoints"][7]) >> 31 and E.journal_analysis(s)["delivery"]["endpoints"] == ["c2", "n0", "service0", "service249"]
    s, m = E.journal_messages_history(K.well_formed()["times near 2^32"][0], K.N, K.SLOTS)
    assert int(m["send_time_us"].min()) >= 0xFFFFFF00 and int(s["latency"][1]["q_us"][4]) == 0x80 + 2 * 39
    s, m = E.journal_messages_history(K.well_formed()["a recv timed before its send"][0], K.N, K.SLOTS)
    assert [int(x) for x in m["latency_us"]] == [0, 0]


def test_python_entries(lib):
    events = CASES["2W + 1 events"][0]
    s, m = E.journal_messages_history(events, K.N, K.SLOTS)
    assert len(m) == int(s["n_msgs"]) == int(s["send_count"][0]) and m.dtype == E.JOURNAL_MSG_DT and s.dtype == E.JOURNAL_SUMMARY_DT
    s2, m2 = E.journal_messages_history(events, K.N, K.SLOTS, max_msgs=5)
    assert len(m2) == 5 and m2.tobytes() == m[:5].tobytes() and int(s2["flags"]) == A.JOURNAL_TABLE_TRUNCATED
    an = E.journal_analysis(s, m)
    assert an["valid?"] is True and set(an) == {"all", "clients", "servers", "delivery", "valid?"}
    assert an["all"] == {"send-count": int(s["send_count"][0]), "recv-count": int(s["recv_count"][0]), "msg-count": int(s["msg_count"][0])}
    d = an["delivery"]
    assert d["undelivered"]["all"] == len(d["undelivered-ids"]) == int((m["recv_event"] == A.NO_VALUE).sum()) > 0
    assert d["latency"]["servers"]["quantiles-us"][0.5] == int(s["latency"][1]["q_us"][1]) and d["endpoints"] == ["c0", "c1", "c2", "n0", "n1", "n2"]
    assert E.journal_analysis(host(CASES["a double recv"][0], 0)[0])["delivery"]["extra-recvs"] == 1


def test_null_arguments(lib):
    L = A.load()
    ev = np.ascontiguousarray(CASES["W events"][0])
    summ, recs = np.zeros(1, dtype=E.JOURNAL_SUMMARY_DT), np.zeros(4, dtype=E.JOURNAL_MSG_DT)
    assert L.msim_journal_messages_rows(ev.ctypes.data, len(ev), 3, 3, summ.ctypes.data, None, 0) == 0 and int(summ[0]["flags"]) == A.JOURNAL_TABLE_TRUNCATED
    assert L.msim_journal_messages_rows(ev.ctypes.data, len(ev), 3, 3, summ.ctypes.data, None, 1) == A.E_INVALID
    assert L.msim_journal_messages_rows(ev.ctypes.data, len(ev), 3, 3, None, recs.ctypes.data, 4) == A.E_INVALID
    assert L.msim_journal_messages_rows(None, 1, 3, 3, summ.ctypes.data, recs.ctypes.data, 4) == A.E_INVALID
    assert L.msim_journal_messages_rows(None, 0, 3, 3, summ.ctypes.data, recs.ctypes.data, 4) == 0 and int(summ[0]["valid"]) == 1
    off = np.zeros(2, dtype=np.uint64)
    assert L.msim_journal_messages_batch(0, None, None, 1, 3, 3, summ.ctypes.data, None, 0, None) == A.E_INVALID
    assert L.msim_journal_messages_batch(0, None, off.ctypes.data, 0, 3, 3, summ.ctypes.data, None, 0, None) == A.E_INVALID
    assert L.msim_journal_messages_batch(0, None, off.ctypes.data, 1, 3, 3, None, None, 0, None) == A.E_INVALID
    assert L.msim_journal_messages_batch(0, None, off.ctypes.data, 1, 3, 3, summ.ctypes.data, None, 2, None) == A.E_INVALID
    assert L.msim_journal_messages(None, summ.ctypes.data, None, 0, 1) == A.E_INVALID


def test_abi(lib):
    """the records and entries against include/maelsim_journal.h (which maelsim.h includes): arity by the declarations, as
    tests/test_abi_tables.py does for maelsim.h's own"""
    header = open(os.path.join(ROOT, "include", "maelsim_journal.h")).read()
    assert '#include "maelsim_journal.h"' in open(os.path.join(ROOT, "include", "maelsim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = {name: params.split(",") for name, params in re.findall(r"^int\s*(msim_[a-z0-9_]+)\(([^)]*)\);", text, re.M)}
    assert list(decls) == list(A.JOURNAL_PROTOTYPES) and len(decls) == 4
    for name, params in decls.items():
        restype, argtypes = A.JOURNAL_PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(params), name
        for t, p in zip(argtypes, params):
            assert ("*" in p) == (t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)), (name, p)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == list(argtypes), name
    assert set(re.findall(r"^\}\s*(msim_[a-z0-9_]+);", header, re.M)) == set(A.JOURNAL_RECORDS)
    assert [np.dtype(s).itemsize for s in A.JOURNAL_RECORDS.values()] == [32, 192] and E.JOURNAL_SUMMARY_DT.itemsize % 16 == 0
    flags = dict(re.findall(r"#define (MSIM_JOURNAL_[A-Z_]+) (\d+)u", header))
    assert (int(flags["MSIM_JOURNAL_TRUNCATED"]), int(flags["MSIM_JOURNAL_TABLE_TRUNCATED"])) == (A.JOURNAL_TRUNCATED, A.JOURNAL_TABLE_TRUNCATED)
    unit = open(os.path.join(ROOT, "maelstrom_amd", "csrc", "journal_dev.hip")).read()
    assert int(re.search(r"constexpr u32 JWG = (\d+);", unit).group(1)) == A.JOURNAL_WG


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_records_match_the_header(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "maelsim.h"', "int main(void) {"]
    for name, st in A.JOURNAL_RECORDS.items():
        lines.append(f'  printf("{name} - %zu 0\\n", sizeof({name}));')
        for field, _ in st._fields_:
            lines.append(f'  printf("{name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    seen = 0
    for line in filter(None, subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")):
        name, field, a, b = line.split()
        st, (a, b) = A.JOURNAL_RECORDS[name], (int(a), int(b))
        dt = np.dtype(st)
        if field == "-":
            assert C.sizeof(st) == a == dt.itemsize, line
        else:
            assert (getattr(st, field).offset, getattr(st, field).size) == (a, b) == (dt.fields[field][1], dt.fields[field][0].itemsize), line
        seen += 1
    assert seen == 2 + 8 + 16


@pytest.mark.parametrize("name", list(ORACLE))
def test_oracle_journals(lib, name):
    """the journals the oracle writes are well-formed, and the classes are the reference's: the counts of all three equal the counters
    the oracle keeps while it runs (msim_net_stats) — for the lin-kv proxy, whose service endpoint lies behind the client slots, that
    pins the class rule (journal_stats counts the service as a client)"""
    cfg, ora = oracle_journals(name)
    for i in range(ora.n):
        ev = ora.events(i)
        assert int(ora.meta[i]["flags"]) == 0 and 200 <= len(ev) <= 3100   # (hand-sized; the largest, ack-retry's second instance, has 3003)
        ids = np.unique(ev["msg"] >> 8)
        assert ids[0] == 0 and ids[-1] == len(ids) - 1   # dense from 0
        s, m = E.journal_messages_history(ev, cfg.n_nodes, slots_of(cfg))
        assert int(s["valid"]) == 1 and int(s["flags"]) == 0 and len(m) == int(s["n_msgs"])
        st = ora.stats[i]
        for k, cls in enumerate(("all", "clients", "servers")):
            assert (int(s["send_count"][k]), int(s["recv_count"][k])) == (int(st[cls + "_send"]), int(st[cls + "_recv"])), (name, i, cls)
        assert list(s["msg_count"]) == list(s["send_count"])
        got = m[m["recv_event"] != A.NO_VALUE]
        assert (got["recv_event"] > got["send_event"]).all() and len(got) == int(s["recv_count"][0])
        assert int(s["undelivered"][0]) == len(m) - len(got) == int(s["send_count"][0]) - int(s["recv_count"][0])
        if name == "ack-retry":
            assert int(s["undelivered"][2]) > 0 and int(s["latency"][1]["q_us"][1]) > 0   # partitions drop; the net has a latency
        if name == "lin-kv proxy":
            legacy = E.journal_stats(ev, cfg.n_nodes)
            assert legacy["clients"]["send-count"] > int(s["send_count"][1]) == int(st["clients_send"])
            assert E.journal_analysis(s, service_names=["lin-kv"])["delivery"]["endpoints"][-1] == "lin-kv"
        assert host(ev, len(m), cfg.n_nodes, slots_of(cfg))[0].tobytes() == R.packed(ev, cfg.n_nodes, slots_of(cfg), len(m))[0].tobytes()


def test_a_capped_journal_is_a_well_formed_prefix(lib):
    cfg, ora = oracle_journals("ack-retry", 1000)
    full = oracle_journals("ack-retry")[1]
    for i in range(ora.n):
        ev = ora.events(i)
        assert int(ora.meta[i]["flags"]) & A.FLAG_JOURNAL_OVERFLOW and len(ev) == 1000 and ev.tobytes() == full.events(i)[:1000].tobytes()
        s, m = E.journal_messages_history(ev, cfg.n_nodes, slots_of(cfg))
        assert int(s["valid"]) == 1 and int(s["n_events"]) == 1000
