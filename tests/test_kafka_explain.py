"""The explained kafka verdicts on the host (msim_explain_kafka_rows, csrc/kafka_check.cpp; the contract: include/maelsim.h, "kafka: the
explanation of a verdict") against tests/kafka_explain_ref.py — the contract restated in pure Python — on the reference text's known
answer (workload/kafka.clj:42-60), one history per anomaly, the order-sensitive pairs and the 72 corrupted oracle histories.  Needs no
device; tests/test_kafka_explain_gpu.py holds the device entries against this host entry byte for byte."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import kafka_classify_cases as K
import kafka_explain_ref as X
from test_kafka import _h, _poll, _send
from test_kafka_check_gpu import FIELDS, _anomalies, _host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT = X.BIT
_BAD, _GOOD = _anomalies()
HAND = {name: E.encode_kafka_history(ops) for name, ops in list(_BAD.items()) + list(_GOOD.items())}
POISON = 0xA5A5A5A5


def host(h, max_findings=64):
    """one host entry call -> (CHECK_DT record, KAFKA_EXPLAIN_DT header, the whole slab of max_findings records); the entry clears what it
    does not write"""
    rows = np.ascontiguousarray(h[0]); pay = np.ascontiguousarray(h[1], dtype=np.uint32)
    out = np.zeros(1, dtype=E.CHECK_DT)
    hdr = np.full(E.KAFKA_EXPLAIN_DT.itemsize // 4, POISON, dtype=np.uint32).view(E.KAFKA_EXPLAIN_DT)
    slab = np.full(max(max_findings, 1) * 8, POISON, dtype=np.uint32).view(E.KAFKA_FINDING_DT)
    rc = A.load().msim_explain_kafka_rows(rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), out.ctypes.data_as(C.POINTER(A.CheckResult)),
                                          hdr.ctypes.data, slab.ctypes.data, max_findings)
    assert rc == 0, rc
    return out[0], hdr[0], slab[:max_findings]


def as_arrays(found, count, max_findings):
    """the reference's findings as the header and slab the contract lays out"""
    hdr = np.zeros(1, dtype=E.KAFKA_EXPLAIN_DT)
    slab = np.zeros(max_findings, dtype=E.KAFKA_FINDING_DT)
    n = min(len(found), max_findings)
    hdr[0]["n_findings"], hdr[0]["truncated"], hdr[0]["count"] = n, int(len(found) > max_findings), count
    for i, f in enumerate(found[:n]):
        slab[i] = f + (0,)
    return hdr[0], slab


def invariants(out, hdr, what):
    bits = int(out["error_count"])
    for i in range(10):
        assert (int(hdr["count"][i]) > 0) == bool(bits >> i & 1), (what, i, bits, hdr)
    assert int(hdr["count"][0]) == int(out["lost_count"]) and int(hdr["count"][7]) == int(out["duplicated_count"]), (what, hdr, out)
    assert int(hdr["count"][9]) <= 1


def against_ref(h, what, max_findings=64):
    """record, header and slab of one history: the record msim_check_kafka_rows writes, the reference's findings byte for byte, the
    three invariants"""
    out, hdr, slab = host(h, max_findings)
    plain = _host(*h)
    assert {f: int(out[f]) for f in FIELDS} == plain, (what, out, plain)
    found, count = X.explain(*h)
    want_hdr, want_slab = as_arrays(found, count, max_findings)
    assert hdr.tobytes() == want_hdr.tobytes(), (what, max_findings, hdr, want_hdr)
    assert slab.tobytes() == want_slab.tobytes(), (what, max_findings, slab[:8], want_slab[:8])
    invariants(out, hdr, what)
    return out, hdr, slab[:int(hdr["n_findings"])]


def test_abi(lib):
    """the records and entries against include/maelsim_kafka_explain.h (which maelsim.h includes): sizes and offsets by a C probe, arity
    by the declarations, as tests/test_abi_tables.py does for maelsim.h's own"""
    header = open(os.path.join(ROOT, "include", "maelsim_kafka_explain.h")).read()
    main = open(os.path.join(ROOT, "include", "maelsim.h")).read()
    assert '#include "maelsim_kafka_explain.h"' in main and "kafka: the explanation of a verdict" in main
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = {name: [p for p in params.split(",")] for name, params in re.findall(r"^int\s*(msim_[a-z0-9_]+)\(([^)]*)\);", text, re.M)}
    assert list(decls) == list(A.KAFKA_EXPLAIN_PROTOTYPES)
    for name, params in decls.items():
        restype, argtypes = A.KAFKA_EXPLAIN_PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(params), name
        for t, p in zip(argtypes, params):
            assert ("*" in p) == (t is C.c_void_p or issubclass(t, C._Pointer)), (name, p)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == list(argtypes), name
    assert set(re.findall(r"^\}\s*(msim_[a-z0-9_]+);", header, re.M)) == set(A.KAFKA_EXPLAIN_RECORDS)
    assert E.KAFKA_FINDING_DT.itemsize == C.sizeof(A.KafkaFinding) == 32 and E.KAFKA_EXPLAIN_DT.itemsize == C.sizeof(A.KafkaExplain) == 48
    assert (A.KAFKA_EXPLAIN_TABLE_BOUND, A.KAFKA_EXPLAIN_MAX_FINDINGS) == (384, 1024)
    assert lib.msim_abi_version() == 1


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_records_match_the_header(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "maelsim.h"', "int main(void) {"]
    for name, st in A.KAFKA_EXPLAIN_RECORDS.items():
        lines.append(f'  printf("{name} - %zu 0\\n", sizeof({name}));')
        for field, _ in st._fields_:
            lines.append(f'  printf("{name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    seen = 0
    for line in filter(None, subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")):
        name, field, a, b = line.split()
        st, (a, b) = A.KAFKA_EXPLAIN_RECORDS[name], (int(a), int(b))
        dt = np.dtype(st)
        if field == "-":
            assert C.sizeof(st) == a == dt.itemsize, line
        else:
            assert (getattr(st, field).offset, getattr(st, field).size) == (a, b) == (dt.fields[field][1], dt.fields[field][0].itemsize), line
        seen += 1
    assert seen == 2 + 8 + 3


def test_the_reference_texts_known_answer(lib):
    """workload/kafka.clj:42-60 with key "5": the process polled up to offset 5, then from 8 on — :delta 3, offsets 6 and 7 skipped"""
    out, hdr, fs = against_ref(HAND["poll_skip"], "poll_skip")
    assert int(hdr["n_findings"]) == 1 and int(hdr["truncated"]) == 0
    f = fs[0]
    assert tuple(int(f[n]) for n in ("anomaly", "key", "offset", "value", "other", "row_a", "row_b", "reserved")) == (BIT["poll-skip"], 5, 8, 2, 5, 19, 21, 0)
    named = E.kafka_findings(hdr, fs)
    assert named == [{"anomaly": "poll-skip", "key": 5, "offset": 8, "value": 2, "other": 5, "row-a": 19, "row-b": 21, "delta": 3, "skipped-count": 2}]
    rows, pay = HAND["poll_skip"]
    ops = E.decode_history(rows, pay, 3, A.WL_KAFKA)
    assert ops[19]["f"] == ops[21]["f"] == ":poll" and ops[19]["type"] == ops[21]["type"] == ":ok" and ops[19]["process"] == ops[21]["process"] == 0


WANT = {   # name: [(anomaly, key, offset, value, other, row_a, row_b)] — worked out by hand from the histories of _anomalies()
    "lost": [("lost-write", 1, 1, 2, 2, 3, 9)],
    "nm_poll": [("nonmonotonic-poll", 1, 1, 2, 1, 5, 7)],
    "nm_send": [("nonmonotonic-send", 1, 3, 2, 3, 1, 3), ("inconsistent-offsets", 1, 3, 2, 1, 1, 3)],
    "int_skip": [("lost-write", 1, 1, 2, 3, 3, 11), ("lost-write", 1, 2, 3, 3, 5, 11), ("int-poll-skip", 1, 3, 2, 0, 11, 11)],
    "int_nm": [("int-nonmonotonic-poll", 1, 0, 1, 1, 5, 5)],
    "incons": [("inconsistent-offsets", 1, 0, 7, 1, 1, 3)],
    "dup": [("duplicate", 1, 1, 1, 0, 1, 3)],
    "aborted": [("aborted-read", 1, 0, 1, 0, 1, 3)],
    "returning": [("nonmonotonic-send", 1, 0, 3, 0, 1, 5), ("inconsistent-offsets", 1, 0, 3, 1, 1, 5)],
}


@pytest.mark.parametrize("name", list(HAND))
def test_one_history_per_anomaly(lib, name):
    """tests/test_kafka_check_gpu.py's hand-made histories: the findings worked out by hand, the good ones none; `returning` (a process
    that comes back) is the host's to judge on every route, so it is judged here"""
    out, hdr, fs = against_ref(HAND[name], name)
    got = [(A.KAFKA_ANOMALIES[int(f["anomaly"])],) + tuple(int(f[n]) for n in ("key", "offset", "value", "other", "row_a", "row_b")) for f in fs]
    if name == "poll_skip":
        return
    assert got == WANT.get(name, []), (name, got)
    assert (name in _GOOD) == (int(hdr["n_findings"]) == 0 and int(out["valid"]) != 0)


def _what_differs(a, b):
    """the findings' rows and values, as lists: the pair inside ONE row differs in how many findings hold a value"""
    return sorted((int(f["row_a"]), int(f["row_b"]), int(f["value"])) for f in a) != sorted((int(f["row_a"]), int(f["row_b"]), int(f["value"])) for f in b)


def test_order_vectors(lib):
    """the same observations in another order: last(k,o), home(k,m) and the first disagreeing observation move, so each fwd / rev pair
    differs in row_a / row_b or value"""
    vec = K.order_vectors()
    got = {name: against_ref(h, name) for name, h in vec.items()}
    for a, b in (("A fwd", "A rev"), ("B fwd", "B rev"), ("B one row", "B one reversed")):
        assert _what_differs(got[a][2], got[b][2]), (a, got[a][2], got[b][2])
    a_rev = E.kafka_findings(got["A rev"][1], got["A rev"][2])
    assert [f["anomaly"] for f in a_rev] == ["inconsistent-offsets", "aborted-read"] and a_rev[0]["value"] == 1 and a_rev[0]["other"] == 2


def test_corrupted_family(lib):
    """the 72 mutated oracle histories: every record, header and slab the reference's; the invariants on each; findings of at least six kinds"""
    hs = K.corrupted_family()
    assert len(hs) == 72
    kinds, unclean = set(), 0
    for i, h in enumerate(hs):
        out, hdr, fs = against_ref(h, f"family {i}", max_findings=256)
        assert int(hdr["truncated"]) == 0
        kinds |= {int(f["anomaly"]) for f in fs}
        unclean += int(hdr["n_findings"]) > 0
    assert unclean >= 20 and len(kinds) >= 6, (unclean, kinds)


def _many():
    """nine findings of seven kinds in one history (tests/test_kafka_classify_gpu.py's _five_bits)"""
    return E.encode_kafka_history(_h(*(sum((_send(0, "1", m, m - 1) for m in range(1, 6)), [])), *_send(0, "1", 6, 4), *_send(0, "1", 9, typ=":fail"),
                                     *_poll(1, {"1": [[0, 1], [3, 4]]}), *_poll(1, {"1": [[3, 4]]}), *_poll(2, {"1": [[5, 9]]}), *_poll(2, {"1": [[6, 1]]})))


def test_truncation(lib):
    """max_findings 0, 1, n - 1 and n: the first ones in the contract's order, zeros beyond n_findings, the true counts always"""
    h = _many()
    full_out, full_hdr, full = against_ref(h, "many")
    n = int(full_hdr["n_findings"])
    assert n >= 6 and int(full_hdr["truncated"]) == 0
    keys = [tuple(int(f[x]) for x in ("anomaly", "key", "offset", "value", "other", "row_a", "row_b")) for f in full]
    assert keys == sorted(keys)
    for cap in (0, 1, n - 1, n):
        out, hdr, slab = host(h, cap)
        assert out.tobytes() == full_out.tobytes()
        assert int(hdr["n_findings"]) == cap and int(hdr["truncated"]) == int(cap < n) and list(hdr["count"]) == list(full_hdr["count"])
        assert slab[:cap].tobytes() == full[:cap].tobytes()
        against_ref(h, "many", cap)
    out, hdr, slab = host(h, n + 3)
    assert int(hdr["n_findings"]) == n and not slab[n:].tobytes().strip(b"\0")
    rows, pay = h
    out = np.zeros(1, dtype=E.CHECK_DT); hdr = np.zeros(1, dtype=E.KAFKA_EXPLAIN_DT)
    args = (rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), out.ctypes.data_as(C.POINTER(A.CheckResult)), hdr.ctypes.data)
    assert A.load().msim_explain_kafka_rows(*args, None, 0) == 0 and int(hdr[0]["truncated"]) == 1   # (no slab is legal with max_findings 0)
    assert A.load().msim_explain_kafka_rows(*args, None, 1) == A.E_INVALID


def test_python_entry(lib):
    out, hdr, fs = E.explain_kafka_history(*_many(), max_findings=4)
    assert len(fs) == 4 and int(hdr["truncated"]) == 1 and len(fs.base) == 4
    named = E.kafka_findings(hdr, fs)
    assert [f["anomaly"] for f in named[:4]] == ["lost-write"] * 3 + ["nonmonotonic-poll"] and named[3]["delta"] == 0
    assert named[-1] == {"truncated": {"lost-write": 3, "nonmonotonic-poll": 1, "nonmonotonic-send": 1, "int-poll-skip": 1, "inconsistent-offsets": 1,
                                       "duplicate": 1, "aborted-read": 1}}
