"""The explained pn-counter / g-counter, unique-ids and echo verdicts on the host (msim_explain_{pn,unique,echo}_rows, csrc/pn_check.cpp;
the contract: include/maelsim_small_explain.h) against tests/small_explain_ref.py — the contract restated in pure Python — on the
histories of tests/small_explain_cases.py and the reference's own pn-counter vectors.  Needs no device;
tests/test_small_explain_gpu.py holds the device entries against these host entries byte for byte."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import small_explain_cases as K
import small_explain_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5A5A5A5
PN, UNIQ, ECHO = K.pn_cases(), {**K.unique_cases(), **K.unique_bound_cases()}, K.echo_cases()
TABLES = K.unique_table_cases()
NO_PAY = np.zeros(1, dtype=np.uint32)


def host(entry, rows, hdr_dt, rec_dt, cap, *extra):
    """one host entry call over poisoned arrays -> (CHECK_DT record, header, the whole slab of `cap` records): the entry clears what it
    does not write"""
    rows = np.ascontiguousarray(rows)
    out = np.zeros(1, dtype=E.CHECK_DT)
    hdr = np.full(hdr_dt.itemsize // 4, POISON, dtype=np.uint32).view(hdr_dt)
    slab = np.full(max(cap, 1) * 4, POISON, dtype=np.uint32).view(rec_dt)
    rc = getattr(A.load(), entry)(rows.ctypes.data, len(rows), *extra, out.ctypes.data_as(C.POINTER(A.CheckResult)), hdr.ctypes.data, slab.ctypes.data, cap)
    assert rc == 0, (entry, rc)
    return out[0], hdr[0], slab[:cap]


def host_pn(rows, cap):
    return host("msim_explain_pn_rows", rows, E.PN_EXPLAIN_DT, E.PN_READ_DT, cap)


def host_unique(rows, cap):
    return host("msim_explain_unique_rows", rows, E.UNIQUE_EXPLAIN_DT, E.UNIQUE_DUP_DT, cap)


def host_echo(rows, concurrency, cap):
    return host("msim_explain_echo_rows", rows, E.ECHO_EXPLAIN_DT, E.ECHO_ERROR_DT, cap, concurrency)


def _same(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), (what, got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), (what, got[1][:6], want[1][:6])


def _pn_ops(rows):
    return E.decode_history(rows, NO_PAY, 0, A.WL_PN_COUNTER)


def _pn_total(rows):
    _, reads, ranges = X.pn(_pn_ops(rows))
    return len(reads), len(ranges)


@pytest.mark.parametrize("name", list(PN))
def test_pn_rows_against_the_walk(lib, name):
    """header and slab the walk's at a roomy capacity, at none, at the reads only and at one record short; the counts stay in the record"""
    rows = PN[name][0]
    ops = _pn_ops(rows)
    nr, ng = _pn_total(rows)
    for cap in sorted({nr + ng + 5, 0, nr, max(nr + ng - 1, 0), max(nr - 1, 0)}):
        out, hdr, slab = host_pn(rows, cap)
        _same((hdr, slab), X.pn_arrays(ops, cap), (name, cap))
        assert (int(out["attempt_count"]), int(out["stable_count"])) == (nr, ng)
        assert int(out["error_count"]) == sum(1 for r in X.pn(ops)[1] if not r[3])
        assert int(hdr["truncated"]) == int(cap < nr + ng)


def test_pn_plain_record_is_unchanged_by_the_sink(lib):
    for name, (rows, _) in PN.items():
        plain = A.CheckResult()
        rows = np.ascontiguousarray(rows)
        assert A.load().msim_check_pn_rows(rows.ctypes.data, len(rows), C.byref(plain), None, 0, None) == 0
        assert bytes(plain) == host_pn(rows, 8)[0].tobytes(), name


def test_pn_shapes_of_the_cases(lib):
    """the cases are what their names say"""
    assert _pn_total(PN["powers of two"][0]) == (4, 1024)
    _, reads, ranges = X.pn(_pn_ops(PN["run ends on bit 63"][0]))
    assert ranges == [(0, 63), (128, 191)] and [r[3] for r in reads] == [1, 0, 1, 1, 0]
    assert X.pn(_pn_ops(PN["run spans a word boundary"][0]))[2] == [(0, 10), (60, 70)]
    assert X.pn(_pn_ops(PN["run covers a word"][0]))[2] == [(0, 130), (1000, 1130)]
    for name, width in (("window 4095", 4095), ("window 4096", 4096)):
        ranges = X.pn(_pn_ops(PN[name][0]))[2]
        assert ranges[-1][1] - ranges[0][0] == width and len(ranges) == 4
    assert [r[0] for r in X.pn(_pn_ops(PN["reads in rows 63 and 64"][0]))[1]] == [63, 64, 65]
    assert [r[:2] for r in X.pn(_pn_ops(PN["reads that are not listed"][0]))[1]] == [(4, 2)]
    assert [r[3] for r in X.pn(_pn_ops(PN["below and above the window"][0]))[1]] == [0, 0, 1]


REFERENCE = [   # test/maelstrom/workload/pn_counter_test.clj:10-36
    ([], {"valid?": True, "errors": None, "final-reads": [], "acceptable": [[0, 0]]}),
    ([{"type": ":ok", "f": ":add", "value": 2}, {"type": ":ok", "f": ":add", "value": 3},
      {"type": ":ok", "f": ":read", "final?": True, "value": 5}, {"type": ":ok", "f": ":read", "final?": True, "value": 4}],
     {"valid?": False, "errors": [{"type": ":ok", "f": ":read", "final?": True, "value": 4}], "final-reads": [5, 4], "acceptable": [[5, 5]]}),
    ([{"type": ":ok", "f": ":add", "value": 10}, {"type": ":info", "f": ":add", "value": 5}, {"type": ":info", "f": ":add", "value": -1},
      {"type": ":info", "f": ":add", "value": -1}, {"type": ":ok", "f": ":read", "final?": True, "value": 11},
      {"type": ":ok", "f": ":read", "final?": True, "value": 15}],
     {"valid?": False, "errors": [{"type": ":ok", "f": ":read", "final?": True, "value": 11}], "final-reads": [11, 15], "acceptable": [[8, 10], [13, 15]]}),
]


@pytest.mark.parametrize("ops,want", REFERENCE)
def test_pn_analysis_gives_the_references_maps(lib, ops, want):
    rows = E.encode_pn_history(ops)
    got = E.pn_analysis(*E.explain_pn_history(rows), rows=rows)
    errors = got.pop("errors")
    assert got == {k: v for k, v in want.items() if k != "errors"}
    assert (errors and [{k: o[k] for k in ("type", "f", "final?", "value")} for o in errors]) == want["errors"]
    assert E.pn_analysis(*E.explain_pn_history(rows))["errors"] == ([i for i, o in enumerate(ops) if o in (want["errors"] or [])] or None)   # (without rows: row indices)


def _uniq_ops(rows):
    return E.decode_history(rows, NO_PAY, 0, A.WL_UNIQUE_IDS, A.NODE_TSO_IDS)


@pytest.mark.parametrize("name", list(UNIQ) + [next(iter(t)) for t in TABLES])
def test_unique_rows_against_the_walk(lib, name):
    rows = {**UNIQ, **TABLES[0], **TABLES[1]}[name][0]
    ops = _uniq_ops(rows)
    n = len(X.unique(ops))
    for cap in sorted({n + 3, 0, 1, max(n - 1, 0)}):
        out, hdr, slab = host_unique(rows, cap)
        _same((hdr, slab), X.unique_arrays(ops, cap), (name, cap))
        assert int(out["duplicated_count"]) == n and int(hdr["truncated"]) == int(cap < n)
    plain = A.CheckResult()
    assert A.load().msim_check_unique_rows(np.ascontiguousarray(rows).ctypes.data, len(rows), C.byref(plain)) == 0
    assert bytes(plain) == out.tobytes()


def test_unique_shapes_of_the_cases(lib):
    assert [d[:2] for d in X.unique(_uniq_ops(UNIQ["2, 3 and 70 times"][0]))] == [(13, 70), (12, 3), (11, 2)]
    assert X.unique(_uniq_ops(UNIQ["first rows adjacent"][0])) == [(500, 2, 10, 11)]
    assert X.unique(_uniq_ops(UNIQ["first rows in two chunks"][0])) == [(501, 3, 5, 200)]
    assert X.unique(_uniq_ops(UNIQ["first rows in two wavefronts"][0])) == [(502, 3, 3, 64)]
    assert [d[:2] for d in X.unique(_uniq_ops(UNIQ["ties in count"][0]))] == [(4, 3), (9, 2), (8, 2), (7, 2), (6, 2), (5, 2)]
    assert X.unique(_uniq_ops(UNIQ["smallest and largest id"][0])) == [(0xFFFFFFFF, 3, 1, 4), (0xFFFFFFFE, 2, 5, 7), (0, 2, 0, 3)]
    d = A.UNIQUE_EXPLAIN_MAX_DUPS
    assert d >= 48 and len(X.unique(_uniq_ops(UNIQ["at the bound"][0]))) == d and len(X.unique(_uniq_ops(UNIQ["beyond the bound"][0]))) == d + 1
    assert len(X.unique(_uniq_ops(TABLES[0]["table more than half full"][0]))) == 40 and len(TABLES[0]["table more than half full"][0]) > 32768 // 2
    assert len(TABLES[1]["19661 ids"][0]) == 19661


def test_unique_ids_analysis(lib):
    rows = UNIQ["ties in count"][0]
    got = E.unique_ids_analysis(*E.explain_unique_history(rows), node_program=A.NODE_TSO_IDS)
    assert got["valid?"] is False and got["duplicated-count"] == 6 and got["acknowledged-count"] == len(rows)
    assert got["duplicated"] == [[4, 3], [5, 2], [6, 2], [7, 2], [8, 2], [9, 2]] and got["range"][0] == 4
    flake = E.unique_ids_analysis(*E.explain_unique_history(K.gen_rows([(7 << 20) | (3 << 5) | 2] * 2)))
    assert flake["duplicated"] == [[[7, 3, "n2"], 2]] and flake["range"] == [[7, 3, "n2"], [7, 3, "n2"]]
    at = E.unique_ids_analysis(*E.explain_unique_history(UNIQ["at the bound"][0]), node_program=A.NODE_TSO_IDS)
    assert len(at["duplicated"]) == 48 and at["truncated"] is True and at["duplicated-count"] == A.UNIQUE_EXPLAIN_MAX_DUPS
    assert [d[0] for d in at["duplicated"]] == list(range(A.UNIQUE_EXPLAIN_MAX_DUPS - 47, A.UNIQUE_EXPLAIN_MAX_DUPS + 1))


def _echo_ops(rows):
    return E.decode_history(rows, NO_PAY, 0, A.WL_ECHO)


@pytest.mark.parametrize("name", list(ECHO))
def test_echo_rows_against_the_walk(lib, name):
    rows, conc = ECHO[name]
    ops = _echo_ops(rows)
    n = len(X.echo(ops, rows, conc))
    for cap in sorted({n + 3, 0, 1, max(n - 1, 0)}):
        out, hdr, slab = host_echo(rows, conc, cap)
        _same((hdr, slab), X.echo_arrays(ops, rows, conc, cap), (name, cap))
        assert int(out["error_count"]) == n and int(out["valid"]) == int(n == 0) and int(hdr["truncated"]) == int(cap < n)
        assert int(out["op_count"]) == sum(1 for o in ops if o["type"] == ":invoke" and o["process"] != ":nemesis")


def test_echo_shapes_of_the_cases(lib):
    NO = A.NO_VALUE
    assert X.echo(_echo_ops(ECHO["invocation in row 63"][0]), None, 3) == [(63, 64, 901, 902)]
    assert X.echo(_echo_ops(ECHO["every kind of error"][0]), None, 3) == [(0, NO, 1, NO), (1, 4, 2, 9), (5, NO, 4, NO), (10, 11, 6, 7), (12, NO, 8, NO), (13, NO, 10, NO)]
    assert len(X.echo(_echo_ops(ECHO["100 errors"][0]), None, 4)) == 100
    got = E.echo_analysis(*E.explain_echo_history(ECHO["every kind of error"][0], 3))
    assert got["valid?"] is False and got["errors"][:2] == [
        ["Expected a message with :echo", "Please echo 1", "But received", None],
        ["Expected a message with :echo", "Please echo 2", "But received", {"type": "echo_ok", "echo": "Please echo 9"}]]
    assert E.echo_analysis(*E.explain_echo_history(ECHO["clean"][0], 2)) == {"valid?": True, "errors": []}


def test_null_arguments(lib):
    rows = np.ascontiguousarray(PN["info 5"][0])
    out, hdr = A.CheckResult(), np.zeros(1, dtype=E.PN_EXPLAIN_DT)
    L = A.load()
    assert L.msim_explain_pn_rows(rows.ctypes.data, len(rows), C.byref(out), hdr.ctypes.data, None, 0) == 0 and int(hdr[0]["truncated"]) == 1
    assert L.msim_explain_pn_rows(rows.ctypes.data, len(rows), C.byref(out), hdr.ctypes.data, None, 1) == A.E_INVALID
    assert L.msim_explain_unique_rows(rows.ctypes.data, len(rows), C.byref(out), None, None, 0) == A.E_INVALID
    assert L.msim_explain_echo_rows(rows.ctypes.data, len(rows), 0, C.byref(out), hdr.ctypes.data, None, 0) == A.E_INVALID


def test_abi(lib):
    """the records and entries against include/maelsim_small_explain.h (which maelsim.h includes): arity by the declarations, as
    tests/test_abi_tables.py does for maelsim.h's own"""
    header = open(os.path.join(ROOT, "include", "maelsim_small_explain.h")).read()
    assert '#include "maelsim_small_explain.h"' in open(os.path.join(ROOT, "include", "maelsim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = {name: params.split(",") for name, params in re.findall(r"^int\s*(msim_[a-z0-9_]+)\(([^)]*)\);", text, re.M)}
    assert list(decls) == list(A.SMALL_EXPLAIN_PROTOTYPES) and len(decls) == 9
    for name, params in decls.items():
        restype, argtypes = A.SMALL_EXPLAIN_PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(params), name
        for t, p in zip(argtypes, params):
            assert ("*" in p) == (t is C.c_void_p or issubclass(t, C._Pointer)), (name, p)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == list(argtypes), name
    assert set(re.findall(r"^\}\s*(msim_[a-z0-9_]+);", header, re.M)) == set(A.SMALL_EXPLAIN_RECORDS)
    assert [np.dtype(s).itemsize for s in A.SMALL_EXPLAIN_RECORDS.values()] == [16, 16, 24, 16, 8, 16, 8]
    bound = int(re.search(r"#define MSIM_UNIQUE_EXPLAIN_MAX_DUPS (\d+)u", header).group(1))
    assert bound == A.UNIQUE_EXPLAIN_MAX_DUPS >= 48 and A.PN_EXPLAIN_WINDOW == 4096


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_records_match_the_header(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "maelsim.h"', "int main(void) {"]
    for name, st in A.SMALL_EXPLAIN_RECORDS.items():
        lines.append(f'  printf("{name} - %zu 0\\n", sizeof({name}));')
        for field, _ in st._fields_:
            lines.append(f'  printf("{name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    seen = 0
    for line in filter(None, subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")):
        name, field, a, b = line.split()
        st, (a, b) = A.SMALL_EXPLAIN_RECORDS[name], (int(a), int(b))
        dt = np.dtype(st)
        if field == "-":
            assert C.sizeof(st) == a == dt.itemsize, line
        else:
            assert (getattr(st, field).offset, getattr(st, field).size) == (a, b) == (dt.fields[field][1], dt.fields[field][0].itemsize), line
        seen += 1
    assert seen == 7 + 4 + 2 + 5 + 4 + 2 + 4 + 2
