"""The non-cycle findings of the transactional checkers on the host (msim_explain_txn_findings_rows, csrc/txn_check.cpp) against the
contract of include/maelsim_txn_findings.h as tests/txn_findings_ref.py restates it: header and slab byte for byte on every history of
tests/txn_findings_cases.py under all five models, the check record that of msim_check_txn_rows / msim_check_rw_rows; the invariant
between count[] and the record's anomaly bits; truncation; the ABI tables against the header; the reference documentation's
transactions (tests/golden/elle_doc_vectors.json) with the findings the documentation prints.  Needs no device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import test_elle_reference_vectors as V
import txn_findings_cases as K
import txn_findings_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = list(E.CONSISTENCY_MODELS)
NV = A.NO_VALUE
_REF = {}


def ref(rw, name):
    """the reference's (header, records) of a case, computed once"""
    if (rw, name) not in _REF:
        rows, pay = K.cases(rw)[name]
        _REF[(rw, name)] = R.findings(rows, pay, rw)
    return _REF[(rw, name)]


def host(h, rw, model="strict-serializable", max_findings=64):
    """msim_explain_txn_findings_rows -> (CHECK_DT record, header, the whole slab of max_findings records)"""
    out, hdr, recs = E.explain_txn_findings_history(h[0], h[1], K.WORKLOAD[rw], model, max_findings)
    slab = recs.base if recs.base is not None else recs
    return out, hdr, slab[:max_findings]


def plain_check(h, rw, model):
    lib = A.load()
    rows = np.ascontiguousarray(h[0]); pay = np.ascontiguousarray(h[1], dtype=np.uint32)
    res = A.CheckResult()
    if rw:
        rc = lib.msim_check_rw_rows(rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), E.CONSISTENCY_MODELS[model], C.byref(res))
    else:
        rc = lib.msim_check_txn_rows(rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), C.byref(res))
    assert rc == 0
    return np.frombuffer(bytes(res), dtype=E.CHECK_DT)[0]


@pytest.mark.parametrize("rw", [False, True], ids=["list-append", "rw-register"])
def test_host_entry_equals_the_reference(lib, rw):
    """every case, all five models: header and slab are the reference's bytes, `out` is the plain check's record (list-append's plain
    entry judges under strict-serializable: under another model only `valid` may differ, by msim_violated_anomalies), and count[i] > 0
    iff bit i of error_count, for the seven non-cycle bits"""
    seen = set()
    for name, h in K.cases(rw).items():
        want_hdr, want = ref(rw, name)
        cap = max(len(want), 1)
        w_hdr, w_slab = R.truncated(want_hdr, want, cap)
        for model in MODELS:
            out, hdr, slab = host(h, rw, model, cap)
            assert hdr.tobytes() == w_hdr.tobytes(), (name, model, hdr, w_hdr)
            assert slab.tobytes() == w_slab.tobytes(), (name, model, [tuple(x) for x in slab[:4]], [tuple(x) for x in w_slab[:4]])
            check = plain_check(h, rw, model if rw else "strict-serializable")
            if not rw and model != "strict-serializable":
                violated = lib.msim_violated_anomalies(int(check["error_count"]), E.CONSISTENCY_MODELS[model])
                check = check.copy()
                check["valid"] = 0 if violated else (2 if int(check["ok_count"]) == 0 else 1)
            assert out.tobytes() == check.tobytes(), (name, model, out, check)
            for n in R.NON_CYCLE:
                bit = R.BIT[n]
                assert (int(hdr["count"][bit.bit_length() - 1]) > 0) == bool(int(out["error_count"]) & bit), (name, model, n, hdr, out)
            assert all(int(hdr["count"][i]) == 0 for i in (0, 3, 4, 5, 9))
        seen |= {n for n in R.NON_CYCLE if int(want_hdr["count"][R.BIT[n].bit_length() - 1])}
    missing = set(R.NON_CYCLE) - seen
    assert missing == ({"incompatible-order", "dirty-update"} if rw else {"cyclic-versions"}), missing


@pytest.mark.parametrize("rw", [False, True], ids=["list-append", "rw-register"])
def test_finding_counts(lib, rw):
    c = K.cases(rw)
    for n in K.COUNTS:
        hdr, recs = ref(rw, f"{n} findings")
        assert len(recs) == n and int(hdr["count"][1]) == n, (n, hdr)
    for n in K.SIZES:
        out, _, _ = host(c[f"{n} transactions"], rw)
        assert int(out["attempt_count"]) == n


@pytest.mark.parametrize("rw", [False, True], ids=["list-append", "rw-register"])
def test_truncation(lib, rw):
    """max_findings 0, 1, n - 1 and n: the first records in order, truncated iff one is missing, count[] the true numbers, the rest zero"""
    for name in ("65 findings", "hand: dirty-update" if not rw else "two payloads outside the area", "internal, G1a and duplicate on one read" if not rw else "internal and G1a in one transaction"):
        h = K.cases(rw)[name]
        want_hdr, want = ref(rw, name)
        n = len(want)
        assert n >= 2, name
        for cap in (0, 1, n - 1, n, n + 3):
            _, hdr, slab = host(h, rw, max_findings=cap)
            w_hdr, w_slab = R.truncated(want_hdr, want, cap)
            assert hdr.tobytes() == w_hdr.tobytes() and slab.tobytes() == w_slab.tobytes(), (name, cap, hdr, w_hdr)
            assert int(hdr["truncated"]) == (1 if cap < n else 0) and int(hdr["n_findings"]) == min(cap, n)
            assert list(hdr["count"]) == list(want_hdr["count"])
    lib_ = A.load()
    rows, pay = K.cases(rw)["65 findings"]
    rows = np.ascontiguousarray(rows); pay = np.ascontiguousarray(pay, dtype=np.uint32)
    out, hdr = np.zeros(1, dtype=E.CHECK_DT), np.zeros(1, dtype=E.TXN_EXPLAIN_DT)
    args = (rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), 0, out.ctypes.data_as(C.POINTER(A.CheckResult)), hdr.ctypes.data)
    wl = E.WORKLOADS[K.WORKLOAD[rw]]
    assert lib_.msim_explain_txn_findings_rows(wl, *args, None, 0) == 0 and int(hdr[0]["truncated"]) == 1      # the header alone
    assert lib_.msim_explain_txn_findings_rows(wl, *args, None, 4) == A.E_INVALID
    assert lib_.msim_explain_txn_findings_rows(A.WL_KAFKA, *args, None, 0) == A.E_INVALID
    assert lib_.msim_explain_txn_findings_rows(wl, *args[:4], 5, *args[5:], None, 0) == A.E_INVALID


def test_register_value_64_is_invalid(lib):
    h = E.encode_txn_history(K.RWT._ops((0, ":ok", [[":w", 1, 64]], [[":w", 1, 64]])), rw=True)
    with pytest.raises(E.EngineError, match="-1"):
        E.explain_txn_findings_history(h[0], h[1], "txn-rw-register")
    with pytest.raises(ValueError):
        R.findings(h[0], h[1], True)


def test_abi(lib):
    """the records and entries against include/maelsim_txn_findings.h (which maelsim.h includes)"""
    header = open(os.path.join(ROOT, "include", "maelsim_txn_findings.h")).read()
    main = open(os.path.join(ROOT, "include", "maelsim.h")).read()
    assert '#include "maelsim_txn_findings.h"' in main and "witnesses for the non-cycle anomalies" not in main
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = {name: params.split(",") for name, params in re.findall(r"^int\s*(msim_[a-z0-9_]+)\(([^)]*)\);", text, re.M)}
    assert list(decls) == list(A.TXN_FINDINGS_PROTOTYPES) and len(decls) == 3
    for name, params in decls.items():
        restype, argtypes = A.TXN_FINDINGS_PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(params), name
        for t, p in zip(argtypes, params):
            assert ("*" in p) == (t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)), (name, p)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == list(argtypes), name
    assert set(re.findall(r"^\}\s*(msim_[a-z0-9_]+);", header, re.M)) == set(A.TXN_FINDINGS_RECORDS)
    assert [np.dtype(s).itemsize for s in A.TXN_FINDINGS_RECORDS.values()] == [48, 64]
    assert int(re.search(r"#define MSIM_TXN_FINDINGS_CAPACITY (\d+)u", header).group(1)) == A.TXN_FINDINGS_CAPACITY >= 1024
    assert lib.msim_abi_version() == A.ABI_VERSION == 1


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_records_match_the_header(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "maelsim.h"', "int main(void) {"]
    for name, st in A.TXN_FINDINGS_RECORDS.items():
        lines.append(f'  printf("{name} - %zu 0\\n", sizeof({name}));')
        for field, _ in st._fields_:
            lines.append(f'  printf("{name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    seen = 0
    for line in filter(None, subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")):
        name, field, a, b = line.split()
        st, (a, b) = A.TXN_FINDINGS_RECORDS[name], (int(a), int(b))
        dt = np.dtype(st)
        if field == "-":
            assert C.sizeof(st) == a == dt.itemsize, line
        else:
            assert (getattr(st, field).offset, getattr(st, field).size) == (a, b) == (dt.fields[field][1], dt.fields[field][0].itemsize), line
        seen += 1
    assert seen == 2 + 12 + 4


def _vector(i, max_findings=64):
    v = V.VECTORS[i]
    rows, pay = E.encode_txn_history(v["history"])
    out, hdr, recs = E.explain_txn_findings_history(rows, pay, max_findings=max_findings)
    return v, rows, pay, hdr, recs, E.txn_findings_analysis(rows, pay, hdr, recs)["anomalies"]


def doc_vector_checks(explain):
    """What the reference's documentation prints for its transactions (tests/golden/elle_doc_vectors.json), asked of `explain(i) ->
    (rows, payload, header, records)`; shared with tests/test_txn_findings_gpu.py."""
    def of(i):
        rows, pay, hdr, recs = explain(i)
        return hdr, recs, E.txn_findings_analysis(rows, pay, hdr, recs)["anomalies"]
    count = lambda hdr, name: int(hdr["count"][R.BIT[name].bit_length() - 1])
    # vector 0: 01-single-node.md:117-141 — three transactions that do not see their own append
    hdr, recs, an = of(0)
    assert int(hdr["n_findings"]) == 3 and count(hdr, "internal") == 3
    assert all((int(f["key"]), int(f["mop"]), int(f["other_mop"]), int(f["count"])) == (9, 1, NV, 1) for f in recs)
    assert [e["mop"] for e in an["internal"]] == [[":r", 9, None]] * 3
    assert sorted(e["expected"][1] for e in an["internal"]) == [6, 12, 16] and all(e["expected"][0] == "..." and len(e["expected"]) == 2 for e in an["internal"])
    assert all(e["op"]["type"] == ":ok" and e["op"]["value"][1] == [":r", 9, None] for e in an["internal"])
    # vector 1: 01-single-node.md:260-287 — a read that misses the two appends since the transaction's earlier read
    hdr, recs, an = of(1)
    assert int(hdr["n_findings"]) == 1 and count(hdr, "internal") == 1
    assert (int(recs[0]["mop"]), int(recs[0]["other_mop"]), int(recs[0]["count"])) == (3, 0, 2)
    assert an["internal"][0]["mop"] == [":r", 9, [1, 2, 3, 4, 5, 6, 7]]
    # vector 2: 01-single-node.md:358-366 — four keys read in two orders
    hdr, recs, an = of(2)
    assert count(hdr, "incompatible-order") == 4 and count(hdr, "internal") == 0 and len(an["incompatible-order"]) == 4
    got = {e["key"]: {tuple(x) for x in e["values"]} for e in an["incompatible-order"]}
    assert got == {7: {(3, 4), (1, 2)}, 9: {(4, 5, 7), (1, 2, 3)}, 10: {(8,), (1,)}, 8: {(3, 4), (1, 2, 5)}}, got
    # vector 3: 02-shared-state.md:226-233 — process 2's transaction reads key 51 twice, differently
    hdr, recs, an = of(3)
    assert int(hdr["n_findings"]) == 1 and count(hdr, "internal") == 1
    assert (int(recs[0]["key"]), int(recs[0]["mop"]), int(recs[0]["other_mop"]), int(recs[0]["count"])) == (51, 1, 0, 0)
    assert an["internal"][0]["op"]["process"] == 2
    # vectors 4 and 5 (G-single-realtime): no non-cycle anomaly
    for i in (4, 5):
        hdr, recs, an = of(i)
        assert not hdr.tobytes().strip(b"\0") and len(recs) == 0 and an == {}


def test_doc_vectors(lib):
    """the reference documentation's transactions: the findings it prints, through the host entry and txn_findings_analysis"""
    assert len(V.VECTORS) >= 6

    def explain(i):
        _, rows, pay, hdr, recs, _ = _vector(i)
        return rows, pay, hdr, recs
    doc_vector_checks(explain)


def test_analysis_names_every_kind(lib):
    """txn_findings_analysis on the hand-made histories: every kind under elle's name, ops as decode_history gives them, and a slab
    shorter than the findings marked"""
    la, rw = K.cases(False), K.cases(True)

    def analysis(c, name, is_rw, cap=64):
        rows, pay = c[name]
        _, hdr, recs = E.explain_txn_findings_history(rows, pay, K.WORKLOAD[is_rw], max_findings=cap)
        return E.txn_findings_analysis(rows, pay, hdr, recs, rw=is_rw)["anomalies"]
    a = analysis(la, "hand: G1a-failed", False)
    assert a["G1a"][0]["element"] == 1 and a["G1a"][0]["writer"]["type"] == ":fail" and a["G1a"][0]["mop"] == [":r", 1, [1]]
    a = analysis(la, "hand: G1a-unwritten", False)
    assert a["G1a"][0]["element"] == 9 and a["G1a"][0]["writer"] is None
    a = analysis(la, "hand: G1b", False)
    assert (a["G1b"][0]["element"], a["G1b"][0]["writer-final"]) == (1, 2) and a["G1b"][0]["writer"]["value"] == [[":append", 1, 1], [":append", 1, 2]]
    a = analysis(la, "hand: duplicate-elements", False)
    assert a["duplicate-elements"][0]["positions"] == [0, 1] and a["duplicate-elements"][0]["element"] == 1
    a = analysis(la, "hand: dirty-update", False)
    assert (a["dirty-update"][0]["element"], a["dirty-update"][0]["aborted-element"]) == (2, 1) and a["dirty-update"][0]["writer"]["type"] == ":fail"
    a = analysis(la, "hand-off: appended three times", False)
    assert a["duplicate-elements"][0]["count"] == 3 and a["duplicate-elements"][0]["other-mop"] == [":append", 1, 1]
    a = analysis(la, "internal after a read", False)
    assert a["internal"][0]["expected"] == [1, 5, 6] and a["internal"][0]["mop"] == [":r", 1, [1, 5]]
    a = analysis(la, "65 findings", False, cap=3)
    assert len(a["G1a"]) == 4 and a["G1a"][-1] == {"truncated": 65}
    a = analysis(rw, "cyclic-versions", True)
    assert a["cyclic-versions"] == [{"key": 2, "element": 1, "count": 3}]
    a = analysis(rw, "internal after a write", True)
    assert a["internal"][0]["expected"] == 1 and a["internal"][0]["mop"] == [":r", 1, 2]
