"""The explaining lin-kv check on the host (msim_explain_lin_kv_rows, csrc/lin_check.cpp): per key Knossos' :op, :previous-ok, the
register values of the :configs and the open calls (include/maelsim.h msim_lin_key_result), against tests/lin_explain_ref.py (a search
without pruning) and against what tests/lin_explain_cases.py writes out by hand; the final register values the reference's docs print
(tests/golden/checker_doc_vectors.json); the three entries' declarations, exports, prototypes and argument checks.  Needs no device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import lin_explain_cases as K
import lin_explain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("msim_explain_lin_kv_rows", "msim_explain_lin_kv_batch", "msim_explain_lin_kv")
FIELDS = ("key", "valid", "op_row", "previous_ok_row", "n_pending", "n_values")


def _as_dict(rec):
    d = {f: int(rec[f]) for f in FIELDS}
    d["values"] = [int(v) for v in rec["values"]]
    return d


def _explain(lib, rows, max_keys=256):
    """the raw entry: (check record, key records, n_keys)"""
    rows = np.ascontiguousarray(rows)
    out = A.CheckResult()
    keys = np.zeros(max_keys, dtype=E.LIN_KEY_DT)
    n = C.c_uint32()
    assert lib.msim_explain_lin_kv_rows(rows.ctypes.data, len(rows), C.byref(out), keys.ctypes.data, max_keys, C.byref(n)) == A.OK
    return out, keys, n.value


def _same_as_plain_check(lib, rows, out):
    plain = A.CheckResult()
    assert lib.msim_check_lin_kv_rows(np.ascontiguousarray(rows).ctypes.data, len(rows), C.byref(plain)) == A.OK
    assert bytes(plain) == bytes(out)


@pytest.mark.parametrize("nemesis", [False, True], ids=["plain", "nemesis rows in between"])
@pytest.mark.parametrize("name", list(K.HAND))
def test_hand_written_histories(lib, name, nemesis):
    ops, want = K.HAND[name]
    rows = K.encode(K.with_nemesis(ops) if nemesis else ops)
    at = [i for i, op in enumerate(K.with_nemesis(ops) if nemesis else ops) if op["process"] != ":nemesis"]   # row of the i-th client op
    out, keys, n = _explain(lib, rows)
    _same_as_plain_check(lib, rows, out)
    ref = R.explain(rows)
    assert n == len(want) == len(ref) == out.attempt_count
    for got, r, (k, w) in zip(keys[:n], ref, sorted(want.items())):
        got = _as_dict(got)
        assert got == r, (name, got, r)
        w = dict(w, key=k, values=(w["values"] + [0] * 8)[:8])
        for f in ("op_row", "previous_ok_row"):
            if w[f] != K.NO:
                w[f] = at[w[f]]
        assert got == w, (name, got, w)
    assert out.error_count == sum(1 for w in want.values() if w["valid"] == 0)
    assert all(int(v) == 0 for v in keys[n:]["valid"]) and not keys[n:]["n_values"].any()   # nothing beyond the history's keys is touched


def test_max_keys_smaller_than_the_key_count(lib):
    ops, want = K.HAND["two interleaved keys, one bad"]
    rows = K.encode(ops)
    out, keys, n = _explain(lib, rows, max_keys=1)
    _same_as_plain_check(lib, rows, out)
    assert n == 2 and (out.attempt_count, out.error_count, out.valid) == (2, 1, 0)   # the true count; the bad key 7 is still judged
    assert _as_dict(keys[0]) == R.explain(rows)[0] and int(keys[0]["key"]) == 3


def test_small_synthetic_histories_equal_the_unpruned_search(lib):
    """a few dozen rows each, overlaps, wrong results, :fail, :info, rows no client produces: every field of every record"""
    verdicts = set()
    for seed in range(40):
        ops = K.synthetic(seed, n_rows=12 + seed, keys=(0, 1), workers=4, p_overlap=0.4, p_wrong=0.08, p_info=0.1, odd=0.05 if seed % 3 == 0 else 0.0)
        rows = K.encode(ops)
        out, keys, n = _explain(lib, rows)
        _same_as_plain_check(lib, rows, out)
        ref = R.explain(rows)
        assert n == len(ref)
        assert [_as_dict(k) for k in keys[:n]] == ref, seed
        verdicts |= {r["valid"] for r in ref}
    assert {0, 1} <= verdicts


def test_more_than_64_open_calls_is_unknown(lib):
    for n_open, valid in ((63, 1), (64, 2)):   # (the read is a call too: 64 and 65 open at once)
        rows = K.encode(K.many_open_calls(n_open))
        out, keys, n = _explain(lib, rows)
        _same_as_plain_check(lib, rows, out)
        assert n == 1 and int(keys[0]["valid"]) == valid == out.valid
        if valid == 2:
            assert _as_dict(keys[0]) == dict(key=0, valid=2, op_row=K.NO, previous_ok_row=K.NO, n_pending=0, n_values=0, values=[0] * 8)
        else:
            assert (int(keys[0]["n_pending"]), int(keys[0]["n_values"]), int(keys[0]["values"][0])) == (63, 1, 1)   # (only a register of 1 lets the read return)


def test_a_failing_read_beside_many_open_writes(lib):
    """the closure before the failing read starts from hundreds of configurations (every subset of the open writes may have taken effect
    already); a call is linearized no earlier than a return needs it, so their values are those of the writes that returned"""
    for n_writes, done, read_value, n_info in ((9, 3, 99, 0), (8, 3, 99, 1), (7, 2, 12, 2)):
        rows = K.encode(K.wide_then_bad_read(n_writes, done, read_value, n_info))
        out, keys, n = _explain(lib, rows)
        _same_as_plain_check(lib, rows, out)
        assert n == 1 and [_as_dict(k) for k in keys[:1]] == R.explain(rows)
        if read_value == 99:
            first_read_ok = 2 + n_writes + n_info + done + 1
            want = dict(key=0, valid=0, op_row=first_read_ok, previous_ok_row=first_read_ok - 2, n_pending=n_writes - done + n_info,
                        n_values=done, values=([10 + i for i in range(done)] + [0] * 8)[:8])
            assert _as_dict(keys[0]) == want
        else:
            assert int(keys[0]["valid"]) == 1


with open(os.path.join(ROOT, "tests", "golden", "checker_doc_vectors.json")) as f:
    LIN = [v for v in json.load(f)["vectors"] if v["checker"] == "linearizable"]


@pytest.mark.parametrize("v", LIN, ids=[v["doc"] for v in LIN])
def test_doc_vectors_come_back_with_their_final_value(lib, v):
    rows = E.encode_lin_kv_history(v["history"])
    rec, keys = E.explain_lin_kv_history(rows)
    assert len(keys) == 1 and bool(keys[0]["valid"]) is v["expect"]["valid?"] and bool(rec["valid"]) is v["expect"]["valid?"]
    assert [_as_dict(k) for k in keys] == R.explain(rows)
    if "final-value" in v["expect"]:   # ":configs ({:model #knossos.model.CASRegister{:value 3}": the only entry of `values`
        assert int(keys[0]["n_values"]) == 1 and int(keys[0]["values"][0]) == v["expect"]["final-value"]
    a = E.lin_kv_analysis(rows, keys)
    assert a["valid?"] is v["expect"]["valid?"] and a["failures"] == ([] if v["expect"]["valid?"] else [int(keys[0]["key"])])


def test_analysis_map_names_the_ops(lib):
    ops, _ = K.HAND["two interleaved keys, one bad"]
    rows = K.encode(ops)
    _, keys = E.explain_lin_kv_history(rows)
    a = E.lin_kv_analysis(rows, keys)
    assert a["valid?"] is False and a["failures"] == [7] and sorted(a["results"]) == [3, 7]
    bad, good = a["results"][7]["linearizable"], a["results"][3]["linearizable"]
    assert (bad["valid?"], bad["op"]["index"], bad["op"]["type"], bad["op"]["f"], bad["op"]["value"]) == (False, 6, ":ok", ":read", [7, 4])
    assert (bad["previous-ok"]["index"], bad["previous-ok"]["value"], bad["configs"], bad["pending-count"]) == (2, [7, 1], [{"model": 1}], 0)
    assert good == {"valid?": True, "op": None, "previous-ok": None, "configs": [{"model": 2}], "value-count": 1, "pending-count": 0}
    _, keys = E.explain_lin_kv_history(K.encode(K.HAND["the first operation fails"][0]))
    assert E.lin_kv_analysis(K.encode(K.HAND["the first operation fails"][0]), keys)["results"][0]["linearizable"]["configs"] == [{"model": None}]


def test_entries_are_declared_exported_and_prototyped(lib):
    with open(os.path.join(ROOT, "include", "maelsim.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert name in A.EXPORTS and re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(lib, name) and getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    m = re.search(r"typedef struct msim_lin_key_result \{(.*?)\} msim_lin_key_result;", header, re.S)
    assert re.findall(r"(\w+)(?:\[8\])?;", m.group(1)) == [n for n in E.LIN_KEY_DT.names]
    assert E.LIN_KEY_DT.itemsize == C.sizeof(A.LinKeyResult) == 32
    assert all(callable(getattr(E, n)) for n in ("explain_lin_kv_history", "explain_lin_kv_batch", "lin_kv_analysis")) and callable(E.Engine.explain_lin_kv)


def test_entries_refuse_null_zero_and_out_of_range_arguments(lib):
    rows = np.zeros(2, dtype=E.OP_DT); off = np.asarray([0, 2], dtype=np.uint64); out = np.zeros(1, dtype=E.CHECK_DT)
    keys = np.zeros(4, dtype=E.LIN_KEY_DT); nk = C.c_uint32()
    res = C.cast(out.ctypes.data, C.POINTER(A.CheckResult))
    good = [rows.ctypes.data, 2, res, keys.ctypes.data, 4, C.byref(nk)]
    assert lib.msim_explain_lin_kv_rows(*good) == A.OK
    for i in (0, 2, 3, 5):                       # rows, out, keys, n_keys
        args = list(good); args[i] = None
        assert lib.msim_explain_lin_kv_rows(*args) == A.E_INVALID, i
    for mk in (0, 257):
        args = list(good); args[4] = mk
        assert lib.msim_explain_lin_kv_rows(*args) == A.E_INVALID, mk
    # the batch entry refuses before it touches a device
    good = [0, rows.ctypes.data, off.ctypes.data, 1, out.ctypes.data, keys.ctypes.data, 4, C.addressof(nk), None]
    for i in (1, 2, 4, 5, 7):                    # rows, row offsets, out, keys, n_keys
        args = list(good); args[i] = None
        assert lib.msim_explain_lin_kv_batch(*args) == A.E_INVALID, i
    args = list(good); args[3] = 0               # no histories
    assert lib.msim_explain_lin_kv_batch(*args) == A.E_INVALID
    for mk in (0, 257):
        args = list(good); args[6] = mk
        assert lib.msim_explain_lin_kv_batch(*args) == A.E_INVALID, mk
    assert lib.msim_explain_lin_kv(None, keys.ctypes.data, 4, C.addressof(nk), 1) == A.E_INVALID
