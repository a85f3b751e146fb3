"""CPU-only: the two tables of maelstrom_amd/_abi.py (RECORDS, PROTOTYPES) against include/maelsim.h, the one calling convention they
allow (an array goes in as its address), and the two marshalling helpers of maelstrom_amd/engine.py against arrays written out by hand."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "maelsim.h")).read()


# ---- records ----
def _hand_written_dtypes():
    """the dtypes engine.py spelled out before it derived them"""
    u4 = "<u4"
    latency = np.dtype([("count", u4), ("q_us", u4, (5,)), ("sum_us", "<u8")])
    f_stats = np.dtype([("f", u4), ("valid", u4), ("count", u4), ("ok_count", u4), ("fail_count", u4), ("info_count", u4),
                        ("unpaired", u4), ("reserved", u4), ("latency", latency, (3,))])
    element = np.dtype([(n, u4) for n in ("element", "outcome", "latency_ms", "known_row", "last_present_row", "last_absent_row")])
    return {
        "OP_DT": np.dtype([("time_len", "<u8"), ("packed", u4), ("value", u4)]),
        "STATS_DT": np.dtype([(n, "<u8") for n in ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv")]),
        "META_DT": np.dtype([(n, u4) for n in ("n_rows", "n_payload_words", "flags", "n_rounds", "n_events", "r0", "r1", "r2")]),
        "EVENT_DT": np.dtype([(n, u4) for n in ("time_us", "msg", "a", "route")]),
        "CHECK_DT": np.dtype([("valid", u4), ("attempt_count", u4), ("stable_count", u4), ("lost_count", u4), ("never_read_count", u4),
                              ("stale_count", u4), ("duplicated_count", u4), ("error_count", u4), ("stable_latency_ms", u4, (5,)),
                              ("op_count", u4), ("ok_count", u4), ("fail_count", u4), ("info_count", u4)]),
        "LIN_KEY_DT": np.dtype([("key", u4), ("valid", u4), ("op_row", u4), ("previous_ok_row", u4), ("n_pending", u4), ("n_values", u4),
                                ("values", "u1", (8,))]),
        "CYCLE_DT": np.dtype([("anomalies", u4), ("length", u4), ("n_steps", u4), ("reserved", u4)]),
        "CYCLE_STEP_DT": np.dtype([("txn", u4), ("inv_row", u4), ("cmp_row", u4), ("kinds", u4)]),
        "SET_ELEMENT_DT": element,
        "SET_EXPLAIN_DT": np.dtype([("n_lost", u4), ("n_never_read", u4), ("n_stale", u4), ("truncated", u4), ("n_worst_stale", u4),
                                    ("lost_latency_ms", u4, (5,)), ("worst_stale", element, (8,))]),
        "LATENCY_DT": latency,
        "F_STATS_DT": f_stats,
        "PERF_DT": np.dtype([("valid", u4), ("n_f", u4), ("count", u4), ("ok_count", u4), ("fail_count", u4), ("info_count", u4),
                             ("open_count", u4), ("flags", u4), ("by_f", f_stats, (4,))]),
    }


def test_every_dtype_engine_exports_equals_the_one_it_had():
    for name, dt in _hand_written_dtypes().items():
        got = getattr(E, name)
        assert got == dt and got.itemsize == dt.itemsize, name
        assert {n: (f[0], f[1]) for n, f in got.fields.items()} == {n: (f[0], f[1]) for n, f in dt.fields.items()}, name


def test_the_record_table_names_every_struct_of_the_header():
    closed = set(re.findall(r"^\}\s*(msim_[a-z0-9_]+);", HEADER, re.M))
    assert len(closed) == 16
    assert set(A.RECORDS) == closed | {"msim_latency_dist"}   # (a one-line typedef)


def _probe_source():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "maelsim.h"', "int main(void) {"]
    for name, st in A.RECORDS.items():
        lines.append(f'  printf("{name} - %zu 0\\n", sizeof({name}));')
        for field, _ in st._fields_:
            lines.append(f'  printf("{name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
    return "\n".join(lines + ["  return 0;", "}", ""])


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_records_match_the_header_in_ctypes_and_in_numpy(tmp_path):
    """A C program generated from RECORDS prints the header's sizeof / offsetof / field size of every record and field; ctypes and the
    numpy dtype derived from the Structure must say the same.  A field the header does not have does not compile."""
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(_probe_source())
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        name, field, a, b = line.split()
        st, (a, b) = A.RECORDS[name], (int(a), int(b))
        dt = np.dtype(st)
        if field == "-":
            assert C.sizeof(st) == a == dt.itemsize, line
        else:
            assert (getattr(st, field).offset, getattr(st, field).size) == (a, b), line
            assert (dt.fields[field][1], dt.fields[field][0].itemsize) == (a, b), line
        seen += 1
    assert seen == sum(1 + len(st._fields_) for st in A.RECORDS.values())
    # the one dtype kept beside its Structure: reserved[3] as r0, r1, r2
    assert E.META_DT.itemsize == C.sizeof(A.InstMeta)
    assert [E.META_DT.fields[n][1] for n in ("r0", "r1", "r2")] == [A.InstMeta.reserved.offset + 4 * i for i in range(3)]
    assert all(E.META_DT.fields[n][1] == getattr(A.InstMeta, n).offset for n, _ in A.InstMeta._fields_[:-1])


# ---- prototypes ----
def _declarations():
    """{entry: (return type, [parameter text ...])} of the header, comments stripped"""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decls = {}
    for ret, name, params in re.findall(r"^(int|uint32_t|void|const char \*)\s*(msim_[a-z0-9_]+)\(([^)]*)\);", text, re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        decls[name] = (ret, [] if params == ["void"] else params)
    return decls


def _c_class(param):
    if "*" in param or "[" in param:
        return "pointer"
    return {"uint32_t": "u32", "uint64_t": "u64", "size_t": "u64", "int": "int", "double": "double"}[" ".join(param.split()[:-1])]


def _ctypes_class(t):
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    assert C.sizeof(C.c_size_t) == 8
    return {C.c_uint32: "u32", C.c_uint64: "u64", C.c_size_t: "u64", C.c_int: "int", C.c_double: "double"}[t]


def test_prototypes_match_the_header():
    decls = _declarations()
    assert len(decls) == 63 and list(decls) == A.EXPORTS == list(A.PROTOTYPES)
    for name, (ret, params) in decls.items():
        restype, argtypes = A.PROTOTYPES[name]
        assert restype is {"int": C.c_int, "uint32_t": C.c_uint32, "const char *": C.c_char_p, "void": None}[ret], name
        assert [_ctypes_class(t) for t in argtypes] == [_c_class(p) for p in params], name


def test_load_applies_the_table_and_skips_what_the_library_lacks(lib, monkeypatch):
    for name, (restype, argtypes) in A.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    monkeypatch.setitem(A.PROTOTYPES, "msim_entry_of_a_later_build", (C.c_int, (C.c_void_p,)))
    monkeypatch.setattr(A, "_lib", None)
    older = A.load()   # as with MSIM_LIB naming a build from before the entry
    assert older.msim_abi_version() == A.ABI_VERSION
    with pytest.raises(AttributeError):
        older.msim_entry_of_a_later_build(None)


# ---- one convention: an array goes in as its address, a plain int ----
A_, R_, W_ = ":append", ":r", ":w"


def _ops(*ops):
    return [{"type": t, "process": p, "value": v} for t, p, v in ops]


def _record(entry, rows, payload, *model):
    res = A.CheckResult()
    addr = rows.ctypes.data, payload.ctypes.data
    assert all(type(a) is int for a in addr)
    assert getattr(A.load(), entry)(addr[0], len(rows), addr[1], len(payload), *model, C.byref(res)) == 0
    return res


def test_host_entries_take_plain_addresses(lib):
    # list-append (tests/test_txn_list_append.py): a lone completed append is clean; a read of a failed append is G1a
    rows, pay = E.encode_txn_history(_ops((":invoke", 0, [[A_, 1, 1]]), (":ok", 0, [[A_, 1, 1]])))
    res = _record("msim_check_txn_rows", rows, pay)
    assert (res.valid, res.error_count, res.attempt_count, res.ok_count) == (1, 0, 1, 1)
    got = E.check_txn_history(rows, pay)
    assert got["valid?"] is True and got["anomalies"] == [] and got["txn-count"] == 1
    rows, pay = E.encode_txn_history(_ops((":invoke", 0, [[A_, 1, 1]]), (":fail", 0, [[A_, 1, 1]]), (":invoke", 1, [[R_, 1, None]]), (":ok", 1, [[R_, 1, [1]]])))
    res = _record("msim_check_txn_rows", rows, pay)
    assert res.valid == 0 and res.error_count & 2
    got = E.check_txn_history(rows, pay)
    assert got["valid?"] is False and "G1a" in got["anomalies"] and got["anomaly-bits"] == res.error_count
    # rw-register (tests/test_txn_rw_register.py): a transaction that does not read its own write
    rows, pay = E.encode_txn_history(_ops((":invoke", 0, [[W_, 1, 1], [R_, 1, None]]), (":ok", 0, [[W_, 1, 1], [R_, 1, None]])), rw=True)
    assert _record("msim_check_rw_rows", rows, pay, A.CM_SNAPSHOT_ISOLATION).valid == 0
    res = _record("msim_check_rw_rows", rows, pay, A.CM_READ_COMMITTED)
    assert (res.valid, res.error_count) == (1, 64)
    got = E.check_rw_history(rows, pay, "snapshot-isolation")
    assert got["anomalies"] == ["internal"] and got["valid?"] is False
    assert E.check_rw_history(rows, pay, "read-committed")["valid?"] is True


def test_counter_and_id_entries_take_plain_addresses(lib):
    # pn-counter (pn_counter_test.clj:17-25 as tests/test_pn_counter.py has it, the read of 4 alone)
    rows = E.encode_pn_history([{"type": ":ok", "f": ":add", "value": 2}, {"type": ":ok", "f": ":add", "value": 3},
                                {"type": ":ok", "f": ":read", "final?": True, "value": 4}])
    res, ranges, n = A.CheckResult(), np.zeros(8, dtype=np.int64), np.zeros(1, dtype=np.uint32)
    assert lib.msim_check_pn_rows(rows.ctypes.data, len(rows), C.addressof(res), ranges.ctypes.data, 4, n.ctypes.data) == 0
    assert (res.valid, res.error_count, int(n[0]), ranges[:2].tolist()) == (0, 1, 1, [5, 5])
    got = E.check_pn_history(rows)
    assert got == {"valid?": False, "error-count": 1, "final-reads": [4], "acceptable": [[5, 5]]}
    # unique-ids (tests/test_unique_ids.py): 5 acknowledged twice
    rows = np.zeros(3, dtype=E.OP_DT)
    rows["packed"] = [A.T_OK | (A.F_GENERATE << 2) | (i << 12) for i in range(3)]
    rows["value"] = [5, 9, 5]
    res = A.CheckResult()
    assert lib.msim_check_unique_rows(rows.ctypes.data, len(rows), C.addressof(res)) == 0
    assert (res.valid, res.duplicated_count, res.ok_count, res.attempt_count, list(res.stable_latency_ms)[:2]) == (0, 1, 3, 0, [5, 9])


def test_anomaly_sets_need_no_restype_at_the_call_site(lib):
    models = (A.CM_READ_UNCOMMITTED, A.CM_READ_COMMITTED, A.CM_SNAPSHOT_ISOLATION, A.CM_SERIALIZABLE, A.CM_STRICT_SERIALIZABLE)
    sets = [lib.msim_proscribed_anomalies(m) for m in models]
    for weaker, stronger in zip(sets, sets[1:]):   # tests/test_txn_rw_register.py::test_proscribed_sets_nest
        assert weaker & stronger == weaker and weaker != stronger
    assert all(type(s) is int and s > 0 for s in sets)
    g_single_realtime, internal = 16 | 512, 64   # tests/test_elle_reference_vectors.py: what the docs' re-runs under weaker models say
    assert lib.msim_violated_anomalies(g_single_realtime, A.CM_STRICT_SERIALIZABLE) != 0
    assert lib.msim_violated_anomalies(g_single_realtime, A.CM_SERIALIZABLE) == 0
    assert lib.msim_violated_anomalies(internal, A.CM_SNAPSHOT_ISOLATION) != 0 and lib.msim_violated_anomalies(internal, A.CM_READ_COMMITTED) == 0


# ---- the marshalling helpers ----
def _rows(*values):
    r = np.zeros(len(values), dtype=E.OP_DT)
    r["time_len"] = [1000 * v for v in values]
    r["packed"] = [A.T_OK | (A.F_TXN << 2) | (v << 12) for v in values]
    r["value"] = values
    return r


H0, H1, H3 = _rows(), _rows(7), _rows(1, 2, 3)
WORDS = ([], [70], [10, 20, 30, 40])


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (g, w)


def test_offsets_form():
    cat = np.zeros(4, dtype=E.OP_DT)
    cat[0], cat[1:] = H1[0], H3
    off = np.array([0, 0, 1, 4], dtype=np.uint64)
    _same(E._offsets_form([H0, H1, H3], payload=False), (cat, off))
    with_words = [(h, np.array(w, dtype=np.uint32)) for h, w in zip((H0, H1, H3), WORDS)]
    _same(E._offsets_form(with_words), (cat, off, np.array([70, 10, 20, 30, 40], dtype=np.uint32), np.array([0, 0, 1, 5], dtype=np.uint64)))
    no_words = [(h, []) for h in (H0, H1, H3)]   # no payload word at all: one zero word, so that the entry gets a readable address
    _same(E._offsets_form(no_words), (cat, off, np.zeros(1, dtype=np.uint32), np.zeros(4, dtype=np.uint64)))
    _same(E._offsets_form([]), (np.zeros(0, dtype=E.OP_DT), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)))
    rows, off1 = E._offsets_form([H0, H0], payload=False)   # no rows stay no rows (explain_lin_kv_batch pads them itself)
    assert len(rows) == 0 and off1.tolist() == [0, 0, 0]


def test_slab_form():
    slab = np.zeros((3, 3), dtype=E.OP_DT)
    slab[1, 0], slab[2] = H1[0], H3
    n_rows = np.array([0, 1, 3], dtype=np.uint32)
    _same(E._slab_form([H0, H1, H3]), (slab, n_rows))
    wide = np.zeros((3, 5), dtype=E.OP_DT)
    wide[:, :3] = slab
    _same(E._slab_form([H0, H1, H3], max_rows=5), (wide, n_rows))
    words = np.array([[0, 0, 0, 0], [70, 0, 0, 0], [10, 20, 30, 40]], dtype=np.uint32)
    _same(E._slab_form(list(zip((H0, H1, H3), WORDS)), payload=True), (slab, n_rows, words))
    _same(E._slab_form([(h, []) for h in (H0, H1, H3)], payload=True), (slab, n_rows, np.zeros((3, 1), dtype=np.uint32)))
    _same(E._slab_form([H0]), (np.zeros((1, 1), dtype=E.OP_DT), np.zeros(1, dtype=np.uint32)))   # a slab is at least one row wide
    for empty in (lambda: E._slab_form([]), lambda: E._slab_form([], payload=True), lambda: E._set_full_slabs([], None)):
        with pytest.raises(ValueError):
            empty()
    _same(E._slab_form([], max_rows=4), (np.zeros((0, 4), dtype=E.OP_DT), np.zeros(0, dtype=np.uint32)))   # check_perf_batch(max_rows=...)


def test_set_full_slabs_derive_max_values():
    adds = np.zeros(40, dtype=E.OP_DT)
    adds["packed"] = A.T_INVOKE | (A.F_BROADCAST << 2)
    rows, n_rows, pay, max_values = E._set_full_slabs([(H3, [1]), (adds, [])], None)
    assert (rows.shape, n_rows.tolist(), pay.tolist(), max_values) == ((2, 40), [3, 40], [[1], [0]], 64)
    assert E._set_full_slabs([(H3, [1])], None)[3] == 32 and E._set_full_slabs([(adds, [])], 2048)[3] == 2048
