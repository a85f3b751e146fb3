"""The witness cycle of the transactional verdicts on the host (msim_explain_txn_rows / msim_explain_rw_rows, csrc/txn_check.cpp;
the contract: include/maelsim.h msim_cycle_result) against tests/txn_witness_ref.py — the definition restated in pure Python over an
edge map built independently — and against cycles written out by hand.  Needs no device; tests/test_txn_explain_gpu.py holds the device
entries against these host entries byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import test_rw_classify_gpu as RWT
import test_txn_classify_gpu as T
import txn_witness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = T.MODELS
WW, WR, RW, RT = 1, 2, 4, 8
NV = A.NO_VALUE


def host(h, model="strict-serializable", max_steps=64, rw=False):
    """one host entry call -> (CHECK_DT record, CYCLE_DT record, the whole slab of max_steps CYCLE_STEP_DT)"""
    rows = np.ascontiguousarray(h[0]); pay = np.ascontiguousarray(h[1], dtype=np.uint32)
    out = np.zeros(1, dtype=E.CHECK_DT); cyc = np.zeros(1, dtype=E.CYCLE_DT)
    steps = np.full(max_steps, 0xA5A5A5A5, dtype=np.uint32).repeat(4).view(E.CYCLE_STEP_DT)   # (the entry clears what it does not write)
    fn = A.load().msim_explain_rw_rows if rw else A.load().msim_explain_txn_rows
    rc = fn(rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), E.CONSISTENCY_MODELS[model], out.ctypes.data_as(C.POINTER(A.CheckResult)),
            cyc.ctypes.data, steps.ctypes.data, max_steps)
    assert rc == 0, rc
    return out[0], cyc[0], steps


def against_ref(ops, h, what, rw=False, max_steps=1024):
    """the host entry's witness of one history = the reference's, and it verifies against the reference's edge map"""
    txns, edges = (R.edges_rw if rw else R.edges_list_append)(ops)
    bits, cycle = R.witness(edges)
    out, cyc, steps = host(h, max_steps=max_steps, rw=rw)
    cycle_bits = int(out["error_count"]) & (R.G0 | R.G1C | R.G_SINGLE | R.G2 | R.REALTIME)
    assert int(cyc["anomalies"]) == bits == cycle_bits, (what, int(cyc["anomalies"]), bits, cycle_bits)
    assert int(cyc["length"]) == len(cycle) and int(cyc["n_steps"]) == min(len(cycle), max_steps) and int(cyc["reserved"]) == 0, (what, cyc, len(cycle))
    got = [(int(s["txn"]), int(s["inv_row"]), int(s["cmp_row"]), int(s["kinds"])) for s in steps[:int(cyc["n_steps"])]]
    want = [(t, txns[t]["inv"], txns[t]["cmp"], k) for t, k in cycle][:max_steps]
    assert got == want, (what, got, want)
    assert not steps[int(cyc["n_steps"]):].tobytes().strip(b"\0"), what
    if bits and len(cycle) <= max_steps:
        assert R.verify(edges, int(cyc["anomalies"]), [(t, k) for t, _, _, k in got])
    return out, cyc, steps


# the eight cycle cases of test_txn_classify_gpu.HAND: (txn, :invoke row, completion row, kinds) per step, derived by hand
HAND_CYCLES = {
    "G0": [(0, 0, 2, WW), (1, 1, 3, WW)],                          # key 1: T0 before T1, key 2: T1 before T0
    "G1c": [(0, 0, 2, WR), (1, 1, 3, WR)],                         # each read the other's append
    "G-single": [(0, 0, 2, WR), (1, 1, 3, RW)],                    # T1 read T0's append of key 1 and missed the one of key 2
    "G2": [(0, 0, 2, RW), (1, 1, 3, RW)],                          # write skew
    "G0-realtime": [(0, 0, 1, RT), (1, 2, 3, WW)],                 # T0 completed before T1 began; key 1 has T1's element first
    "G1c-realtime": [(0, 0, 1, RT), (1, 2, 3, WR)],                # T0 read what T1 appended later
    "G-single-realtime": [(0, 0, 1, RT), (1, 2, 3, RW)],           # the stale read T1 follows T0 and misses its append
    "G2-realtime": [(0, 0, 5, RW), (1, 1, 2, RT), (2, 3, 4, RW)],  # process 1's transaction -rw-> process 2's -realtime-> process 0's -rw-> back
}


@pytest.mark.parametrize("name", list(HAND_CYCLES))
def test_hand_written_cycles(lib, name):
    ops, want_names = T.HAND[name]
    h = T.HAND_HS[list(T.HAND).index(name)]
    out, cyc, steps = against_ref(T._ops(*ops), h, name)
    assert {n for b, n in A.ANOMALIES.items() if int(cyc["anomalies"]) & b} == want_names
    want = HAND_CYCLES[name]
    assert int(cyc["length"]) == len(want) == int(cyc["n_steps"])
    assert [(int(s["txn"]), int(s["inv_row"]), int(s["cmp_row"]), int(s["kinds"])) for s in steps[:len(want)]] == want
    plain = T.S._host(*h)
    assert bytes(plain) == out.tobytes(), name          # *out is what msim_check_txn_rows writes
    got = E.explain_txn_history(h[0], h[1])
    assert got[1].tobytes() == cyc.tobytes() and got[2].tobytes() == steps[:len(want)].tobytes()


def test_no_cycle_is_the_zero_record(lib):
    """every hand-made history without a cycle has the all-zero record and no step; two-kinds (a cycle beside a G1a) that of plain G2"""
    names = list(T.HAND)
    for name in names:
        if name in HAND_CYCLES or name == "two-kinds":
            continue
        out, cyc, steps = against_ref(T._ops(*T.HAND[name][0]), T.HAND_HS[names.index(name)], name)
        assert not cyc.tobytes().strip(b"\0") and not steps.tobytes().strip(b"\0"), name
    assert {"empty", "all-fail"} <= set(names) - set(HAND_CYCLES)
    two = host(T.HAND_HS[names.index("two-kinds")])
    g2 = host(T.HAND_HS[names.index("G2")])
    assert two[1].tobytes() == g2[1].tobytes() and two[2].tobytes() == g2[2].tobytes() and int(two[1]["length"]) == 2
    assert T.S._names(two[0]["error_count"]) == {"G2", "G1a"} and int(two[1]["anomalies"]) == R.G2


@pytest.mark.parametrize("i,s", list(enumerate((16, 17, 255, 256, 257, 600))))
def test_chains_and_truncation(lib, i, s):
    """a realtime chain closed by one anti-dependency: the witness is the whole component; max_steps 8 truncates it (length kept, the rest
    of the slab zero), 1024 holds it and it verifies"""
    h = T.CHAINS[i]
    out, cyc, steps = host(h, max_steps=1024)
    assert int(cyc["anomalies"]) == R.G_SINGLE | R.REALTIME and int(cyc["length"]) == s == int(cyc["n_steps"]) == int(out["stale_count"])
    assert [int(x) for x in steps["txn"][:s]] == list(range(s)) and (steps["kinds"][:s - 1] == RT).all() and int(steps["kinds"][s - 1]) == RW
    assert (steps["inv_row"][:s] == 2 * np.arange(s)).all() and (steps["cmp_row"][:s] == 2 * np.arange(s) + 1).all()
    assert not steps[s:].tobytes().strip(b"\0")
    ops = E.decode_history(h[0], h[1], 0, A.WL_TXN_LIST_APPEND)
    _, edges = R.edges_list_append(ops)
    assert R.verify(edges, int(cyc["anomalies"]), list(zip((int(x) for x in steps["txn"][:s]), (int(x) for x in steps["kinds"][:s]))))
    out8, cyc8, steps8 = host(h, max_steps=8)
    assert out8.tobytes() == out.tobytes() and int(cyc8["length"]) == s and int(cyc8["n_steps"]) == 8 and int(cyc8["anomalies"]) == int(cyc["anomalies"])
    assert steps8.tobytes() == steps[:8].tobytes()
    _, cyc1, steps1 = host(h, max_steps=1)
    assert int(cyc1["n_steps"]) == 1 and steps1.tobytes() == steps[:1].tobytes()


def _models_agree(h, rw, plain_strict):
    """the five models: only `valid` of the check record varies; the witness does not"""
    base = host(h, "strict-serializable", 256, rw)
    for model in MODELS:
        out, cyc, steps = host(h, model, 256, rw)
        assert cyc.tobytes() == base[1].tobytes() and steps.tobytes() == base[2].tobytes(), model
        a, b = out.copy(), base[0].copy()
        a["valid"] = b["valid"] = 0
        assert a.tobytes() == b.tobytes(), model
        bits = int(out["error_count"])
        want = 0 if T._violates(bits, model) else (2 if int(out["ok_count"]) == 0 else 1)
        assert int(out["valid"]) == want, (model, int(out["valid"]), want)
    assert base[0].tobytes() == plain_strict


def test_store_without_isolation_against_the_reference(lib):
    """test_txn_classify_gpu's 64 histories of a store without isolation (every cycle class, components past 64): the reference's witness"""
    seen = set()
    for i, (ops, h) in enumerate(zip(T._no_isolation_ops(), T._no_isolation_hs())):
        out, cyc, _ = against_ref(ops, h, ("no isolation", i))
        seen.add(int(cyc["anomalies"]))
        _models_agree(h, False, bytes(T.S._host(*h)))
    assert {R.G0, R.G1C, R.G_SINGLE, R.G2} <= {b & ~R.REALTIME for b in seen} and any(b & R.REALTIME for b in seen), seen


def test_rw_register_against_the_reference(lib):
    """test_rw_classify_gpu's hand-made histories and its 240 random ones with reads from the future, through msim_explain_rw_rows"""
    seen = set()
    sets = [(list(RWT.HAND), [ops for ops, _ in RWT.HAND.values()], RWT.HAND_HS),
            (list(range(240)), [RWT._case(s) for s in range(240)], RWT._random_hs())]
    for names, all_ops, hs in sets:
        strict = RWT._host(hs, "strict-serializable")
        for name, ops, h, plain in zip(names, all_ops, hs, strict):
            out, cyc, steps = against_ref(ops, h, ("rw", name), rw=True)
            seen.add(int(cyc["anomalies"]))
            if isinstance(name, str) or name % 8 == 0:
                _models_agree(h, True, plain.tobytes())
            else:
                assert out.tobytes() == plain.tobytes(), name
            got = E.explain_rw_history(h[0], h[1], max_steps=1024)
            assert got[1].tobytes() == cyc.tobytes() and got[2].tobytes() == steps[:int(cyc["n_steps"])].tobytes()
    assert {0, R.G0, R.G1C, R.G_SINGLE, R.G2} <= {b & ~R.REALTIME for b in seen} and any(b & R.REALTIME for b in seen), seen


def test_analysis_formatting(lib):
    """txn_cycle_analysis: elle's :anomalies map from the record, the ops from decode_history"""
    names = list(T.HAND)
    h = T.HAND_HS[names.index("G-single-realtime")]
    _, cyc, steps = E.explain_txn_history(h[0], h[1])
    got = E.txn_cycle_analysis(h[0], h[1], cyc, steps)
    ops = E.decode_history(h[0], h[1], 0, A.WL_TXN_LIST_APPEND)
    assert got == {"anomalies": {"G-single-realtime": [{"cycle": [ops[1], ops[3]], "steps": [{"type": "realtime"}, {"type": "rw"}]}]}}
    h = T.HAND_HS[names.index("empty")]
    _, cyc, steps = E.explain_txn_history(h[0], h[1])
    assert E.txn_cycle_analysis(h[0], h[1], cyc, steps) == {"anomalies": {}}
    h = T.CHAINS[0]
    _, cyc, steps = E.explain_txn_history(h[0], h[1], max_steps=4)
    got = E.txn_cycle_analysis(h[0], h[1], cyc, steps)["anomalies"]["G-single-realtime"][0]
    assert got["truncated"] == 16 and len(got["cycle"]) == 4 and got["steps"] == [{"type": "realtime"}] * 4


ENTRIES = ["msim_explain_txn_rows", "msim_explain_rw_rows", "msim_explain_txn_batch", "msim_explain_rw_batch", "msim_explain_txn"]


def test_entries_are_declared_exported_and_prototyped(lib):
    header = open(os.path.join(ROOT, "include", "maelsim.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in A.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    for text in ("typedef struct msim_cycle_result", "typedef struct msim_cycle_step", "MSIM_EDGE_WW = 1u, MSIM_EDGE_WR = 2u, MSIM_EDGE_RW = 4u, MSIM_EDGE_RT = 8u"):
        assert text in header, text
    assert E.CYCLE_DT.itemsize == 16 and E.CYCLE_STEP_DT.itemsize == 16
    assert A.EDGE_KINDS == {1: "ww", 2: "wr", 4: "rw", 8: "realtime"}


def test_entries_refuse_null_zero_and_bad_arguments(lib):
    rows, pay = T.HAND_HS[0]
    rows = np.ascontiguousarray(rows); pay = np.ascontiguousarray(pay, dtype=np.uint32)
    out = np.zeros(1, dtype=E.CHECK_DT); cyc = np.zeros(1, dtype=E.CYCLE_DT); steps = np.zeros(4, dtype=E.CYCLE_STEP_DT)
    o = out.ctypes.data_as(C.POINTER(A.CheckResult))
    for fn in (lib.msim_explain_txn_rows, lib.msim_explain_rw_rows):
        good = [rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), 0, o, cyc.ctypes.data, steps.ctypes.data, 4]
        for at, bad in ((0, None), (2, None), (4, 5), (5, None), (6, None), (7, None), (8, 0)):
            args = list(good); args[at] = bad
            assert fn(*args) == A.E_INVALID, (fn, at)
    ro = np.asarray([0, len(rows)], dtype=np.uint64); po = np.asarray([0, len(pay)], dtype=np.uint64)
    nh = C.c_uint32()
    for fn in (lib.msim_explain_txn_batch, lib.msim_explain_rw_batch):      # (refused before any device is touched)
        good = [0, rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, 1, 0, out.ctypes.data, C.byref(nh), cyc.ctypes.data, steps.ctypes.data, 4]
        for at, bad in ((1, None), (2, None), (4, None), (5, 0), (6, 5), (7, None), (9, None), (10, None), (11, 0)):
            args = list(good); args[at] = bad
            assert fn(*args) == A.E_INVALID, (fn, at)
    assert lib.msim_explain_txn(None, cyc.ctypes.data, steps.ctypes.data, 4, 1) == A.E_INVALID
