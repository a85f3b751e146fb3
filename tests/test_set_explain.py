"""The explained set-full verdicts on the host (msim_explain_set_full_rows, csrc/set_check.cpp; the contract: include/maelsim.h
msim_set_element / msim_set_explain) against tests/setfull_explain_ref.py — the definitions restated in pure Python — on the
tutorial's known answer, the healthy map, synthetic histories with all three classes and hand-written edges.  Needs no device;
tests/test_set_explain_gpu.py holds the device entries against this host entry byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import setfull_explain_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV = A.NO_VALUE


def host(h, max_elements=256, workload=A.WL_G_SET):
    """one host entry call on an encoded history -> (CHECK_DT record, SET_EXPLAIN_DT header, the whole slab of max_elements records)"""
    rows = np.ascontiguousarray(h[0]); pay = np.ascontiguousarray(h[1], dtype=np.uint32)
    out = np.zeros(1, dtype=E.CHECK_DT)
    hdr = np.full(E.SET_EXPLAIN_DT.itemsize // 4, 0xA5A5A5A5, dtype=np.uint32).view(E.SET_EXPLAIN_DT)   # (the entry clears what it does not write)
    slab = np.full(max(max_elements, 1) * 6, 0xA5A5A5A5, dtype=np.uint32).view(E.SET_ELEMENT_DT)
    rc = A.load().msim_explain_set_full_rows(workload, rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), out.ctypes.data_as(C.POINTER(A.CheckResult)),
                                             hdr.ctypes.data, slab.ctypes.data, max_elements)
    assert rc == 0, rc
    return out[0], hdr[0], slab[:max_elements]


def against_ref(ops, what, max_elements=256):
    """the host entry's record, header and slab of one history are the reference's, byte for byte"""
    out, hdr, slab = host(E.encode_set_history(ops), max_elements)
    want = X.record_of(ops)
    got = {k: ([int(x) for x in out[k]] if k == "stable_latency_ms" else int(out[k])) for k in want}
    assert got == want, (what, got, want)
    ref_hdr, ref_recs = X.explain(ops, max_elements)
    want_hdr, want_slab = X.as_arrays(ref_hdr, ref_recs, max_elements)
    assert hdr.tobytes() == want_hdr.tobytes(), (what, max_elements, hdr, want_hdr)
    assert slab.tobytes() == want_slab.tobytes(), (what, max_elements, slab[:8], want_slab[:8])
    return out, hdr, slab


def test_abi(lib):
    header = open(os.path.join(ROOT, "include", "maelsim.h")).read()
    for name in ("msim_explain_set_full_rows", "msim_explain_set_full_batch", "msim_explain_set_full"):
        assert name in A.EXPORTS and re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(lib, name)
    assert E.SET_ELEMENT_DT.itemsize == 24 and E.SET_EXPLAIN_DT.itemsize == 40 + 8 * 24
    assert lib.msim_abi_version() == 1
    assert "[upstream, unpinned" in header and "LARGER element first" in header


def test_the_tutorials_known_answer(lib):
    """01-broadcast.md:423-437: attempt 21, stable 1, :stale (8), :lost = 0..20 without 8"""
    ops = X.tutorial()
    out, hdr, slab = against_ref(ops, "tutorial")
    assert (int(out["attempt_count"]), int(out["stable_count"]), int(out["stale_count"]), int(out["lost_count"]), int(out["valid"])) == (21, 1, 1, 20, 0)
    rows, pay = E.encode_set_history(ops)
    m = E.set_full_analysis(out, hdr, slab[:21], rows, pay, n_nodes=5)
    assert m["stale"] == [8] and m["lost"] == [e for e in range(21) if e != 8] and m["never-read"] == [] and m["valid?"] is False
    assert [w["element"] for w in m["worst-stale"]] == [8]
    w = m["worst-stale"][0]
    # 8 was acknowledged by its broadcast_ok and last missed by the read process 1 invoked (the latest-invoked read but process 4's)
    assert w["known"]["f"] == ":broadcast" and w["known"]["type"] == ":ok" and w["known"]["value"] == 8
    assert w["last-absent"]["f"] == ":read" and w["last-absent"]["type"] == ":invoke" and w["last-absent"]["process"] == 1
    assert w["outcome"] == "stable" and w["stable-latency"] > 0 and set(m["lost-latencies"]) == {0, 0.5, 0.95, 0.99, 1}
    # every lost element was last seen by the read of its own node and last missed by process 4's read, the last invoked
    last_inv = max(op["index"] for op in ops if op["type"] == ":invoke")
    assert all(int(e["last_absent_row"]) == last_inv and int(e["last_present_row"]) != NV for e in slab[:20])
    # without rows: the row indices
    m = E.set_full_analysis(out, hdr, slab[:21])
    assert m["worst-stale"][0]["known"] == 2 * 8 + 1 and ops[m["worst-stale"][0]["last-absent"]]["process"] == 1


def test_the_healthy_map(lib):
    """:564-577: exactly the documented key set, empty lists, :worst-stale ()"""
    ops = X.healthy(32)
    out, hdr, slab = against_ref(ops, "healthy")
    m = E.set_full_analysis(out, hdr, slab[:0])
    assert set(m) == {"worst-stale", "duplicated-count", "valid?", "lost-count", "lost", "stable-count", "stale-count", "stale", "never-read-count",
                      "stable-latencies", "attempt-count", "never-read", "duplicated"}
    assert m == {"worst-stale": [], "duplicated-count": 0, "valid?": True, "lost-count": 0, "lost": [], "stable-count": 32, "stale-count": 0, "stale": [],
                 "never-read-count": 0, "stable-latencies": {0: 0, 0.5: 0, 0.95: 0, 0.99: 0, 1: 0}, "attempt-count": 32, "never-read": [], "duplicated": {}}
    assert not hdr.tobytes().strip(b"\0")


@pytest.mark.parametrize("seed", list(X.SYNTH))
def test_synthetic_histories(lib, seed):
    make, _, want = X.SYNTH[seed]
    ops = make()
    assert len(ops) == want["rows"]
    for max_elements in (256, 7, 0):
        out, hdr, slab = against_ref(ops, seed, max_elements)
        assert (int(out["stable_count"]), int(out["lost_count"]), int(out["never_read_count"]), int(out["stale_count"])) == \
            (want["stable"], want["lost"], want["never"], want["stale"]), out
    if seed == 7006:
        assert int(out["valid"]) in (0, 2)


def test_the_large_history(lib):
    make, _, want = X.BIG
    ops = make()
    out, hdr, slab = against_ref(ops, "7003", 1408)
    assert (int(hdr["n_lost"]), int(hdr["n_never_read"]), int(hdr["n_stale"]), int(hdr["truncated"])) == (want["lost"], want["never"], want["stale"], 0)
    out, hdr, slab = against_ref(ops, "7003", 64)   # truncation falls inside the never-read segment
    assert (int(hdr["n_lost"]), int(hdr["n_never_read"]), int(hdr["n_stale"]), int(hdr["truncated"])) == (19, 45, 0, 1)


EDGES = X.edges()


@pytest.mark.parametrize("name", list(EDGES))
def test_hand_written_edges(lib, name):
    ops = EDGES[name]
    out, hdr, slab = against_ref(ops, name)
    n_lost, n_never, n_stale = int(out["lost_count"]), int(out["never_read_count"]), int(out["stale_count"])
    # max_elements of 0, exactly n_lost, n_lost + 1, n_lost + n_never, and one short of everything
    for m in sorted({0, n_lost, n_lost + 1, n_lost + n_never, max(0, n_lost + n_never + n_stale - 1)}):
        _, h, _ = against_ref(ops, name, m)
        assert int(h["truncated"]) == (1 if m < n_lost + n_never + n_stale else 0)
        assert int(h["n_lost"]) + int(h["n_never_read"]) + int(h["n_stale"]) == min(m, n_lost + n_never + n_stale)
    rec = lambda e: tuple(int(x) for x in e.tolist())
    if name == "no elements":
        assert int(out["attempt_count"]) == 0 and int(out["valid"]) == 2 and not hdr.tobytes().strip(b"\0")
    elif name.endswith(" elements"):
        lost, never, stale = X.BLOCKS[int(name.split()[0])]
        assert [int(e["element"]) for e in slab[:n_lost + n_never + n_stale]] == lost + never + stale
    elif name == "classes in the second block only":
        assert [int(e["element"]) for e in slab[:6]] == [64, 99, 65, 98, 66, 97]
    elif name.endswith(" stale") and name[0] in "789":
        k = int(name[0])
        stale = list(range(3, 3 + 7 * k, 7))
        assert n_stale == k and int(hdr["n_worst_stale"]) == min(k, 8)
        assert [int(e["element"]) for e in hdr["worst_stale"][:min(k, 8)]] == stale[::-1][:8]   # latency 5 + e: descending elements
        assert [int(e["latency_ms"]) for e in hdr["worst_stale"][:min(k, 8)]] == [5 + e for e in stale[::-1][:8]]
    elif name == "nine equal stale":
        assert n_stale == 9 and {int(e["latency_ms"]) for e in slab[:9]} == {9}
        assert [int(e["element"]) for e in hdr["worst_stale"]] == list(range(2, 70, 8))[::-1][:8]   # ties: the larger element first
    elif name == "known is a read":
        assert n_lost + n_never + n_stale == 0 and int(out["stable_count"]) == 1
        assert X.element_records(ops)[0] == (0, X.STABLE, 0, 3, 4, NV)   # known = the first read's :ok row
    elif name == "no known":
        assert rec(slab[0]) == (1, A.SET_NEVER_READ, NV, NV, NV, NV) and n_never == 1
    elif name == "lost never present":
        assert rec(slab[0]) == (0, A.SET_LOST, 0, 1, NV, 4) and [int(x) for x in hdr["lost_latency_ms"]] == [0] * 5 and int(out["valid"]) == 0
    else:
        raise AssertionError(name)


def test_refusals(lib):
    """echo and every non-set workload: MSIM_E_UNSUPPORTED; missing arrays: MSIM_E_INVALID"""
    rows, pay = E.encode_set_history(X.healthy(3))
    out = np.zeros(1, dtype=E.CHECK_DT); hdr = np.zeros(1, dtype=E.SET_EXPLAIN_DT); slab = np.zeros(4, dtype=E.SET_ELEMENT_DT)
    call = lambda wl, h=hdr.ctypes.data, s=slab.ctypes.data, m=4: lib.msim_explain_set_full_rows(
        wl, rows.ctypes.data, len(rows), pay.ctypes.data, len(pay), out.ctypes.data_as(C.POINTER(A.CheckResult)), h, s, m)
    for wl in (A.WL_ECHO, A.WL_LIN_KV, A.WL_TXN_LIST_APPEND, A.WL_PN_COUNTER, A.WL_KAFKA):
        assert call(wl) == -6, wl
    assert call(A.WL_BROADCAST) == 0 and call(A.WL_G_SET) == 0
    assert call(A.WL_G_SET, h=None) == -1 and call(A.WL_G_SET, s=None) == -1 and call(A.WL_G_SET, s=None, m=0) == 0
    with pytest.raises(E.EngineError, match="-6"):
        E.explain_set_full_history(rows, pay, workload=A.WL_ECHO)
    rec, h, els = E.explain_set_full_history(rows, pay, workload=A.WL_BROADCAST)
    assert int(rec["stable_count"]) == 3 and len(els) == 0 and int(h["truncated"]) == 0
