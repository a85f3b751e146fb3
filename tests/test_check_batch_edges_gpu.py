"""The edges of the device checkers' batch entries that the other tests reach only in passing (the host side of csrc/*_check_dev.hip:
the upload of a caller's histories, the chunked launches, the hand-off to the host checkers): histories with zero rows at the front, in
the middle and at the end of a batch, a history with rows and no payload words, a batch whose whole payload is empty, and the record of
a history that the device hands to the host — it must be the one that comes back, and n_host must count it.  Every entry against its
host `_rows` twin, record by record, byte for byte.

Each entry gets FIVE = [no rows, handed to the host, no rows, rows without payload words, no rows] (the slab entries, which carry no
payload: an ordinary history in the fourth place), BARE = FIVE with the second history without payload words too, and NINE = FIVE + four
ordinary histories.  Under MSIM_DEV_FLAGS 0x10000 (test_chunked, a child process: the batch entries read the switch once) a launch takes
at most 7 histories: FIVE is one partial chunk, NINE reaches first > 0.  The histories are those of the other tests, none beyond 40 rows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import kafka_classify_cases as KC
import lin_explain_cases as LK
import test_rw_classify_gpu as RWT
import test_txn_classify_gpu as T
from test_kafka_classify_gpu import BAD_HS, GOOD_HS, T_BOUND, _at_offset
from test_perf_stats_gpu import synth
from test_pn_check_synthetic_gpu import final, info_add, ok_add
from test_txn_explain import host as explain_host
import perf_ref

pytestmark = pytest.mark.gpu

DEV_FLAGS = int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0)
NO_ROWS = np.zeros(0, dtype=E.OP_DT)
NO_WORDS = np.zeros(0, dtype=np.uint32)
EMPTY = (NO_ROWS, NO_WORDS)


def _record(fn, *args):
    """one host `_rows` entry -> the CHECK_DT record it fills (a history without rows or words still hands in a readable address)"""
    res = A.CheckResult()
    assert fn(*args, C.byref(res)) == 0
    return np.frombuffer(bytes(res), dtype=E.CHECK_DT)[0]


def _addr(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return (a if len(a) else np.zeros(1, dtype=dtype)).ctypes.data_as(C.c_void_p), len(a)


def _sets(handed, bare, ordinary, pad=EMPTY):
    """(FIVE, BARE, NINE) of one entry family: `handed` goes to the host, `bare` has rows and no payload words"""
    five = (pad, handed, pad, bare, pad)
    return five, (pad, bare, pad, bare, pad), five + tuple(ordinary)


def _same(dev, want, what):
    assert len(dev) == len(want)
    for i in range(len(want)):
        assert bytes(dev[i]) == bytes(want[i]), (what, i, dev[i], want[i])


def _small(hs):
    assert all(len(h[0] if isinstance(h, tuple) else h) <= 40 for h in hs), [len(h[0] if isinstance(h, tuple) else h) for h in hs]
    return hs


# ---- txn-list-append: a (key, element) appended twice is the host's; a transaction without micro-ops has no payload words ----
TXN = _sets(T._twice_appended(), E.encode_txn_history(T._ops(*T._pair(0, []), *T._pair(1, []))), T.HAND_HS[:4])


def _txn_host(h):
    (r, n), (p, w) = _addr(h[0], E.OP_DT), _addr(h[1], np.uint32)
    return _record(A.load().msim_check_txn_rows, r, n, p, w)


@pytest.mark.parametrize("which", range(3))
def test_txn(lib, which):
    hs = _small(TXN[which])
    want = [_txn_host(h) for h in hs]
    _same(E.check_txn_batch(list(hs)), want, "msim_check_txn_batch")
    dev, n_host = E.classify_txn_batch(list(hs))
    _same(dev, want, "msim_classify_txn_batch")
    assert n_host == (0 if which == 1 else 1), n_host
    out, cyc, steps, n_host = E.explain_txn_batch(list(hs), max_steps=8)
    assert n_host == (0 if which == 1 else 1), n_host
    for i, h in enumerate(hs):
        o, c, s = explain_host(h if len(h[1]) else (h[0], np.zeros(1, dtype=np.uint32)), max_steps=8)
        assert bytes(out[i]) == bytes(o) == bytes(want[i]) and bytes(cyc[i]) == bytes(c) and steps.slab[i].tobytes() == s.tobytes(), ("msim_explain_txn_batch", i, out[i], o, cyc[i], c)


# ---- txn-rw-register: a value written twice to one key is the host's ----
_W11 = [RWT._w(1, 1)]
RW = _sets(E.encode_txn_history(RWT._ops((0, ":ok", _W11, _W11), (1, ":ok", _W11, _W11)), rw=True),
           E.encode_txn_history(RWT._ops((0, ":ok", [], []), (1, ":ok", [], [])), rw=True), RWT.HAND_HS[:4])
MODEL = "serializable"


def _rw_host(h):
    (r, n), (p, w) = _addr(h[0], E.OP_DT), _addr(h[1], np.uint32)
    return _record(A.load().msim_check_rw_rows, r, n, p, w, E.CONSISTENCY_MODELS[MODEL])


@pytest.mark.parametrize("which", range(3))
def test_rw(lib, which):
    hs = _small(RW[which])
    want = [_rw_host(h) for h in hs]
    handed = 0 if which == 1 else 1
    dev, n_host = E.classify_rw_batch(list(hs), MODEL)
    _same(dev, want, "msim_classify_rw_batch")
    assert n_host == handed, n_host
    dev, n_host = E.check_rw_batch(list(hs), MODEL)
    assert n_host == handed, n_host
    for i, (g, h) in enumerate(zip(dev, want)):
        if bytes(g) != bytes(h):   # the first pass's own record, only of a history it proved valid: tests/test_rw_classify_gpu.py, _both_entries
            assert int(g["valid"]) == int(h["valid"]) != 0 and int(g["error_count"]) & ~int(h["error_count"]) == 0 and int(g["stale_count"]) == 0, ("msim_check_rw_batch", i, g, h)
            assert all(int(g[f]) == int(h[f]) for f in ("attempt_count", "stable_count", "op_count", "ok_count", "fail_count", "info_count")), ("msim_check_rw_batch", i, g, h)
    out, cyc, steps, n_host = E.explain_rw_batch(list(hs), MODEL, max_steps=8)
    assert n_host == handed, n_host
    for i, h in enumerate(hs):
        o, c, s = explain_host(h if len(h[1]) else (h[0], np.zeros(1, dtype=np.uint32)), MODEL, max_steps=8, rw=True)
        assert bytes(out[i]) == bytes(o) == bytes(want[i]) and bytes(cyc[i]) == bytes(c) and steps.slab[i].tobytes() == s.tobytes(), ("msim_explain_rw_batch", i, out[i], o, cyc[i], c)


# ---- kafka: the plain entry hands every unclean history to the host, the classifying one what names an offset from 1152 on; sends
# carry no payload words ----
def _no_words(h):
    assert not any((int(t) >> 48) for t in h[0]["time_len"])
    return h[0], NO_WORDS


KAFKA = _sets(E.encode_kafka_history(_at_offset(T_BOUND)), _no_words(KC.raw_history(("send", A.T_INVOKE, 0, 1, 5, 0x7FF), ("send", A.T_OK, 0, 1, 5, 0))),
              [BAD_HS["dup"], GOOD_HS[next(iter(GOOD_HS))], KC.order_vectors()["A rev"], KC.order_vectors()["B fwd"]])


def _kafka_host(h):
    (r, n), (p, w) = _addr(h[0], E.OP_DT), _addr(h[1], np.uint32)
    return _record(A.load().msim_check_kafka_rows, r, n, p, w)


@pytest.mark.parametrize("which", range(3))
def test_kafka(lib, which):
    hs = _small(KAFKA[which])
    want = [_kafka_host(h) for h in hs]
    dev, n_host = E.check_kafka_batch(list(hs), 3)
    _same(dev, want, "msim_check_kafka_batch")
    assert n_host == sum(int(w["error_count"]) != 0 or int(w["valid"]) == 0 for w in want) and (n_host >= 1 or which == 1), n_host
    dev, n_host = E.classify_kafka_batch(list(hs), 3)
    _same(dev, want, "msim_classify_kafka_batch")
    assert n_host == (0 if which == 1 else 1), n_host


# ---- lin-kv (rows only): no history this small outgrows the device search; with the tiny pools of MSIM_DEV_FLAGS 0x2000 (test_tiny_pools)
# nine overlapping writes do, and the host search finishes them ----
LIN = _sets(LK.encode(LK.wide_then_bad_read(9, 3, 99, 0)), LK.encode(LK.HAND["a stale read"][0]),
            [LK.encode(LK.HAND[k][0]) for k in ("sequential and valid", "two interleaved keys, one bad", "an :info write stays open", "an open write beside the failing read")],
            pad=NO_ROWS)


@pytest.mark.parametrize("which", range(3))
def test_lin_kv(lib, which):
    hs = _small(LIN[which])
    want = [E.explain_lin_kv_history(h if len(h) else np.zeros(1, dtype=E.OP_DT)[:0]) for h in hs]
    _same(E.check_lin_kv_batch(list(hs)), [w[0] for w in want], "msim_check_lin_kv_batch")
    res, n_host = E.explain_lin_kv_batch(list(hs), with_n_host=True)
    _same([r[0] for r in res], [w[0] for w in want], "msim_explain_lin_kv_batch")
    for i, ((_, keys), (_, hkeys)) in enumerate(zip(res, want)):
        assert keys.tobytes() == hkeys.tobytes(), (i, keys, hkeys)
    assert n_host == (1 if DEV_FLAGS & 0x2000 and which != 1 else 0), n_host


# ---- pn-counter (slabs): a window of acceptable sums wider than 4096 is the host's ----
PN = _sets(E.encode_pn_history([ok_add(7), info_add(5000), final(7), final(5007), final(9)]), E.encode_pn_history([ok_add(1), info_add(2), final(3), final(2)]),
           [E.encode_pn_history(ops) for ops in ([ok_add(1)], [info_add(-3), final(-3), final(1)], [ok_add(2)] * 39, [final(0)])], pad=NO_ROWS)


def _pn_host(h):
    r, n = _addr(h, E.OP_DT)
    res = A.CheckResult()
    assert A.load().msim_check_pn_rows(r, n, C.byref(res), None, 0, None) == 0
    return np.frombuffer(bytes(res), dtype=E.CHECK_DT)[0]


@pytest.mark.parametrize("which", (0, 2))
def test_pn(lib, which):
    hs = _small(PN[which])
    _same(E.check_pn_batch(list(hs)), [_pn_host(h) for h in hs], "msim_check_pn_batch")


# ---- unique-ids and :stats / :perf (slabs, complete on the device) ----
def _ids(*acks):
    rows = np.zeros(2 * len(acks), dtype=E.OP_DT)
    for i, v in enumerate(acks):
        rows[2 * i] = (2000 * i, A.T_INVOKE | (A.F_GENERATE << 2) | ((i % 3) << 12), A.NO_VALUE)
        rows[2 * i + 1] = (2000 * i + 1000, A.T_OK | (A.F_GENERATE << 2) | ((i % 3) << 12), v)
    return rows


UNIQUE = _sets(_ids(5, 6, 5, 7), _ids(1, 2, 3), [_ids(9), _ids(*range(20)), _ids(4, 4, 4), _ids(0xFFFFFFFF, 0xFFFFFFFF)], pad=NO_ROWS)


@pytest.mark.parametrize("which", (0, 2))
def test_unique(lib, which):
    hs = _small(UNIQUE[which])
    want = [_record(A.load().msim_check_unique_rows, *_addr(h, E.OP_DT)) for h in hs]
    _same(E.check_unique_batch(list(hs)), want, "msim_check_unique_batch")


PERF = _sets(perf_ref.rows_of(synth(3, 18, 3)), perf_ref.rows_of(synth(4, 20, 3, p_never=0.2)), [perf_ref.rows_of(synth(10 + i, 5 + 5 * i, 3)) for i in range(4)], pad=NO_ROWS)


@pytest.mark.parametrize("which", (0, 2))
def test_perf(lib, which):
    hs = _small(PERF[which])
    for window_s, n_windows in ((None, 0), (0.01, 4)):
        got = E.check_perf_batch(list(hs), 3, window_s, n_windows)
        for i, h in enumerate(hs):
            assert got[i] == E.check_perf_rows(h, 3, window_s, n_windows), ("msim_check_perf_batch", i, n_windows)


def _child(flags, select, passed):
    assert DEV_FLAGS == 0
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", select],
                       env=dict(os.environ, MSIM_DEV_FLAGS=flags), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"{passed} passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_chunked(lib):
    """the payload-carrying entries (the chunked loops) again under MSIM_DEV_FLAGS 0x10000: at most 7 histories per launch"""
    _child("0x10000", "txn or rw or kafka", 9)


def test_tiny_pools(lib):
    """lin-kv again under MSIM_DEV_FLAGS 0x2000: the host search finishes a history, and its record is what comes back"""
    _child("0x2000", "lin_kv", 3)
