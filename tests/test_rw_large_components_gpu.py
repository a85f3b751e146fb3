"""Strongly connected components beyond the LDS matrix of the rw-register classification (csrc/rw_check_dev.hip, rw_classify:
single_by_search): a component of more than 256 transactions is decided on the device by a multi-source search, 64 heads of rw edges at a
time, and no longer handed to the host.  Every case compares E.classify_rw_batch and E.check_rw_batch with the host analysis
(msim_check_rw_rows), every field, under all five models (tests/test_rw_classify_gpu.py::_both_entries), with n_host == 0.

MSIM_DEV_FLAGS bit 0x20000 makes the matrix's capacity 16 transactions with the search behind it, so that small histories of every
cycle class take the search; bit 0x2000 keeps its meaning (capacity 16, anything larger is the host's)."""
import os
import subprocess
import sys

import pytest

from maelstrom_amd import engine as E

import oracle_lib as O
import test_rw_classify_gpu as T
from test_rw_classify_gpu import _both_entries, _host, _same

pytestmark = pytest.mark.gpu

TINY = T.TINY          # MSIM_DEV_FLAGS bit 0x2000 (test_bit_13_keeps_the_host_fallback's child): components of more than 16 are the host's
R, W = ":r", ":w"
WAVE = 48              # transactions invoked together, then completed together, a process each: below the 64 open calls of the device


def _waves(txns, wave=WAVE):
    """[(requested, completed)] -> ops: waves of `wave` transactions, each wave invoked together and then completed together"""
    ops = []
    for b in range(0, len(txns), wave):
        part = txns[b:b + wave]
        ops += [{"type": ":invoke", "process": p, "f": ":txn", "value": req} for p, (req, _) in enumerate(part)]
        ops += [{"type": ":ok", "process": p, "f": ":txn", "value": done} for p, (_, done) in enumerate(part)]
    return ops


def _same_txn(mops):
    return (mops, mops)


def g2_ring(n, k0=0):
    """T_i = [r k_i nil, w k_(i+1) 1]: the rw edges T_i -> T_(i-1) are one ring of n, and no other dependency edge exists"""
    return [_same_txn([[R, k0 + i, None], [W, k0 + (i + 1) % n, 1]]) for i in range(n)]


def deep_g_single(n, k0=0):
    """one rw edge T_(n-1) -> T_0 (key z = k0), closed by a wr path of n - 1 links"""
    z = k0
    k = lambda i: k0 + i
    txns = [_same_txn([[W, z, 1], [W, k(1), 1]])]
    for i in range(1, n - 1):
        txns.append(([[R, k(i), None], [W, k(i + 1), 1]], [[R, k(i), 1], [W, k(i + 1), 1]]))
    txns.append(([[R, k(n - 1), None], [R, z, None]], [[R, k(n - 1), 1], [R, z, None]]))
    return txns


def open_chain(n):
    """T_i = [r k_i nil, w k_(i+1) 1] on n + 1 keys: the rw edges T_(i+1) -> T_i alone are acyclic; a realtime edge closes those that
    cross a wave boundary"""
    return [_same_txn([[R, i, None], [W, i + 1, 1]]) for i in range(n)]


def g2_realtime(links):
    """X_j = [w q_j 1, r p_(j-1) nil] one after the other on process 0; B_j = [r q_j nil, w p_j 1] on processes 1 and 2 alternately,
    invoked before X_j completes and completed after X_(j+1) is invoked: X_(j+1) -rw-> B_j -rw-> X_j, X_j before X_(j+1) in real time"""
    q = lambda j: 2 * j + 2
    p = lambda j: 2 * j + 3          # p(-1) = 1: a key nobody writes
    X = lambda j: [[W, q(j), 1], [R, p(j - 1), None]]
    B = lambda j: [[R, q(j), None], [W, p(j), 1]]
    op = lambda typ, proc, v: {"type": typ, "process": proc, "f": ":txn", "value": v}
    ops = [op(":invoke", 0, X(0))]
    for j in range(links):
        pb = 1 + j % 2
        ops += [op(":invoke", pb, B(j)), op(":ok", 0, X(j)), op(":invoke", 0, X(j + 1)), op(":ok", pb, B(j))]
    ops.append(op(":ok", 0, X(links)))
    return ops


def wr_ring(n):
    """T_i = [w k_i 1, r k_(i+1) -> 1]: the wr edges T_(i+1) -> T_i are one ring"""
    return [([[W, i, 1], [R, (i + 1) % n, None]], [[W, i, 1], [R, (i + 1) % n, 1]]) for i in range(n)]


def _enc(ops):
    return E.encode_txn_history(ops, rw=True)


def _classes(rec):
    return {n for n, b in T.BITS.items() if int(rec["error_count"]) & b}


def _check(hs, want, sizes, expect_host=False):
    """the host's records name the classes `want[i]` and `sizes[i]` transactions in cycles; both device entries give the host's records"""
    host = _host(hs, "strict-serializable")
    for i in range(len(hs)):
        assert _classes(host[i]) == want[i] and int(host[i]["stale_count"]) == sizes[i], (i, _classes(host[i]), host[i])
    _both_entries(hs, expect_host=expect_host)


_KEEP = {}


def _hs(name, make):
    """the encoded histories of a case (a tuple, kept: _host keeps its records by the tuple's identity)"""
    if name not in _KEEP:
        _KEEP[name] = tuple(_enc(ops) for ops in make())
    return _KEEP[name]


@pytest.mark.parametrize("n", [256, 257, 300, 1500])
def test_g2_ring(lib, n):
    """256 is the last size on the matrix; 1500 is 24 batches of heads and three chunks of transactions per lane.  Under MSIM_DEV_FLAGS
    bit 0x2000 (test_bit_13_keeps_the_host_fallback's child) the ring is the host's."""
    hs = _hs(("ring", n), lambda: [_waves(g2_ring(n))])
    _check(hs, [{"G2"}], [n], expect_host=TINY)


@pytest.mark.parametrize("n", [300, 1500])
def test_deep_g_single(lib, n):
    """a wr path of n - 1 links closes the one rw edge; issued in this order and in reverse"""
    hs = _hs(("deep", n), lambda: [_waves(deep_g_single(n)), _waves(deep_g_single(n)[::-1])])
    _check(hs, [{"G-single"}, {"G-single"}], [n, n])


def test_g_single_realtime(lib):
    hs = _hs("open-chain", lambda: [_waves(open_chain(300))])
    _check(hs, [{"G-single", "realtime"}], [300])


def test_g2_realtime(lib):
    hs = _hs("g2-realtime", lambda: [g2_realtime(150)])
    _check(hs, [{"G2", "realtime"}], [301])


def test_two_large_components(lib):
    """the search goes on past a large component without a G-single: a ring of 300 first, then a deep G-single of 300 on keys of its
    own; and the ring followed by the two-transaction G-single of test_rw_classify_gpu.HAND"""
    def make():
        small = [{**op, "value": [[f, k + 2000, v] for f, k, v in op["value"]]} for op in T.HAND["G-single"][0]]
        return [_waves(g2_ring(300) + deep_g_single(300, k0=1000)), _waves(g2_ring(300)) + small]
    hs = _hs("two", make)
    _check(hs, [{"G-single"}, {"G-single"}], [600, 302])


def test_large_g1c_component(lib):
    """a wr ring of 300: G0 and G1c never use the matrix"""
    hs = _hs("wr-ring", lambda: [_waves(wr_ring(300))])
    _check(hs, [{"G1c"}], [300])


ENGINE_FIRST = 0
_ENGINE = []


def _engine_cfg():
    return T._cfg(node_count=5, latency=5, rate=100.0, time_limit=30.0, nemesis=("partition",), nemesis_interval=10.0)


def test_engine_histories_with_large_components(lib):
    """Eight histories of five nodes, about 3000 transactions each (instances ENGINE_FIRST .. ENGINE_FIRST + 7), 356 to 658 of them in
    cycles.  Before the search the library handed instances 1, 3, 6 and 7 to the host under serializable and strict-serializable (found
    on the emulator with the library of the commit before); the others' components each fit the matrix."""
    if not _ENGINE:
        o = O.run(_engine_cfg(), ENGINE_FIRST, 8)
        _ENGINE.append(tuple(o.history(i) for i in range(8)))
    hs = _ENGINE[0]
    host = _host(hs, "serializable")
    assert int(host["stale_count"].max()) > 256 and int(host["attempt_count"].min()) > 2500, (host["stale_count"], host["attempt_count"])
    _both_entries(hs)


def test_engine_check_classify_with_large_components(lib):
    with E.Engine(_engine_cfg()) as eng:
        eng.run(ENGINE_FIRST, 8)
        eng.check(classify=True)
        assert eng.check_host_rechecks() == 0
        res = eng.check_results().copy()
        eng.fetch()
        hs = tuple((eng.raw_history(i)[0].copy(), eng.raw_history(i)[1].copy()) for i in range(8))
        host = _host(hs, "read-committed")
        assert int(host["stale_count"].max()) > 256
        _same(res, host, "Engine.check(classify=True)")


def _child(flags, target, k):
    env = dict(os.environ, MSIM_DEV_FLAGS=flags)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", target, "-k", k],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("flags", ["0x20000", "0x30000"])
def test_every_class_on_the_search(lib, flags):
    """The 240 random histories of tests/test_rw_classify_gpu.py (every cycle class, components of up to 71 transactions) in a process
    of its own under MSIM_DEV_FLAGS bit 0x20000: the matrix holds 16 transactions, larger components take the search; that test asserts
    n_host == 0 and the host's records through both entries.  0x30000: at most 7 histories per launch as well."""
    assert not int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0) & 0x22000
    _child(flags, os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_rw_classify_gpu.py"), "test_random_histories")


def test_bit_13_keeps_the_host_fallback(lib):
    """the ring of 300 in a process of its own under MSIM_DEV_FLAGS=0x2000: n_host > 0, and the records are still the host's"""
    assert not TINY
    _child("0x2000", os.path.abspath(__file__), "test_g2_ring and 300")
