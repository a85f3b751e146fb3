"""The witness cycles found on the device (csrc/cycle_classify.inc behind txn_explain_kernel / rw_explain_kernel) through
E.explain_txn_batch / E.explain_rw_batch (msim_explain_txn_batch / msim_explain_rw_batch) and Engine.explain_txn (msim_explain_txn),
against the host entries (msim_explain_txn_rows / msim_explain_rw_rows, which tests/test_txn_explain.py holds against the definition):
the check record over FIELDS, the cycle records and the whole slabs of steps byte for byte.  The sets are those of
tests/test_txn_classify_gpu.py, tests/test_rw_classify_gpu.py and tests/test_rw_large_components_gpu.py (the large components a few
hundred transactions here); no history reaches the host unless it has one of the shapes of HAND_OFF or MSIM_DEV_FLAGS bit 0x2000 is set
(test_children)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import test_rw_classify_gpu as RWT
import test_rw_large_components_gpu as BIG
import test_txn_classify_gpu as T
import txn_witness_ref as R
from test_txn_check_gpu import FIELDS
from test_txn_explain import host

pytestmark = pytest.mark.gpu

DEV_FLAGS = int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0)
TINY = bool(DEV_FLAGS & 0x2000)   # a component of more than 16 transactions is the host's
_HOST = {}


def _twin(hs, model, max_steps, rw):
    """the host entry's (records, cycles, slabs) of the histories `hs` (a tuple, kept: computed once per set, model and max_steps)"""
    key = (id(hs), model, max_steps, rw)
    if key not in _HOST:
        got = [host(h, model, max_steps, rw) for h in hs]
        _HOST[key] = (hs, np.asarray([g[0] for g in got]), np.asarray([g[1] for g in got]), np.stack([g[2] for g in got]))
    return _HOST[key][1:]


def _explained(hs, what, model="strict-serializable", n_host=0, max_steps=64, rw=False):
    """one device entry call: the record, the cycle record and the slab of every history are the host entry's; exactly `n_host` histories
    handed over (None: not asserted).  Returns (cycles, handed)."""
    want_out, want_cyc, want_steps = _twin(hs, model, max_steps, rw)
    out, cyc, steps, handed = (E.explain_rw_batch if rw else E.explain_txn_batch)(list(hs), model, max_steps=max_steps)
    for i in range(len(hs)):
        for f in FIELDS:
            assert int(out[i][f]) == int(want_out[i][f]), (what, model, i, f, int(out[i][f]), int(want_out[i][f]))
        assert cyc[i].tobytes() == want_cyc[i].tobytes(), (what, model, i, cyc[i], want_cyc[i])
        assert steps.slab[i].tobytes() == want_steps[i].tobytes(), (what, model, i, cyc[i], steps.slab[i][:8], want_steps[i][:8])
        assert len(steps[i]) == int(cyc[i]["n_steps"])
    if n_host is not None:
        assert handed == n_host, (what, model, handed, n_host)
    return cyc, handed


def test_hand_made_histories(lib):
    """test_txn_classify_gpu.HAND as a batch under every model and each history alone (a batch's capacities follow from its longest)"""
    for model in T.MODELS:
        cyc, _ = _explained(T.HAND_HS, "hand-made", model)
    names = list(T.HAND)
    assert int(cyc[names.index("G2-realtime")]["length"]) == 3 and int(cyc[names.index("empty")]["length"]) == 0
    for i, h in enumerate(T.HAND_HS):
        _explained((h,), names[i])


def test_faulted_random_set(lib):
    hs = T._faulted_hs()
    assert len(hs) == 104
    cyc, _ = _explained(hs, "the faulted random set")
    assert (cyc["length"] > 0).sum() >= 10


def test_store_without_isolation(lib):
    """64 histories, every cycle class, components past 64 transactions; under bit 0x2000 the larger components are the host's"""
    hs = T._no_isolation_hs()
    cyc, handed = _explained(hs, "no isolation", n_host=None, max_steps=256)
    classes = {int(c) & ~R.REALTIME for c in cyc["anomalies"]}
    assert {R.G0, R.G1C, R.G_SINGLE, R.G2} <= classes and (cyc["anomalies"] & R.REALTIME != 0).any(), classes
    assert (handed > 0) if TINY else (handed == 0), handed
    _explained(hs, "no isolation", "read-committed", n_host=None, max_steps=256)


def test_component_sizes_around_the_matrix(lib):
    """CHAINS: witnesses of 16, 17 (the tiny matrix of bits 0x2000 / 0x20000), 255, 256, 257 (the matrix of 256) and 600 transactions —
    the last two found by the search of a large component; whole, and truncated to 8 steps"""
    cyc, handed = _explained(T.CHAINS, "chains", n_host=None, max_steps=1024)
    assert [int(c) for c in cyc["length"]] == [16, 17, 255, 256, 257, 600] and (cyc["n_steps"] == cyc["length"]).all()
    assert handed == (5 if TINY else 0), handed
    cyc, _ = _explained(T.CHAINS, "chains, truncated", n_host=None, max_steps=8)
    assert [int(c) for c in cyc["length"]] == [16, 17, 255, 256, 257, 600] and (cyc["n_steps"] == 8).all()
    for h in T.CHAINS[:2]:
        _explained((h,), "a chain alone", n_host=None)


def test_sizes(lib):
    """1, 63, 64, 65 and 129 transactions (blocks of 64 lanes)"""
    hs = [E.encode_txn_history(T._ops(*T._pair(0, [[T.A_, 1, 1], [T.R_, 1, None]])))]
    hs += [E.encode_txn_history(T.no_isolation(300 + n, 3, 3, n)) for n in (63, 64, 65, 129)]
    hs = tuple(hs)
    cyc, _ = _explained(hs, "sizes", n_host=None if TINY else 0, max_steps=256)
    assert int(cyc[0]["length"]) == 0 and (cyc["length"][1:] > 0).all()
    for i in range(len(hs)):
        _explained((hs[i],), ("sizes, alone", i), n_host=None if TINY else 0, max_steps=256)


def test_one_step(lib):
    """max_steps = 1: the first step of every witness, the true length beside it"""
    cyc, _ = _explained(T.HAND_HS, "hand-made, one step", max_steps=1)
    assert int(cyc["n_steps"].max()) == 1 and int(cyc["length"].max()) == 3
    _explained(RWT.HAND_HS, "rw hand-made, one step", "read-committed", max_steps=1, rw=True)


def test_rw_register_hand_made_and_random(lib):
    """test_rw_classify_gpu's hand-made histories under every model, and its 240 random ones with reads from the future"""
    for model in RWT.MODELS:
        _explained(RWT.HAND_HS, "rw hand-made", model, rw=True)
    hs = RWT._random_hs()
    cyc, handed = _explained(hs, "rw random", n_host=None, max_steps=256, rw=True)
    classes = {int(c) & ~R.REALTIME for c in cyc["anomalies"]}
    assert {0, R.G0, R.G1C, R.G_SINGLE, R.G2} <= classes, classes
    assert (handed > 0) if TINY else (handed == 0), handed
    _explained(hs, "rw random", "serializable", n_host=None, max_steps=256, rw=True)


_LARGE = []


def _large_hs():
    if not _LARGE:
        two = BIG._waves(BIG.g2_ring(280) + BIG.deep_g_single(270, k0=1000))
        _LARGE.append(tuple(BIG._enc(ops) for ops in (
            BIG._waves(BIG.g2_ring(257)), BIG._waves(BIG.g2_ring(300)), BIG._waves(BIG.deep_g_single(300)), BIG._waves(BIG.open_chain(300)),
            BIG.g2_realtime(140), two, BIG._waves(BIG.wr_ring(300)))))
    return _LARGE[0]


def test_rw_register_large_components(lib):
    """test_rw_large_components_gpu's shapes at 257 - 550 transactions: rings whose witness is the whole ring (G2 of 300, G1c of 300), a
    G-single closed by a wr path of 299 links, realtime-only cycles across the waves, two large components in one history"""
    hs = _large_hs()
    cyc, handed = _explained(hs, "rw large", n_host=None, max_steps=512, rw=True)
    assert [int(c) for c in cyc["length"][:3]] == [257, 300, 300] and int(cyc["length"][6]) == 300
    assert [int(c) for c in cyc["anomalies"][:3]] == [R.G2, R.G2, R.G_SINGLE] and int(cyc["anomalies"][6]) == R.G1C
    assert (handed > 0) if TINY else (handed == 0), handed
    ops = BIG._waves(BIG.g2_ring(300))
    _, edges = R.edges_rw(ops)
    _, c, steps = host(hs[1], max_steps=512, rw=True)
    assert R.verify(edges, int(c["anomalies"]), [(int(s["txn"]), int(s["kinds"])) for s in steps[:300]])


@pytest.mark.parametrize("shape", list(T.HAND_OFF))
def test_hand_off(lib, shape):
    """the shapes that are the host's, a batch each: n_host counts the history and the records are the host entry's"""
    _explained((T.HAND_OFF[shape](),), shape, n_host=1)


def test_engine_explain_txn(lib):
    """Engine.explain_txn over the HBM-resident histories of a run: a txn-list-append run is clean (zero records, check()'s records); a
    txn-rw-register run under serializable has a G2 cycle nearly everywhere, the records are the host entry's on the fetched histories
    and verify; another workload is refused"""
    cfg = E.test_config("txn-list-append", node_count=3, rate=80.0, time_limit=5.0, latency=5, seed=11)
    with E.Engine(cfg) as eng:
        eng.run(0, 16)
        eng.check()
        plain = eng.check_results().tobytes()
        got = eng.explain_txn()
        assert len(got) == 16 and eng.check_results().tobytes() == plain
        assert all(not c.tobytes().strip(b"\0") and len(s) == 0 for _, c, s in got)
    cfg = E.test_config("txn-rw-register", node_count=2, rate=100.0, time_limit=6.0, seed=11, nemesis=("partition",), consistency_model="serializable")
    with E.Engine(cfg) as eng:
        eng.run(0, 32)
        got = eng.explain_txn(max_steps=64)
        res = eng.check_results().copy()
        assert eng.check_host_rechecks() == 0
        eng.fetch()
        witnessed = 0
        for i, (rec, cyc, steps) in enumerate(got):
            rows, pay = eng.raw_history(i)
            h = (rows.copy(), pay.copy())
            out, c, slab = host(h, "serializable", 64, rw=True)
            assert rec.tobytes() == res[i].tobytes()
            for f in FIELDS:
                assert int(rec[f]) == int(out[f]) or (f == "valid" and int(eng.meta(i).flags)), (i, f, rec, out)
            assert cyc.tobytes() == c.tobytes() and steps.tobytes() == slab[:int(c["n_steps"])].tobytes(), (i, cyc, c)
            if int(cyc["length"]):
                witnessed += 1
                if int(cyc["length"]) <= 64:
                    _, edges = R.edges_rw(E.decode_history(h[0], h[1], 2, A.WL_TXN_RW_REGISTER))
                    assert R.verify(edges, int(cyc["anomalies"]), [(int(s["txn"]), int(s["kinds"])) for s in steps])
        assert witnessed >= 24, witnessed
    with E.Engine(E.test_config("lin-kv", node_count=3, rate=10, time_limit=1, seed=1)) as eng:
        eng.run(0, 2)
        with pytest.raises(E.EngineError, match=r"\(-6\)"):
            eng.explain_txn()


CHILDREN = {
    "0x20000": (dict(MSIM_DEV_FLAGS="0x20000"), "not children and not engine"),   # a matrix of 16: small components take the search
    "0x2000": (dict(MSIM_DEV_FLAGS="0x2000"), "store_without_isolation or component_sizes or rw_register"),   # and no search: the host finishes them
    "0x10000": (dict(MSIM_DEV_FLAGS="0x10000"), "not children and not engine"),   # at most 7 histories per launch
    "poison": (dict(MSIM_POISON="0xA5"), "not children"),                         # device allocations filled: nothing read before it is written
}


@pytest.mark.parametrize("child", list(CHILDREN))
def test_children(lib, child):
    """this module again in a process of its own (the batch entries read their switches from the environment once per process)"""
    assert DEV_FLAGS == 0
    extra, select = CHILDREN[child]
    env = dict(os.environ, **extra)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", select],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
