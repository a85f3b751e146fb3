"""The explained set-full verdicts written on the device (csrc/set_full_body.inc behind set_explain_kernel) through
E.explain_set_full_batch (msim_explain_set_full_batch) and Engine.explain_set_full (msim_explain_set_full), against the host entry
(msim_explain_set_full_rows, which tests/test_set_explain.py holds against the definitions): the check record, the header and the whole
slab of element records — the zeros behind the counts included — byte for byte.  The batch is that of the host tests: the tutorial's
answer, the healthy map, the synthetic histories with all three classes, the hand-written edges, and one history of 1100 elements
(18 blocks of 64).  One concurrency serves them all: 120 is a multiple of every history's worker count, and a history's open reads
differ modulo its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import setfull_explain_ref as X
from test_set_explain import host

pytestmark = pytest.mark.gpu

CONCURRENCY = 120
TRACE = 0x1000
_BATCH, _HOST = [], {}


def _batch():
    """[(name, encoded history)], made once"""
    if not _BATCH:
        named = [("tutorial", X.tutorial()), ("healthy", X.healthy())] + [(str(s), make()) for s, (make, _, _) in X.SYNTH.items()]
        named += list(X.edges().items()) + [("7003", X.BIG[0]())]
        _BATCH.extend((name, E.encode_set_history(ops)) for name, ops in named)
    return _BATCH


def _twin(max_elements):
    """the host entry's (records, headers, slabs) of the batch, computed once per max_elements"""
    if max_elements not in _HOST:
        got = [host(h, max_elements) for _, h in _batch()]
        _HOST[max_elements] = (np.asarray([g[0] for g in got]), np.asarray([g[1] for g in got]), np.stack([g[2] for g in got]))
    return _HOST[max_elements]


def _same(what, i, out, hdr, slab, want_out, want_hdr, want_slab):
    assert out.tobytes() == want_out.tobytes(), (what, i, out, want_out)
    assert hdr.tobytes() == want_hdr.tobytes(), (what, i, hdr, want_hdr)
    assert slab.tobytes() == want_slab.tobytes(), (what, i, hdr, slab[:8], want_slab[:8])


@pytest.mark.parametrize("max_elements", [1408, 64])
def test_the_batch(lib, max_elements):
    names = [n for n, _ in _batch()]
    want_out, want_hdr, want_slab = _twin(max_elements)
    out, hdr, els = E.explain_set_full_batch([h for _, h in _batch()], CONCURRENCY, A.WL_G_SET, max_elements=max_elements)
    assert els.slab.shape == (len(names), max_elements)
    for i, name in enumerate(names):
        _same(name, i, out[i], hdr[i], els.slab[i], want_out[i], want_hdr[i], want_slab[i])
        assert len(els[i]) == int(hdr[i]["n_lost"]) + int(hdr[i]["n_never_read"]) + int(hdr[i]["n_stale"])
    big = hdr[names.index("7003")]
    if max_elements == 64:   # truncation falls inside the never-read segment
        assert (int(big["n_lost"]), int(big["n_never_read"]), int(big["n_stale"]), int(big["truncated"])) == (19, 45, 0, 1)
    else:
        assert (int(big["n_lost"]), int(big["n_never_read"]), int(big["n_stale"]), int(big["truncated"])) == (19, 69, 513, 0)
        assert {int(o) for e in els for o in e["outcome"]} == {A.SET_STABLE, A.SET_LOST, A.SET_NEVER_READ}
        assert int(hdr["n_worst_stale"].max()) == 8 and not hdr["truncated"].any()


def test_the_plain_check_writes_the_same_records(lib):
    """check_kernel and set_explain_kernel are two instantiations of one body: msim_check_set_full_batch's records are the same bytes"""
    plain = E.check_set_full_batch([h for _, h in _batch()], CONCURRENCY, A.WL_G_SET)
    out, _, _ = E.explain_set_full_batch([h for _, h in _batch()], CONCURRENCY, A.WL_G_SET, max_elements=64)
    assert plain.tobytes() == out.tobytes() == _twin(64)[0].tobytes()


def test_histories_alone_and_without_a_slab(lib):
    """a batch's capacities follow from its longest history: the edges again, each alone, with max_elements = 0 (the header only) and 3"""
    for name, h in _batch():
        if name in ("7003", "7001"):
            continue
        for m in (0, 3):
            want = host(h, m)
            out, hdr, els = E.explain_set_full_batch([h], CONCURRENCY, A.WL_BROADCAST, max_elements=m)
            _same(name, m, out[0], hdr[0], els.slab[0], *want)
            assert int(hdr[0]["truncated"]) == (1 if int(out[0]["lost_count"]) + int(out[0]["never_read_count"]) + int(out[0]["stale_count"]) > m else 0)


def test_poisoned_allocations(lib):
    """the batch tests again in a process whose device allocations are filled (MSIM_POISON): zeros behind the counts all the same"""
    if os.environ.get("MSIM_POISON"):
        return
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "the_batch or plain_check"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "3 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def _explain_and_verify(eng, what, capfd, taken):
    """explain_set_full of the last run: `taken` says whether a queued check was waited for; the records are check()'s of the same run,
    and record, header and elements are the host entry's on the fetched histories"""
    capfd.readouterr()
    got = eng.explain_set_full(max_elements=256)
    err = capfd.readouterr().err
    assert ("[check] taken" in err) == taken and "[check] explain" in err, (what, err)
    res = eng.check_results().copy()
    eng.check()   # the plain kernel over the same run
    assert eng.check_results().tobytes() == res.tobytes(), what
    eng.fetch()
    assert len(got) == eng.n
    for i, (rec, hdr, els) in enumerate(got):
        rows, pay = eng.raw_history(i)
        want_out, want_hdr, want_slab = host((rows.copy(), pay.copy()), 256, eng.cfg.workload)
        if int(eng.meta(i).flags):   # a capacity stop: the device says invalid whatever the rows say
            want_out = want_out.copy(); want_out["valid"] = 0
        assert rec.tobytes() == res[i].tobytes() == want_out.tobytes(), (what, i, rec, want_out)
        assert hdr.tobytes() == want_hdr.tobytes(), (what, i, hdr, want_hdr)
        assert els.tobytes() == want_slab[:len(els)].tobytes() and not want_slab[len(els):].tobytes().strip(b"\0"), (what, i)
        m = E.set_full_analysis(rec, hdr, els, rows, pay, eng.cfg.n_nodes, eng.cfg.workload)
        assert len(m["lost"]) == int(rec["lost_count"]) and len(m["stale"]) == int(rec["stale_count"]) and "truncated" not in m
    return got


@pytest.mark.parametrize("shape", ["broadcast-ff", "g-set"])
def test_engine_explain_set_full(lib, capfd, shape):
    """Engine.explain_set_full over the HBM-resident histories of a run, first on a context nobody checked (it launches, and arms), then
    with the check already queued behind the simulation (a checked launch, a second launch, then explain: it takes the queued check)"""
    if shape == "broadcast-ff":   # fire-and-forget gossip under partitions: elements missing on some nodes
        cfg, n = E.test_config("broadcast", bin="broadcast-ff", node_count=5, rate=20, time_limit=20, nemesis=["partition"], nemesis_interval=3, latency=10, seed=6), 16
    else:
        cfg, n = E.test_config("g-set", node_count=5, rate=10, time_limit=10, seed=2), 4
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(TRACE)
        eng.run(0, n)
        _explain_and_verify(eng, (shape, "un-armed"), capfd, taken=False)
        eng.run(1000, n)
        eng.check()
        eng.run(2000, n)
        _explain_and_verify(eng, (shape, "queued"), capfd, taken=True)


def test_refusals(lib):
    """an echo context and an echo batch: MSIM_E_UNSUPPORTED; a run not made yet: MSIM_E_RANGE"""
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        eng.run(0, 2)
        with pytest.raises(E.EngineError, match=r"\(-6\).*not a broadcast or g-set context"):
            eng.explain_set_full()
    with E.Engine(E.test_config("broadcast", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        with pytest.raises(E.EngineError, match=r"\(-5\)"):
            eng.explain_set_full()
    with pytest.raises(E.EngineError, match="-6"):
        E.explain_set_full_batch([_batch()[0][1]], 5, A.WL_ECHO)
