"""The non-cycle findings written on the device (txn_findings_kernel / rw_findings_kernel: csrc/txn_classify_body.inc, csrc/rw_check_dev.hip,
csrc/txn_findings.inc) through E.explain_txn_findings_batch (msim_explain_txn_findings_batch) and Engine.explain_txn_findings
(msim_explain_txn_findings), against the host entry (msim_explain_txn_findings_rows, which tests/test_txn_findings.py holds to the
contract): the check record, the header and the whole slab of every history byte for byte, over tests/txn_findings_cases.py as batches
and each history alone.  No history reaches the host walk unless it is one of the hand-off shapes (is_hand_off: those of the classify
kernels, and one finding more than the region of MSIM_TXN_FINDINGS_CAPACITY holds)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import test_elle_reference_vectors as V
import txn_findings_cases as K
from test_txn_findings import MODELS, doc_vector_checks, host

pytestmark = pytest.mark.gpu

DEV_FLAGS = int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0)
BOTH = pytest.mark.parametrize("rw", [False, True], ids=["list-append", "rw-register"])
_HOST = {}


def _twin(rw, name, model, cap):
    """the host entry's (record, header, slab) of a case, computed once per model and max_findings"""
    key = (rw, name, model, cap)
    if key not in _HOST:
        _HOST[key] = host(K.cases(rw)[name], rw, model, cap)
    return _HOST[key]


def _explained(rw, names, model="strict-serializable", cap=64, n_host=0):
    """one device entry call over the cases `names`: every record, header and slab is the host entry's; exactly n_host hand-overs"""
    hs = [K.cases(rw)[n] for n in names]
    out, hdr, fs, handed = E.explain_txn_findings_batch(hs, K.WORKLOAD[rw], model, max_findings=cap, with_n_host=True)
    for i, name in enumerate(names):
        w_out, w_hdr, w_slab = _twin(rw, name, model, cap)
        assert out[i].tobytes() == w_out.tobytes(), (name, model, out[i], w_out)
        assert hdr[i].tobytes() == w_hdr.tobytes(), (name, model, hdr[i], w_hdr)
        assert fs.slab[i].tobytes() == w_slab.tobytes(), (name, model, cap, [tuple(x) for x in fs.slab[i][:4]], [tuple(x) for x in w_slab[:4]])
        assert len(fs[i]) == int(hdr[i]["n_findings"])
    assert handed == n_host, (names[:3], model, handed, n_host)
    return out, hdr, fs


def _together(rw):
    """the cases whose capacities do not depend on their being alone in a batch: everything but the classify kernels' hand-off shapes"""
    return [n for n in K.cases(rw) if not n.startswith("hand-off: ")]


@BOTH
def test_every_case_as_a_batch(lib, rw):
    """one batch under each model: nothing but the history of capacity + 1 findings goes to the host"""
    names = _together(rw)
    for model in MODELS:
        _, hdr, _ = _explained(rw, names, model, n_host=1)
    i = names.index(f"{K.CAP} findings")
    assert int(hdr[i]["count"][1]) == K.CAP and int(hdr[i]["truncated"]) == 1 and int(hdr[i]["n_findings"]) == 64
    _explained(rw, names, cap=0, n_host=1)          # the headers alone


@BOTH
def test_each_case_alone(lib, rw):
    """a batch's capacities follow from its longest history: each history in a batch of its own, n_host 1 for a hand-off shape"""
    for name in K.cases(rw):
        _explained(rw, [name], n_host=1 if K.is_hand_off(name) else 0)


@BOTH
def test_capacity(lib, rw):
    """exactly MSIM_TXN_FINDINGS_CAPACITY findings stay on the device, one more is the host's; the whole slabs, untruncated"""
    cap = K.CAP + 8
    _, hdr, fs = _explained(rw, [f"{K.CAP} findings"], cap=cap, n_host=0)
    assert int(hdr[0]["n_findings"]) == K.CAP and int(hdr[0]["truncated"]) == 0
    _, hdr, _ = _explained(rw, [f"{K.CAP + 1} findings"], cap=cap, n_host=1)
    assert int(hdr[0]["n_findings"]) == K.CAP + 1
    _explained(rw, [f"{n} findings" for n in K.COUNTS], cap=cap, n_host=1)
    _explained(rw, [f"{n} findings" for n in K.COUNTS], cap=1, n_host=1)


def test_hand_off_shapes_in_one_batch(lib):
    """n_host is exactly the number of hand-off shapes that stay one in a batch of several: the twice-appended element, the payloads
    outside the area, the key and writer tables"""
    names = ["hand: G1b", "hand-off: a (key, element) appended twice", "hand-off: a payload outside the area", "hand-off: appended three times",
             "hand-off: two payloads outside the area", "hand-off: key 4096 (KMAX)", "65 findings"]
    _explained(False, names, n_host=5)
    _explained(True, ["hand: G1a", "hand-off: a (key, value) written twice", "two payloads outside the area"], n_host=1)


def test_doc_vectors(lib):
    """the reference documentation's transactions (tests/golden/elle_doc_vectors.json) through the device entry"""
    hs = [E.encode_txn_history(v["history"]) for v in V.VECTORS]
    out, hdr, fs, handed = E.explain_txn_findings_batch(hs, with_n_host=True)
    assert handed == 0
    doc_vector_checks(lambda i: (hs[i][0], hs[i][1], hdr[i], fs[i]))


@BOTH
def test_engine_explain_txn_findings(lib, rw):
    """Engine.explain_txn_findings over the HBM-resident histories of a 64-instance run equals the batch entry over the fetched
    histories; the check records are those of check(classify=True)"""
    if rw:
        cfg = E.test_config("txn-rw-register", node_count=2, rate=100.0, time_limit=3.0, seed=11, nemesis=("partition",), consistency_model="serializable")
    else:
        cfg = E.test_config("txn-list-append", node_count=3, rate=80.0, time_limit=3.0, latency=5, seed=11)
    with E.Engine(cfg) as eng:
        eng.run(0, 64)
        eng.check(classify=True)
        classified = eng.check_results().tobytes()
        got = eng.explain_txn_findings(max_findings=32)
        assert len(got) == 64 and eng.check_results().tobytes() == classified and eng.check_host_rechecks() == 0
        eng.fetch()
        hs = [tuple(x.copy() for x in eng.raw_history(i)) for i in range(64)]
        out, hdr, fs = E.explain_txn_findings_batch(hs, K.WORKLOAD[rw], "serializable" if rw else "strict-serializable", max_findings=32)
        for i, (rec, h, recs) in enumerate(got):
            assert h.tobytes() == hdr[i].tobytes() and recs.tobytes() == fs[i].tobytes(), (i, h, hdr[i])
            assert int(rec["error_count"]) == int(out[i]["error_count"]) and (int(rec["valid"]) == int(out[i]["valid"]) or int(eng.meta(i).flags))
        if not rw:
            assert all(not h.tobytes().strip(b"\0") for _, h, _ in got)      # the built-in nodes are strict-serializable: the zero header
    if not rw:
        with E.Engine(E.test_config("lin-kv", node_count=3, rate=10, time_limit=1, seed=1)) as eng:
            eng.run(0, 2)
            with pytest.raises(E.EngineError, match=r"\(-6\)"):
                eng.explain_txn_findings()


def test_refusals(lib):
    L = A.load()
    rows, pay = K.cases(False)["hand: G1b"]
    rows = np.ascontiguousarray(rows); pay = np.ascontiguousarray(pay, dtype=np.uint32)
    ro, po = np.asarray([0, len(rows)], dtype=np.uint64), np.asarray([0, len(pay)], dtype=np.uint64)
    out, hdr = np.zeros(1, dtype=E.CHECK_DT), np.zeros(1, dtype=E.TXN_EXPLAIN_DT)
    args = (rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, 1, 0, out.ctypes.data, None)
    assert L.msim_explain_txn_findings_batch(0, A.WL_KAFKA, *args, hdr.ctypes.data, None, 0) == A.E_INVALID
    assert L.msim_explain_txn_findings_batch(0, A.WL_TXN_LIST_APPEND, *args, None, None, 0) == A.E_INVALID
    assert L.msim_explain_txn_findings_batch(0, A.WL_TXN_LIST_APPEND, *args, hdr.ctypes.data, None, 3) == A.E_INVALID
    assert L.msim_explain_txn_findings_batch(0, A.WL_TXN_LIST_APPEND, *args[:5], 9, *args[6:], hdr.ctypes.data, None, 0) == A.E_INVALID
    assert L.msim_explain_txn_findings_batch(0, A.WL_TXN_LIST_APPEND, *args, hdr.ctypes.data, None, 0) == 0 and int(hdr[0]["count"][2]) == 1
    assert L.msim_explain_txn_findings(None, hdr.ctypes.data, None, 0, 1) == A.E_INVALID


CHILDREN = {
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
