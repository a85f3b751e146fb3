"""kafka: the explanation of unclean histories on the device (csrc/kafka_check_dev.hip, kafka_explain_kernel: the classification's passes
with a finding wherever a bit is set, the findings sorted in LDS) through E.explain_kafka_batch (msim_explain_kafka_batch) and
Engine.explain_kafka (msim_explain_kafka), against the host entry (msim_explain_kafka_rows; tests/test_kafka_explain.py holds that one to
the contract's Python restatement): record, header and the whole slab byte for byte, and exactly the stated number of histories handed
to the host walk — none unless the case names the reason."""
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import kafka_classify_cases as K
from test_kafka import _h, _poll, _send
from test_kafka_explain import HAND, _GOOD, _many, host, invariants

pytestmark = pytest.mark.gpu

T_BOUND, F_MAX = A.KAFKA_EXPLAIN_TABLE_BOUND, A.KAFKA_EXPLAIN_MAX_FINDINGS
_HOST = {}


def _host_of(hs, max_findings):
    """the host entry's (record, header, slab) of the histories `hs` (a tuple, kept: computed once per set and slab length)"""
    key = (id(hs), max_findings)
    if key not in _HOST:
        _HOST[key] = (hs, [host(h, max_findings) for h in hs])
    return _HOST[key][1]


def _explained(hs, what, concurrency=3, n_host=0, max_findings=64):
    """one msim_explain_kafka_batch call: every record, header and slab the host entry's, exactly `n_host` histories handed over"""
    want = _host_of(hs, max_findings)
    out, hdr, fs, handed = E.explain_kafka_batch(list(hs), concurrency, max_findings=max_findings)
    for i, (w_out, w_hdr, w_slab) in enumerate(want):
        assert out[i].tobytes() == w_out.tobytes(), (what, i, out[i], w_out)
        assert hdr[i].tobytes() == w_hdr.tobytes(), (what, i, hdr[i], w_hdr)
        assert fs.slab[i].tobytes() == w_slab.tobytes(), (what, i, fs.slab[i][:8], w_slab[:8])
        assert len(fs[i]) == int(w_hdr["n_findings"])
        invariants(out[i], hdr[i], (what, i))
    assert handed == n_host, (what, handed, n_host)
    return out, hdr, fs


ALL_HS = tuple(HAND.values())


def test_hand_made_anomalies_singly_and_in_one_launch(lib):
    """one history per anomaly and the clean ones: alone, then all in one launch — the unclean ones are compacted into a list, their
    records must land at their own history's place.  Only the process that returns is the host's."""
    for name, h in HAND.items():
        out, hdr, fs = _explained((h,), name, n_host=1 if name == "returning" else 0)
        assert (int(hdr[0]["n_findings"]) == 0) == (name in _GOOD), name
    out, hdr, fs = _explained(ALL_HS, "all in one launch", n_host=1)
    assert [int(n) > 0 for n in hdr["n_findings"]] == [name not in _GOOD for name in HAND]
    known = fs[list(HAND).index("poll_skip")]
    assert E.kafka_findings(hdr[list(HAND).index("poll_skip")], known) == [
        {"anomaly": "poll-skip", "key": 5, "offset": 8, "value": 2, "other": 5, "row-a": 19, "row-b": 21, "delta": 3, "skipped-count": 2}]


def test_order_vectors(lib):
    hs = tuple(K.order_vectors().values())
    _explained(hs, "order vectors", concurrency=4)
    for name, h in K.order_vectors().items():
        _explained((h,), name, concurrency=4)


def test_corrupted_family(lib):
    hs = K.corrupted_family()
    out, hdr, fs = _explained(hs, "corrupted family", max_findings=128)
    assert sum(int(n) > 0 for n in hdr["n_findings"]) >= 20 and not hdr["truncated"].any()
    for h in hs[::9]:
        _explained((h,), "one of the family alone", max_findings=128)


def _three_workers():
    """concurrency 9: workers 0 and 8 share wavefront 0, worker 1 walks in wavefront 1; each sends offset 3 twice and polls offset 1 of
    its own key twice, the rows of the three interleaved"""
    per = []
    for w, key in ((0, "1"), (1, "2"), (8, "3")):
        per.append([*_send(w, key, 10 + w, 3), *_poll(w, {key: [[0, 20 + w], [1, 30 + w]]}), *_send(w, key, 10 + w, 3), *_poll(w, {key: [[1, 30 + w]]})])
    return E.encode_kafka_history(_h(*[op for group in zip(*per) for op in group]))


STREAMS = (_three_workers(),)


def test_stream_findings_of_several_wavefronts_come_in_the_contracts_order(lib):
    out, hdr, fs = _explained(STREAMS, "three workers", concurrency=9)
    named = [(f["anomaly"], f["key"]) for f in E.kafka_findings(hdr[0], fs[0])]
    assert named == [("nonmonotonic-poll", 1), ("nonmonotonic-poll", 2), ("nonmonotonic-poll", 3),
                     ("nonmonotonic-send", 1), ("nonmonotonic-send", 2), ("nonmonotonic-send", 3)], named
    rows = [(int(f["row_a"]), int(f["row_b"])) for f in fs[0]]
    assert len(set(rows)) == 6 and all(a < b for a, b in rows)


TIES = (K.raw_history(("poll", 1, [(1, 5, [7]), (1, 5, [7]), (1, 5, [7])])),)


def test_tie_records_are_the_same_bytes(lib):
    """three blocks of one key with the same first offset in one poll: the second and the third are the same internal nonmonotonic step"""
    out, hdr, fs = _explained(TIES, "ties")
    assert int(hdr[0]["n_findings"]) == 2 and fs[0][0].tobytes() == fs[0][1].tobytes()
    assert E.kafka_findings(hdr[0], fs[0])[0] == {"anomaly": "int-nonmonotonic-poll", "key": 1, "offset": 5, "value": 7, "other": 5, "row-a": 0, "row-b": 0, "delta": 0}


def _long_polls():
    """polls of more than 128 payload words whose finding sits behind the staged part: 255 + 5 + 40 pairs in three blocks that jump over
    the acknowledged offsets 260 and 261 (the third block's header is payload word 133); and a block of 255 pairs followed, at payload
    word 129, by a block that steps back to offset 10 — its first message is read from HBM"""
    pairs = [[o, o + 1] for o in range(260)] + [[o, o + 1] for o in range(262, 302)]
    skip = E.encode_kafka_history(_h(*_send(0, "2", 261, 260), *_send(0, "2", 262, 261), *_poll(1, {"2": pairs})))
    back = K.raw_history(("poll", 1, [(2, 0, list(range(1, 256))), (2, 10, [11, 12])]))
    return skip, back


LONG = _long_polls()


def test_findings_behind_the_staged_part_of_a_poll(lib):
    out, hdr, fs = _explained(LONG, "long polls")
    skip = [f for f in E.kafka_findings(hdr[0], fs[0]) if f["anomaly"] == "int-poll-skip"]
    assert skip == [{"anomaly": "int-poll-skip", "key": 2, "offset": 262, "value": 2, "other": 259, "row-a": 5, "row-b": 5, "delta": 3, "skipped-count": 2}]
    assert E.kafka_findings(hdr[1], fs[1]) == [{"anomaly": "int-nonmonotonic-poll", "key": 2, "offset": 10, "value": 11, "other": 254, "row-a": 0, "row-b": 0, "delta": -244}]


def _send_rows(n_sends, filler=0):
    """`n_sends` acknowledged sends of message 1 at offset 3 of key 1 by process 0 (each after the first is one nonmonotonic send), after the
    first one `filler` rows that invoke a poll: 2 * n_sends + filler rows"""
    n = 2 * n_sends + filler
    rows = np.zeros(n, dtype=E.OP_DT)
    rows["time_len"] = np.arange(n, dtype=np.uint64) * 1000
    rows["packed"] = A.T_INVOKE | (A.F_POLL << 2)
    at = np.concatenate([[0], 2 + filler + 2 * np.arange(n_sends - 1)]).astype(np.int64)
    rows["packed"][at] = A.T_INVOKE | (A.F_SEND << 2)
    rows["value"][at] = 1 | (1 << 6) | (0x7FF << 17)
    rows["packed"][at + 1] = A.T_OK | (A.F_SEND << 2)
    rows["value"][at + 1] = 1 | (1 << 6) | (3 << 17)
    return rows, np.zeros(1, dtype=np.uint32)


MANY_ROWS = (_send_rows(2, filler=65537 - 4),)


def test_a_finding_in_the_last_row_of_64k_plus_one_rows(lib):
    assert len(MANY_ROWS[0][0]) == 65537
    out, hdr, fs = _explained(MANY_ROWS, "64k + 1 rows")
    assert E.kafka_findings(hdr[0], fs[0]) == [{"anomaly": "nonmonotonic-send", "key": 1, "offset": 3, "value": 1, "other": 3, "row-a": 1, "row-b": 65536}]


MANY = (_many(),)


def test_truncation(lib):
    n = int(_host_of(MANY, 64)[0][1]["n_findings"])
    assert n == 9
    for cap in (0, 1, n - 1, n):
        out, hdr, fs = _explained(MANY, f"max_findings {cap}", max_findings=cap)
        assert int(hdr[0]["n_findings"]) == cap and int(hdr[0]["truncated"]) == int(cap < n) and int(hdr[0]["count"].sum()) == n


AT_CAPACITY, BEYOND_CAPACITY = (_send_rows(F_MAX + 1),), (_send_rows(F_MAX + 2),)


def test_the_finding_capacity(lib):
    """exactly as many findings as the sort holds stay on the device; one more is the host walk's, with the same bytes"""
    out, hdr, fs = _explained(AT_CAPACITY, "findings at capacity", max_findings=F_MAX + 8)
    assert int(hdr[0]["n_findings"]) == F_MAX and [int(f["row_b"]) for f in fs[0]] == list(range(3, 2 * F_MAX + 2, 2))
    out, hdr, fs = _explained(BEYOND_CAPACITY, "findings beyond capacity", max_findings=F_MAX + 8, n_host=1)
    assert int(hdr[0]["n_findings"]) == F_MAX + 1
    out, hdr, fs = _explained(BEYOND_CAPACITY, "findings beyond capacity, truncated", max_findings=16, n_host=1)
    assert int(hdr[0]["truncated"]) == 1 and int(hdr[0]["count"][2]) == F_MAX + 1


def _at_offset(o):
    return (E.encode_kafka_history(_h(*_send(0, "1", 5, o), *_poll(1, {"1": [[o, 7]]}))),)


BELOW_BOUND, AT_BOUND = _at_offset(T_BOUND - 1), _at_offset(T_BOUND)


def test_the_table_bound(lib):
    for hs, handed in ((BELOW_BOUND, 0), (AT_BOUND, 1)):
        out, hdr, fs = _explained(hs, f"offset {T_BOUND - 1 + handed}", n_host=handed)
        assert [f["anomaly"] for f in E.kafka_findings(hdr[0], fs[0])] == ["inconsistent-offsets"] and int(fs[0][0]["offset"]) == T_BOUND - 1 + handed


def test_engine_explain_kafka(lib):
    """Engine.explain_kafka on a small built-in run: the node is correct, so no history has a finding, and the records are check()'s"""
    cfg = E.test_config("kafka", node_count=3, rate=60, time_limit=4, latency=5, nemesis=["partition"], nemesis_interval=2, seed=14)
    with E.Engine(cfg) as eng:
        eng.run(0, 24)
        eng.check()
        plain = eng.check_results().tobytes()
        got = eng.explain_kafka(max_findings=8)
        assert eng.check_results().tobytes() == plain and eng.check_host_rechecks() == 0
        assert len(got) == 24 and all(int(hdr["n_findings"]) == 0 and not hdr["count"].any() and len(fs) == 0 for _, hdr, fs in got)
        assert b"".join(rec.tobytes() for rec, _, _ in got) == plain and (eng.check_results()["valid"] == 1).all()
        eng.set_dev_flags(0x800)   # the checks on the host cores: the walk explains
        again = eng.explain_kafka(max_findings=8)
        assert b"".join(rec.tobytes() for rec, _, _ in again) == plain and all(int(hdr["n_findings"]) == 0 for _, hdr, _ in again)
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        eng.run(0, 2)
        hdr = np.zeros(2, dtype=E.KAFKA_EXPLAIN_DT)
        assert A.load().msim_explain_kafka(eng._ctx, hdr.ctypes.data, None, 0, 2) == A.E_UNSUPPORTED


def test_poisoned_allocations(lib):
    """this module again in a process of its own with every device allocation filled with 0xA5 first (MSIM_POISON is read once per
    process) and at most 7 histories per launch of the explaining kernel (developer flag 0x10000: its chunks reuse one workspace): no
    LDS table, workspace slab, list or record is read before it is written"""
    if os.environ.get("MSIM_POISON"):
        return
    env = dict(os.environ, MSIM_POISON="165", MSIM_DEV_FLAGS="0x10000")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not poisoned"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
