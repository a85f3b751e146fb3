"""kafka: the device classification of UNCLEAN histories (csrc/kafka_check_dev.hip, kafka_classify_kernel: every pass run, every anomaly
bit and count accumulated, the order of the observations kept by 64-bit ordered table cells) through E.classify_kafka_batch
(msim_classify_kafka_batch) and Engine.check(classify=True), against the host checker (msim_check_kafka_rows = check_kafka of
csrc/kafka_check.cpp; the `_host` of tests/test_kafka_check_gpu.py), field by field over that module's FIELDS.

The yardstick is always the host's record, also where it depends on the order of the rows (test_order_sensitive_vectors;
tests/kafka_check_ref.py is set-based and is not used here).  No history reaches the host (n_host == 0) unless it has one of the
shapes the header names: a row that does not decode, a process that returns after a later process of its worker, an offset or message
from 1152 on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import kafka_classify_cases as K
from test_kafka import _cfg, _h, _ops, _poll, _send
from test_kafka_check_gpu import FIELDS, _anomalies, _host, _same

pytestmark = pytest.mark.gpu

BITS = {name: bit for bit, name in A.KAFKA_ANOMALIES.items()}
T_BOUND = 1152   # include/maelsim.h, msim_classify_kafka_batch: offsets and messages from here on are the host's
_HOST = {}


def _host_of(hs):
    """the host's records of the histories `hs` (a tuple, kept: computed once per set)"""
    if id(hs) not in _HOST:
        _HOST[id(hs)] = (hs, [_host(r, p) for r, p in hs])
    return _HOST[id(hs)][1]


def _names(bits):
    return {n for n, b in BITS.items() if bits & b}


def _classified(hs, what, concurrency=3, n_host=0):
    """one msim_classify_kafka_batch call: every record the host's, exactly `n_host` histories handed over"""
    host = _host_of(hs)
    dev, handed = E.classify_kafka_batch(list(hs), concurrency)
    for i, h in enumerate(host):
        assert _same(dev[i], h), (what, i, {f: int(dev[i][f]) for f in FIELDS}, h, _names(h["error_count"]))
    assert handed == n_host, (what, handed, n_host)
    return dev


_BAD, _GOOD = _anomalies()
BAD_HS = {name: E.encode_kafka_history(ops) for name, ops in _BAD.items()}
GOOD_HS = {name: E.encode_kafka_history(ops) for name, ops in _GOOD.items()}
ALL_HS = tuple(list(BAD_HS.values()) + list(GOOD_HS.values()))


def test_hand_made_anomalies_are_decided_on_the_device(lib):
    """tests/test_kafka_check_gpu.py's hand-made histories, one per anomaly: the host's record without the host (only the process that
    returns is handed over); the default entry still sends every one of them to the host."""
    for name, hs in BAD_HS.items():
        _classified((hs,), name, n_host=1 if name == "returning" else 0)
        assert _host(*hs)["error_count"] != 0 or name == "returning", name
    for name, hs in GOOD_HS.items():
        _classified((hs,), name)
        assert _host(*hs)["error_count"] == 0, name
    _classified(ALL_HS, "all in one launch", n_host=1)
    out, n_host = E.check_kafka_batch(list(ALL_HS), 3)
    assert n_host == len(BAD_HS)
    for rec, h in zip(out, _host_of(ALL_HS)):
        assert _same(rec, h)


def test_order_sensitive_vectors(lib):
    """the host keeps the LAST message of an offset and the FIRST offset of a message: the same observations in another order give
    another record (the table of the classification's issue), across rows and inside one poll"""
    vec = K.order_vectors()
    hs = tuple(vec.values())
    host = dict(zip(vec, _host_of(hs)))
    want = {"A fwd": (64, 0), "A rev": (320, 0), "B fwd": (192, 1), "B rev": (192, 2), "B one row": (208, 1), "B one reversed": (208, 2)}
    for name, (bits, dups) in want.items():
        assert (host[name]["error_count"], host[name]["duplicated_count"]) == (bits, dups), (name, host[name])
    for a, b in (("A fwd", "A rev"), ("B fwd", "B rev"), ("B one row", "B one reversed")):
        assert host[a] != host[b], (a, b)
    _classified(hs, "order vectors", concurrency=4)
    for name, h in vec.items():
        _classified((h,), name, concurrency=4)


def _five_bits():
    """lost-write, nonmonotonic-poll, nonmonotonic-send, int-poll-skip, inconsistent-offsets, duplicate and aborted-read in one history"""
    return _h(*(sum((_send(0, "1", m, m - 1) for m in range(1, 6)), [])), *_send(0, "1", 6, 4), *_send(0, "1", 9, typ=":fail"),
              *_poll(1, {"1": [[0, 1], [3, 4]]}), *_poll(1, {"1": [[3, 4]]}), *_poll(2, {"1": [[5, 9]]}), *_poll(2, {"1": [[6, 1]]}))


MULTI = (E.encode_kafka_history(_BAD["int_skip"]), E.encode_kafka_history(_five_bits()))


def test_several_anomalies_in_one_history(lib):
    """nothing stops at the first anomaly: all bits and all counts accumulate"""
    host = _host_of(MULTI)
    assert _names(host[0]["error_count"]) == {"lost-write", "int-poll-skip"} and host[0]["lost_count"] == 2
    assert _names(host[1]["error_count"]) >= {"lost-write", "nonmonotonic-poll", "nonmonotonic-send", "int-poll-skip", "inconsistent-offsets", "duplicate",
                                              "aborted-read"}, _names(host[1]["error_count"])
    assert host[1]["lost_count"] >= 2 and host[1]["duplicated_count"] >= 1
    _classified(MULTI, "several anomalies")


def test_corrupted_oracle_histories_stay_on_the_device(lib):
    """the 72 mutated oracle histories of tests/test_kafka_check_gpu.py: every record the host's and none handed over (the encoder
    refuses what does not decode, the mutations leave `process` alone, offsets stay below 200).  With the hand-made ones at least eight
    of the nine anomaly bits occur."""
    hs = K.corrupted_family()
    host = _host_of(hs)
    assert len(hs) == 72 and sum(h["error_count"] != 0 for h in host) >= 20
    dev = _classified(hs, "corrupted family")
    seen = set()
    for h in host + _host_of(ALL_HS) + _host_of(MULTI):
        seen |= _names(h["error_count"])
    print("anomalies seen:", sorted(seen), "census of the family:", E.kafka_anomaly_census(dev))
    assert len(seen - {"malformed"}) >= 8, seen
    for h in hs[::9]:
        _classified((h,), "one of the family alone")


def test_anomaly_census(lib):
    hs = K.corrupted_family()
    host = _host_of(hs)
    dev, _ = E.classify_kafka_batch(list(hs), 3)
    want = {name: sum(bool(h["error_count"] & b) for h in host) for b, name in A.KAFKA_ANOMALIES.items()}
    want["clean"] = sum(h["error_count"] == 0 for h in host)
    assert E.kafka_anomaly_census(dev) == want and want["clean"] < 72 and sum(want.values()) >= 72


def _shared_wavefront(procs):
    """a nonmonotonic send of procs[0], a nonmonotonic poll of procs[1] and an internal one of procs[2], their rows interleaved"""
    a, b, c = procs
    s1, s2 = _send(a, "1", 1, 3), _send(a, "1", 2, 3)
    p1, p2 = _poll(b, {"2": [[0, 1], [1, 2]]}), _poll(b, {"2": [[1, 2]]})
    p3 = _poll(c, {"3": [[1, 2], [0, 1]]})
    return _h(*s1, *p1, *p3, *s2, *p2)


def _long_poll():
    """a poll of 300 pairs of one key — 255 + 5 + 40 messages in three blocks, the third block's header at payload word 133, beyond the
    128 words a wavefront stages — that jumps over offsets 260 and 261, which were acknowledged"""
    pairs = [[o, o + 1] for o in range(260)] + [[o, o + 1] for o in range(262, 302)]
    return _h(*_send(0, "2", 261, 260), *_send(0, "2", 262, 261), *_poll(1, {"2": pairs}))


def _word_boundaries():
    """offsets 31 / 32 / 63 / 64 (a 32-entry table's last entry, the bit words' edges): 32 is lost, message 64 is seen at 63 and at 64"""
    return _h(*_send(0, "1", 32, 31), *_send(0, "1", 33, 32), *_send(0, "1", 64, 63), *_send(0, "1", 65, 64),
              *_poll(1, {"1": [[31, 32]]}), *_poll(2, {"1": [[63, 64], [64, 64]]}))


def _at_offset(o):
    return _h(*_send(0, "1", 5, o), *_poll(1, {"1": [[o, 7]]}))


EDGES = {
    # name: (ops, concurrency, bits the host must find (a subset), histories handed over)
    "concurrency 9, workers 0 / 8 in wavefront 0": (_shared_wavefront((0, 8, 8)), 9, {"nonmonotonic-send", "nonmonotonic-poll", "int-nonmonotonic-poll"}, 0),
    "concurrency 64, workers 1 / 9 / 17 in wavefront 1": (_shared_wavefront((1, 9, 17)), 64, {"nonmonotonic-send", "nonmonotonic-poll", "int-nonmonotonic-poll"}, 0),
    "a replaced process, sends": (_h(*_send(1, "1", 1, 5), *_send(4, "1", 2, 0)), 3, set(), 0),
    "a replaced process, polls": (_h(*_poll(1, {"1": [[4, 5]]}), *_poll(4, {"1": [[0, 1]]})), 3, set(), 0),
    "the same polls by ONE process": (_h(*_poll(1, {"1": [[4, 5]]}), *_poll(1, {"1": [[0, 1]]})), 3, {"nonmonotonic-poll"}, 0),
    "a skip behind payload word 128": (_long_poll(), 3, {"int-poll-skip", "lost-write"}, 0),
    "offsets 31 / 32 / 63 / 64": (_word_boundaries(), 3, {"lost-write", "duplicate"}, 0),
    "offset 1151, the tables' last": (_at_offset(T_BOUND - 1), 3, {"inconsistent-offsets"}, 0),
    "offset 1152, beyond the tables": (_at_offset(T_BOUND), 3, {"inconsistent-offsets"}, 1),
    "offset 2046, the layout's last": (_at_offset(2046), 3, {"inconsistent-offsets"}, 1),
}
EDGE_HS = {name: (E.encode_kafka_history(ops),) for name, (ops, _, _, _) in EDGES.items()}


@pytest.mark.parametrize("edge", list(EDGES))
def test_edges(lib, edge):
    """a batch of one each (the tables' size follows from what the launch names)"""
    _, conc, bits, handed = EDGES[edge]
    hs = EDGE_HS[edge]
    found = _names(_host_of(hs)[0]["error_count"])
    assert found >= bits and (bits or not found), (edge, found)
    _classified(hs, edge, concurrency=conc, n_host=handed)


EMPTY_HS = ((np.zeros(0, dtype=E.OP_DT), np.zeros(1, dtype=np.uint32)),)


def test_a_history_with_zero_rows(lib):
    assert _host_of(EMPTY_HS)[0]["valid"] == 2
    _classified(EMPTY_HS, "zero rows")
    both = EMPTY_HS + (BAD_HS["dup"],) + EMPTY_HS
    _HOST.pop(id(both), None)
    _classified(both, "zero rows beside an unclean history")


def test_engine_check_classify(lib):
    """Engine.check(classify=True) on a kafka context: msim_set_check_classify accepts it and the records are check()'s, byte for byte,
    with nothing handed to the host.  The built-in node produces no unclean history, so this covers the switch and the unchanged clean
    records only; the unclean route is the batch entry's, through the same kafka_dev_run."""
    cfg = E.test_config("kafka", node_count=4, rate=100, time_limit=6, latency=5, nemesis=["partition"], nemesis_interval=2, seed=12)
    with E.Engine(cfg) as eng:
        eng.run(0, 96)
        eng.check()
        plain = eng.check_results().tobytes()
        assert A.load().msim_set_check_classify(eng._ctx, 1) == 0
        eng.check(classify=True)
        assert eng.check_results().tobytes() == plain and eng.check_host_rechecks() == 0
        assert (eng.check_results()["valid"] == 1).all()
        eng.check()
        assert eng.check_results().tobytes() == plain
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        assert A.load().msim_set_check_classify(eng._ctx, 1) == A.E_UNSUPPORTED


def test_poisoned_allocations(lib):
    """this module again in a process of its own with every device allocation filled with 0xA5 first (MSIM_POISON is read once per
    process): no LDS table, list or record is read before it is written"""
    if os.environ.get("MSIM_POISON"):
        return
    env = dict(os.environ, MSIM_POISON="0xA5")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not poisoned"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
