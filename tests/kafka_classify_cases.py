"""Kafka histories for the device classification's tests (tests/test_kafka_classify_gpu.py) and its timing tool
(tools/kafka_classify_ab.py): the 72 corrupted oracle histories of tests/test_kafka_check_gpu.py's
test_corrupted_histories_equal_the_host_checker (the same seed, the same mutations), the histories whose host record depends on the
order of the observations, and raw rows / payload where the Python encoder cannot express a block order."""
import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import oracle_lib as O
from test_kafka import _cfg, _h, _ops, _poll, _send

_CACHE = {}


def corrupted_ops():
    """72 op lists: 3 oracle histories x 24 trials of 1 - 3 mutations each (a pair deleted from a poll, an offset pushed up, a message
    replaced, a poll rotated, an acknowledged send's offset pulled down, an :info send turned into a :fail)."""
    if "ops" in _CACHE:
        return _CACHE["ops"]
    cfg = _cfg(node_count=3, rate=80.0, time_limit=5.0)
    o = O.run(cfg, 0, 3)
    rng = np.random.default_rng(9)
    out = []
    for i in range(3):
        ops = _ops(*o.history(i), 3)
        for trial in range(24):
            mut = [dict(op) for op in ops]
            for _ in range(1 + trial % 3):
                op = mut[int(rng.integers(len(mut)))]
                if op["f"] == ":poll" and op["type"] == ":ok" and len(op["value"][0]) > 1:
                    msgs = {k: [list(p) for p in v] for k, v in op["value"][0][1].items()}
                    ks = [k for k in msgs if msgs[k]]
                    if ks:
                        k = ks[int(rng.integers(len(ks)))]
                        what = int(rng.integers(4))
                        if what == 0:
                            del msgs[k][int(rng.integers(len(msgs[k])))]
                        elif what == 1:
                            msgs[k][-1][0] += int(rng.integers(1, 4))
                        elif what == 2:
                            msgs[k][-1][1] = int(rng.integers(1, 30))
                        else:
                            msgs[k] = msgs[k][1:] + msgs[k][:1]                       # out of order inside one poll
                    op["value"] = [[":poll", msgs]]
                elif op["f"] == ":send" and op["type"] == ":ok":
                    v = op["value"][0]
                    op["value"] = [[":send", v[1], [max(0, v[2][0] - int(rng.integers(0, 3))), v[2][1]]]]
                elif op["f"] == ":send" and op["type"] == ":info" and trial % 4 == 0:
                    op["type"] = ":fail"                                                # its message may have been polled: aborted read
            out.append([dict(op, index=n_) for n_, op in enumerate(mut)])
    _CACHE["ops"] = out
    return out


def corrupted_family():
    """the 72 histories as (rows, payload), encoded once"""
    if "hs" not in _CACHE:
        _CACHE["hs"] = tuple(E.encode_kafka_history(ops) for ops in corrupted_ops())
    return _CACHE["hs"]


def raw_history(*ops):
    """(rows, payload) built as include/maelsim.h lays them out.  ops: ("send", type, process, key, msg, offset) — offset 0x7FF when
    the op carries none — or ("poll", process, [(key, first offset, [messages]) ...]): an :ok poll whose blocks are exactly these, in
    this order (the encoder would merge runs that continue one another)."""
    rows = np.zeros(len(ops), dtype=E.OP_DT)
    pay = []
    for i, op in enumerate(ops):
        if op[0] == "send":
            _, typ, p, k, m, o = op
            rows[i] = (i * 1000, typ | (A.F_SEND << 2) | (p << 12), k | (m << 6) | (o << 17))
        else:
            _, p, blocks = op
            at = len(pay)
            for k, o0, ms in blocks:
                pay.append(k | (len(ms) << 8) | (o0 << 16))
                for e in range(0, len(ms), 2):
                    pay.append(ms[e] | ((ms[e + 1] << 16) if e + 1 < len(ms) else 0))
            rows[i] = (i * 1000 | ((len(pay) - at) << 48), A.T_OK | (A.F_POLL << 2) | (p << 12), at)
    return rows, np.asarray(pay if pay else [0], dtype=np.uint32)


def order_vectors():
    """name -> (rows, payload): pairs of histories that hold the same observations in another order, and whose host records differ.
    A: a message whose send failed and another one at the same offset: aborted-read iff the failed one is observed LAST.
    B: message 1 at offsets 0 and 1, message 2 at offsets 2 and 1: offset 1 is one duplicate's second home when message 2 is first
    seen at 2, and offset 2 becomes another when message 2 is first seen at 1 — across rows and inside one poll."""
    fail = _send(0, "1", 1, typ=":fail")
    return {
        "A fwd": E.encode_kafka_history(_h(*fail, *_poll(1, {"1": [[0, 1]]}), *_poll(2, {"1": [[0, 2]]}))),
        "A rev": E.encode_kafka_history(_h(*fail, *_poll(2, {"1": [[0, 2]]}), *_poll(1, {"1": [[0, 1]]}))),
        "B fwd": E.encode_kafka_history(_h(*_poll(1, {"1": [[0, 1], [1, 1]]}), *_poll(2, {"1": [[2, 2]]}), *_poll(3, {"1": [[1, 2]]}))),
        "B rev": E.encode_kafka_history(_h(*_poll(1, {"1": [[0, 1], [1, 1]]}), *_poll(3, {"1": [[1, 2]]}), *_poll(2, {"1": [[2, 2]]}))),
        "B one row": raw_history(("poll", 1, [(1, 0, [1, 1]), (1, 2, [2]), (1, 1, [2])])),
        "B one reversed": raw_history(("poll", 1, [(1, 0, [1, 1]), (1, 1, [2]), (1, 2, [2])])),
    }
