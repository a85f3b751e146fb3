"""Histories for the explaining lin-kv check (msim_explain_lin_kv_rows / _batch; include/maelsim.h msim_lin_key_result): small ones
written out by hand with what the record must say, and a generator of a few hundred rows for the device tests.  TEST INFRASTRUCTURE."""
import random

import numpy as np

NO = 0xFFFFFFFF
NIL = 0xFF


def _inv(p, f, val):
    return {"type": ":invoke", "f": ":" + f, "process": p, "value": val}


def _ok(p, f, val):
    return {"type": ":ok", "f": ":" + f, "process": p, "value": val}


def _fail(p, f, val):
    return {"type": ":fail", "f": ":" + f, "process": p, "value": val}


def _info(p, f, val):
    return {"type": ":info", "f": ":" + f, "process": p, "value": val}


def _w(p, k, v):
    return [_inv(p, "write", [k, v]), _ok(p, "write", [k, v])]


def _r(p, k, v):
    return [_inv(p, "read", [k, None]), _ok(p, "read", [k, v])]


# name -> (ops, {key: the fields the record must have}); the rows are the ops' indices
HAND = {
    "sequential and valid": (
        _w(0, 0, 1) + _r(0, 0, 1) + [_inv(0, "cas", [0, [1, 2]]), _ok(0, "cas", [0, [1, 2]])] + _r(1, 0, 2),
        {0: dict(valid=1, op_row=NO, previous_ok_row=NO, n_pending=0, n_values=1, values=[2])}),
    "a stale read": (
        _w(0, 0, 1) + _w(0, 0, 2) + _r(1, 0, 1),
        {0: dict(valid=0, op_row=5, previous_ok_row=3, n_pending=0, n_values=1, values=[2])}),
    "the first operation fails": (
        _r(0, 0, 3) + _w(0, 0, 1),
        {0: dict(valid=0, op_row=1, previous_ok_row=NO, n_pending=0, n_values=1, values=[NIL])}),
    "an :ok cas from a value nobody wrote": (
        _w(0, 0, 1) + [_inv(1, "cas", [0, [3, 4]]), _ok(1, "cas", [0, [3, 4]])],
        {0: dict(valid=0, op_row=3, previous_ok_row=1, n_pending=0, n_values=1, values=[1])}),
    "two overlapping writes, two final values": (
        [_inv(0, "write", [0, 1]), _inv(1, "write", [0, 2]), _ok(0, "write", [0, 1]), _ok(1, "write", [0, 2])],
        {0: dict(valid=1, op_row=NO, previous_ok_row=NO, n_pending=0, n_values=2, values=[1, 2])}),
    "an :info write stays open": (
        [_inv(0, "write", [0, 1]), _inv(1, "write", [0, 2]), _inv(2, "write", [0, 3]), _ok(0, "write", [0, 1]), _ok(1, "write", [0, 2]), _info(2, "write", [0, 3])],
        {0: dict(valid=1, op_row=NO, previous_ok_row=NO, n_pending=1, n_values=2, values=[1, 2])}),   # (a call is linearized no earlier than a return needs it: 3 is not yet a value)
    "a :fail is ignored": (
        _w(0, 0, 1) + [_inv(1, "write", [0, 4]), _fail(1, "write", [0, 4])] + _r(0, 0, 1),
        {0: dict(valid=1, op_row=NO, previous_ok_row=NO, n_pending=0, n_values=1, values=[1])}),
    "an unfinished read is not counted": (
        _w(0, 0, 1) + [_inv(1, "read", [0, None])] + _r(0, 0, 1) + [_inv(2, "read", [0, None]), _info(2, "read", [0, None])],
        {0: dict(valid=1, op_row=NO, previous_ok_row=NO, n_pending=0, n_values=1, values=[1])}),
    "two interleaved keys, one bad": (
        [_inv(0, "write", [7, 1]), _inv(1, "write", [3, 2]), _ok(0, "write", [7, 1]), _ok(1, "write", [3, 2]),
         _inv(0, "read", [3, None]), _inv(1, "read", [7, None]), _ok(1, "read", [7, 4]), _ok(0, "read", [3, 2])],
        {3: dict(valid=1, op_row=NO, previous_ok_row=NO, n_pending=0, n_values=1, values=[2]),
         7: dict(valid=0, op_row=6, previous_ok_row=2, n_pending=0, n_values=1, values=[1])}),
    # key 0 holds 1, a write of 3 stays open; reads see 1, then 3 (the open write took effect), then 1 again: row 8 cannot return.  The
    # open write is invoked and never completed, so it counts as pending although every configuration before row 8 has linearized it.
    "an open write beside the failing read": (
        _w(0, 0, 1) + [_inv(2, "write", [0, 3])] + _r(1, 0, 1) + _r(1, 0, 3) + _r(1, 0, 1),
        {0: dict(valid=0, op_row=8, previous_ok_row=6, n_pending=1, n_values=1, values=[3])}),
}


def with_nemesis(ops):
    """the same history with nemesis rows in between (they are no key's rows: the row indices shift, nothing else)"""
    out = []
    for i, op in enumerate(ops):
        if i % 2 == 1:
            out.append({"type": ":info", "f": ":start-partition" if i % 4 == 1 else ":stop-partition", "process": ":nemesis", "value": None})
        out.append(op)
    return out


def encode(ops):
    """E.encode_lin_kv_history plus nemesis rows (process 0xFFFFF, f start- / stop-partition)"""
    from maelstrom_amd import _abi as A
    from maelstrom_amd import engine as E
    rows = np.zeros(len(ops), dtype=E.OP_DT)
    for i, op in enumerate(ops):
        if op["process"] == ":nemesis":
            f = A.F_START_PARTITION if op["f"] == ":start-partition" else A.F_STOP_PARTITION
            rows[i] = (i * 1000, A.T_INFO | (f << 2) | (A.PROCESS_NEMESIS << 12), A.NO_VALUE)
        else:
            rows[i] = E.encode_lin_kv_history([dict(op, time=i * 1000)])[0]
    return rows


def synthetic(seed, n_rows, keys=(0, 1, 2), workers=6, p_overlap=0.2, p_wrong=0.02, p_fail=0.1, p_info=0.03, odd=0.0, values=5):
    """A lin-kv history of exactly `n_rows` rows: mostly operations that complete before the next begins, with — at the given rates —
    overlapping operations, results no register held, :fail and :info completions and (`odd`) rows no client produces: a completion
    nobody invoked, a process that invokes twice.  What is still open when the rows run out never completes."""
    rnd = random.Random(seed)
    ops, open_ops, reg = [], [], {}
    free = list(range(workers))
    while len(ops) < n_rows:
        if free and (not open_ops or rnd.random() < p_overlap):
            p = free.pop(rnd.randrange(len(free)))
            k = rnd.choice(keys)
            f = rnd.choice(["read", "write", "cas"])
            v1, v2 = rnd.randrange(values), rnd.randrange(values)
            val = [k, None] if f == "read" else [k, v1] if f == "write" else [k, [v1, v2]]
            ops.append(_inv(p, f, val))
            open_ops.append((p, k, f, v1, v2))
            if rnd.random() < odd:
                ops.append(_inv(p, f, val))                     # the same process again, before its completion
            continue
        p, k, f, v1, v2 = open_ops.pop(rnd.randrange(len(open_ops)))
        x, cur = rnd.random(), reg.get(k)
        if x < p_fail or (f == "cas" and cur != v1 and rnd.random() >= p_wrong):
            typ = _fail
        elif x < p_fail + p_info:
            typ = _info
        else:
            typ = _ok
        if typ is _info and f != "read" and rnd.random() < 0.5:   # an indeterminate write / cas may have happened
            if f == "write": reg[k] = v1
            elif cur == v1: reg[k] = v2
        if typ is _ok:
            if f == "write": reg[k] = v1
            elif f == "cas": reg[k] = v2
            else: v1 = cur if rnd.random() >= p_wrong else rnd.randrange(values)
        ops.append(typ(p, f, [k, v1] if f != "cas" else [k, [v1, v2]]))
        if rnd.random() < odd:
            ops.append(_ok(90 + rnd.randrange(5), "read", [k, rnd.randrange(values)]))   # a completion nobody invoked
        free.append(p)
    return ops[:n_rows]


def many_open_calls(n_open, tail_reads=(1,)):
    """key 0 holds 1; `n_open` processes invoke writes that never return, then process 1 reads `tail_reads`: with more than 64 open
    calls the searches answer "unknown" (valid 2)"""
    ops = _w(1, 0, 1)
    for i in range(n_open):
        ops.append(_inv(10 + i, "write", [0, 2 + i % 3]))
    for v in tail_reads:
        ops += _r(1, 0, v)
    return ops


def wide_then_bad_read(n_writes=9, done=3, read_value=99, n_info=0):
    """key 0 holds 1; `n_writes` processes invoke writes of 10, 11, ... (and `n_info` more that never return), `done` of them return :ok
    — after the first, hundreds of configurations survive: every subset of the others with any of its members written last, the pools
    of the device search —, then a read returns `read_value` while the rest are still open, then they return.  A value nobody wrote:
    the read is the :op, the values of the writes that returned are the :configs values, the open writes are pending."""
    ops = _w(1, 0, 1)
    ops += [_inv(100 + i, "write", [0, 10 + i]) for i in range(n_writes)]
    ops += [_inv(200 + i, "write", [0, 50 + i]) for i in range(n_info)]
    ops += [_ok(100 + i, "write", [0, 10 + i]) for i in range(done)]
    ops += _r(1, 0, read_value)
    ops += [_ok(100 + i, "write", [0, 10 + i]) for i in range(done, n_writes)]
    return ops
