"""The histories tests/test_txn_findings.py (host entry against tests/txn_findings_ref.py) and tests/test_txn_findings_gpu.py (device
entries against the host entry) walk: cases(rw) -> {name: (rows, payload)}, built once per process; is_hand_off(name) says which of them
the device hands to the host walk.  rw False: txn-list-append, True: txn-rw-register."""
from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import test_rw_classify_gpu as RWT
import test_txn_classify_gpu as T

CAP = A.TXN_FINDINGS_CAPACITY
A_, R_, W_ = ":append", ":r", ":w"
SIZES = (1, 63, 64, 65, 129)
COUNTS = (0, 1, 63, 64, 65, CAP, CAP + 1)
_CASES = {}


def garbage_reads(n, first_key=0):
    """exactly n G1a findings and nothing else: transactions that each read up to 63 elements nobody appended, a key each"""
    ops, key = [], first_key
    if n == 0:
        ops += T._pair(0, [[A_, first_key, 1]]) + T._pair(0, [[R_, first_key, None]], [[R_, first_key, [1]]])
    while n > 0:
        k = min(n, 63)
        ops += T._pair(key % 5, [[R_, key, None]], [[R_, key, list(range(1, k + 1))]])
        n -= k; key += 1
    return E.encode_txn_history(T._ops(*ops))


def _la(*ops):
    return E.encode_txn_history(T._ops(*ops))


def _rw(ops):
    return E.encode_txn_history(ops, rw=True)


def _list_append():
    c = {"hand: " + name: h for name, h in zip(T.HAND, T.HAND_HS)}
    c.update({f"faulted {i}": h for i, h in enumerate(T._faulted_hs())})
    c.update({f"no isolation {i}": h for i, h in enumerate(T._no_isolation_hs())})
    c["1 transactions"] = _la(*T._pair(0, [[A_, 1, 1], [R_, 1, None]]))
    c.update({f"{n} transactions": E.encode_txn_history(T.no_isolation(300 + n, 3, 3, n)) for n in SIZES[1:]})
    c.update({f"{n} findings": garbage_reads(n) for n in COUNTS})
    # two anomalies on one (transaction, micro-op): the read misses the own append (internal) and holds an element nobody appended, twice
    # (G1a at two positions, duplicate-elements)
    c["internal, G1a and duplicate on one read"] = _la(*T._pair(0, [[A_, 1, 1], [R_, 1, None]], [[A_, 1, 1], [R_, 1, [9, 9]]]))
    # key 0 and the highest key of a history (4095: the device's tables end there)
    c["key 0 and key 4095"] = _la(*(T._pair(0, [[R_, 0, None]], [[R_, 0, [3]]]) + T._pair(1, [[A_, 4095, 1], [A_, 4095, 2]]) +
                                    T._pair(2, [[R_, 4095, None]], [[R_, 4095, [1]]]) + T._pair(3, [[R_, 4095, None]], [[R_, 4095, [2, 1]]])))
    # an internal finding with an earlier read, an order longer than the read that contradicts it, a read longer than the order's common part
    c["internal after a read"] = _la(*T._pair(0, [[R_, 1, None], [A_, 1, 5], [A_, 1, 6], [R_, 1, None]], [[R_, 1, [1]], [A_, 1, 5], [A_, 1, 6], [R_, 1, [1, 5]]]))
    c["reads that part ways"] = _la(*(T._pair(0, [[A_, 1, 1]]) + T._pair(1, [[A_, 1, 2]]) + T._pair(2, [[A_, 1, 3]]) + T._pair(3, [[R_, 1, None]], [[R_, 1, [1, 2, 3]]]) +
                                      T._pair(4, [[R_, 1, None]], [[R_, 1, [1, 3]]]) + T._pair(5, [[R_, 1, None]], [[R_, 1, [1, 3, 2]]])))
    # a failed append under two committed ones, the failed writer never read as last
    c["dirty update in the middle"] = _la(*(T._pair(0, [[A_, 1, 1]]) + T._pair(1, [[A_, 1, 2]], typ=":fail") + T._pair(2, [[A_, 1, 3]]) +
                                            T._pair(3, [[R_, 1, None]], [[R_, 1, [1, 2, 3]]])))
    c.update({"hand-off: " + name: make() for name, make in T.HAND_OFF.items()})
    # (k, v) appended by three micro-ops, two of them of one transaction; two rows outside the payload area
    c["hand-off: appended three times"] = _la(*(T._pair(0, [[A_, 1, 1], [A_, 1, 1]]) + T._pair(1, [[A_, 1, 1]], typ=":info") + T._pair(2, [[R_, 1, None]], [[R_, 1, [1]]])))
    rows, pay = T._payload_outside()
    rows["value"][0] = len(pay) + 9
    c["hand-off: two payloads outside the area"] = (rows, pay)
    return c


def _rw_ops(*txns):
    return RWT._ops(*txns)


def _rw_register():
    c = {"hand: " + name: h for name, h in zip(RWT.HAND, RWT.HAND_HS)}
    c.update({f"random {i}": h for i, h in enumerate(RWT._random_hs())})
    w = RWT._w
    c["internal after a write"] = _rw(_rw_ops((0, ":ok", [w(1, 1), [R_, 1, None]], [w(1, 1), [R_, 1, 2]])))
    c["internal after a read"] = _rw(_rw_ops((0, ":ok", [w(1, 1)], [w(1, 1)]), (1, ":ok", [[R_, 1, None], [R_, 1, None]], [[R_, 1, 1], [R_, 1, None]])))
    c["G1a unwritten"] = _rw(_rw_ops((0, ":ok", [[R_, 1, None]], [[R_, 1, 7]])))
    c["G1a failed"] = _rw(_rw_ops((0, ":fail", [w(1, 1)], [w(1, 1)]), (1, ":ok", [[R_, 1, None]], [[R_, 1, 1]])))
    c["G1b"] = _rw(RWT._concurrent((0, ":ok", [w(1, 1), w(1, 2)], [w(1, 1), w(1, 2)]), (1, ":ok", [[R_, 1, None], [R_, 0, None]], [[R_, 1, 1], [R_, 0, None]])))
    # a cycle of three versions of key 2, with a version that follows the cycle and is not on it; key 0 is clean
    c["cyclic-versions"] = _rw(RWT._concurrent(*[(p, ":ok", [[R_, 2, None], w(2, b)], [[R_, 2, a], w(2, b)]) for p, (a, b) in enumerate([(1, 2), (2, 3), (3, 1), (3, 4)])],
                                               (5, ":ok", [w(0, 1)], [w(0, 1)])))
    c["1 transactions"] = _rw(_rw_ops((0, ":ok", [w(1, 1), [R_, 1, None]], [w(1, 1), [R_, 1, None]])))
    c.update({f"{n} transactions": _rw(RWT.synth(900 + n, n)) for n in SIZES[1:]})
    # finding counts: a transaction of k reads of values nobody wrote, a key each (a register read holds one value)
    for n in COUNTS:
        txns, key, left = [], 0, n
        if n == 0:
            txns.append((0, ":ok", [w(0, 1)], [w(0, 1)]))
        while left > 0:
            k = min(left, 60)
            txns.append((key % 4, ":ok", [[R_, key + j, None] for j in range(k)], [[R_, key + j, 9] for j in range(k)]))
            left -= k; key += k
        c[f"{n} findings"] = _rw(_rw_ops(*txns))
    c["internal and G1a in one transaction"] = _rw(_rw_ops((0, ":ok", [[R_, 1, None], [R_, 1, None]], [[R_, 1, 5], [R_, 1, 6]])))
    c["key 0 and key 4095"] = _rw(_rw_ops((0, ":ok", [[R_, 0, None], [R_, 4095, None]], [[R_, 0, 3], [R_, 4095, 4]])))
    c["hand-off: a (key, value) written twice"] = _rw(_rw_ops((0, ":ok", [w(1, 1)], [w(1, 1)]), (1, ":info", [w(1, 1), w(1, 1)], [w(1, 1), w(1, 1)]),
                                                              (2, ":ok", [[R_, 1, None]], [[R_, 1, 1]])))
    # (rw_classify_kernel keeps such rows on the device: two findings with equal order keys, in row order)
    rows, pay = _rw(_rw_ops((0, ":ok", [w(1, 1)], [w(1, 1)]), (1, ":ok", [[R_, 1, None]], [[R_, 1, 2]]), (2, ":ok", [[R_, 1, None]], [[R_, 1, 1]])))
    rows["value"][3] = len(pay) + 5; rows["value"][4] = len(pay) + 1
    c["two payloads outside the area"] = (rows, pay)
    return c


def cases(rw):
    if rw not in _CASES:
        _CASES[rw] = _rw_register() if rw else _list_append()
    return _CASES[rw]


def is_hand_off(name):
    """the device hands the history to the host walk: the shapes of the classify kernels, and one finding more than the region holds"""
    return name.startswith("hand-off: ") or name == f"{CAP + 1} findings"


WORKLOAD = {False: "txn-list-append", True: "txn-rw-register"}
