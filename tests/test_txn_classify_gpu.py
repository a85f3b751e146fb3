"""The device analysis of UNCLEAN list-append histories (csrc/txn_check_dev.hip, txn_classify_kernel: every non-cycle anomaly accumulated,
the tagged edges built, the cycles classified by csrc/cycle_classify.inc) through E.classify_txn_batch (msim_classify_txn_batch) and
Engine.check(classify=True), against the host analysis (msim_check_txn_rows = check_history + finish + classify + judge of
csrc/txn_check.cpp; the `_host` of tests/test_txn_check_synthetic_gpu.py), field by field over FIELDS of tests/test_txn_check_gpu.py.

The yardstick is always the host's record under strict-serializable; for another model the expected `valid` is computed here from that
record (msim_violated_anomalies(error_count, model); no :ok transaction -> 2), every other field does not depend on the model.  No
history reaches the host (n_host == 0) unless it has one of the shapes of test_hand_off; MSIM_DEV_FLAGS bit 0x2000 makes the reachability
matrix 16 transactions wide with no search behind it, so that the host fallback is reached (test_children)."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import test_elle_reference_vectors as V
import test_txn_check_synthetic_gpu as S
from test_txn_check_gpu import FIELDS

pytestmark = pytest.mark.gpu

MODELS = ["strict-serializable", "serializable", "snapshot-isolation", "read-committed", "read-uncommitted"]
BITS = {name: bit for bit, name in A.ANOMALIES.items()}
DEV_FLAGS = int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0)
TINY = bool(DEV_FLAGS & 0x2000)   # a component of more than 16 transactions is the host's: test_children's second child
A_, R_ = ":append", ":r"
_HOST = {}


def _host(hs):
    """the host's strict-serializable records of the histories `hs` (a tuple, kept: computed once per set)"""
    if id(hs) not in _HOST:
        _HOST[id(hs)] = (hs, [S._host(r, p) for r, p in hs])
    return _HOST[id(hs)][1]


def _violates(bits, model):
    lib = A.load()
    lib.msim_violated_anomalies.restype = C.c_uint32
    return lib.msim_violated_anomalies(C.c_uint32(bits), C.c_uint32(E.CONSISTENCY_MODELS[model]))


def _classified(hs, what, model="strict-serializable", n_host=0):
    """one msim_classify_txn_batch call: every record the host's (valid by the model), exactly `n_host` histories handed over
    (None: not asserted).  Returns (records, handed)."""
    host = _host(hs)
    dev, handed = E.classify_txn_batch(list(hs), model)
    for i, h in enumerate(host):
        for f in FIELDS:
            want = int(getattr(h, f))
            if f == "valid" and model != "strict-serializable":
                want = 0 if _violates(int(h.error_count), model) else (2 if int(h.ok_count) == 0 else 1)
            assert int(dev[i][f]) == want, (what, model, i, f, int(dev[i][f]), want, S._names(h.error_count))
    if n_host is not None:
        assert handed == n_host, (what, model, handed, n_host)
    return dev, handed


def _ops(*ops):
    return [{"type": t, "process": p, "f": ":txn", "value": v} for t, p, v in ops]


def _pair(p, req, done=None, typ=":ok"):
    return [(":invoke", p, req), (typ, p, req if done is None else done)]


G2 = [(":invoke", 0, [[R_, 1, None], [A_, 2, 1]]), (":invoke", 1, [[R_, 2, None], [A_, 1, 1]]), (":ok", 0, [[R_, 1, None], [A_, 2, 1]]), (":ok", 1, [[R_, 2, None], [A_, 1, 1]]),
      (":invoke", 2, [[R_, 1, None], [R_, 2, None]]), (":ok", 2, [[R_, 1, [1]], [R_, 2, [1]]])]
HAND = {
    "G0": ([(":invoke", 0, [[A_, 1, 1], [A_, 2, 1]]), (":invoke", 1, [[A_, 1, 2], [A_, 2, 2]]), (":ok", 0, [[A_, 1, 1], [A_, 2, 1]]), (":ok", 1, [[A_, 1, 2], [A_, 2, 2]]),
            (":invoke", 2, [[R_, 1, None], [R_, 2, None]]), (":ok", 2, [[R_, 1, [1, 2]], [R_, 2, [2, 1]]])], {"G0"}),
    "G1c": ([(":invoke", 0, [[A_, 1, 1], [R_, 2, None]]), (":invoke", 1, [[A_, 2, 1], [R_, 1, None]]), (":ok", 0, [[A_, 1, 1], [R_, 2, [1]]]), (":ok", 1, [[A_, 2, 1], [R_, 1, [1]]])], {"G1c"}),
    "G-single": ([(":invoke", 0, [[A_, 1, 1], [A_, 2, 1]]), (":invoke", 1, [[R_, 1, None], [R_, 2, None]]), (":ok", 0, [[A_, 1, 1], [A_, 2, 1]]), (":ok", 1, [[R_, 1, [1]], [R_, 2, None]]),
                  (":invoke", 2, [[R_, 2, None]]), (":ok", 2, [[R_, 2, [1]]])], {"G-single"}),
    "G2": (G2, {"G2"}),
    # two appends that did not overlap, read in the other order: the ww edge against the realtime edge
    "G0-realtime": (_pair(0, [[A_, 1, 1]]) + _pair(1, [[A_, 1, 2]]) + _pair(2, [[R_, 1, None]], [[R_, 1, [2, 1]]]), {"G0", "realtime"}),
    # a read of an append that was invoked after the read had completed
    "G1c-realtime": (_pair(0, [[R_, 1, None]], [[R_, 1, [1]]]) + _pair(1, [[A_, 1, 1]]), {"G1c", "realtime"}),
    "G-single-realtime": (_pair(0, [[A_, 1, 1]]) + _pair(1, [[R_, 1, None]]) + _pair(2, [[R_, 1, None]], [[R_, 1, [1]]]), {"G-single", "realtime"}),   # a stale read
    # A -rw-> B -rw-> C, and C completed before A began; B overlaps both; D shows the version orders
    "G2-realtime": ([(":invoke", 1, [[A_, 1, 1], [R_, 2, None]])] + _pair(2, [[A_, 2, 1]]) + _pair(0, [[R_, 1, None]]) + [(":ok", 1, [[A_, 1, 1], [R_, 2, None]])] +
                    _pair(3, [[R_, 1, None], [R_, 2, None]], [[R_, 1, [1]], [R_, 2, [1]]]), {"G2", "realtime"}),
    "G1a-unwritten": (_pair(0, [[A_, 1, 1]]) + _pair(1, [[R_, 1, None]], [[R_, 1, [1, 9]]]), {"G1a"}),
    "G1a-failed": (_pair(0, [[A_, 1, 1]], typ=":fail") + _pair(1, [[R_, 1, None]], [[R_, 1, [1]]]), {"G1a"}),
    "G1b": ([(":invoke", 0, [[A_, 1, 1], [A_, 1, 2]]), (":invoke", 1, [[R_, 1, None]]), (":ok", 1, [[R_, 1, [1]]]), (":ok", 0, [[A_, 1, 1], [A_, 1, 2]])], {"G1b"}),
    "internal-append-then-nil": (_pair(0, [[A_, 1, 1], [R_, 1, None]]), {"internal"}),
    "internal-read-append-nil": (_pair(0, [[R_, 1, None], [A_, 1, 1], [R_, 1, None]]), {"internal"}),
    "internal-read-append-read": (_pair(0, [[R_, 1, None], [A_, 1, 1], [R_, 1, None]], [[R_, 1, None], [A_, 1, 1], [R_, 1, [1]]]), set()),
    "incompatible-order": (_pair(0, [[A_, 1, 1]]) + _pair(1, [[A_, 1, 2]]) + _pair(2, [[R_, 1, None]], [[R_, 1, [1, 2]]]) + _pair(3, [[R_, 1, None]], [[R_, 1, [2, 1]]]),
                           {"incompatible-order"}),
    "duplicate-elements": (_pair(0, [[A_, 1, 1]]) + _pair(1, [[R_, 1, None]], [[R_, 1, [1, 1]]]), {"duplicate-elements"}),
    "dirty-update": (_pair(0, [[A_, 1, 1]], typ=":fail") + _pair(1, [[A_, 1, 2]]) + _pair(2, [[R_, 1, None]], [[R_, 1, [1, 2]]]), {"dirty-update", "G1a"}),
    "info-append-observed": (_pair(0, [[A_, 1, 1]], typ=":info") + _pair(1, [[R_, 1, None]], [[R_, 1, [1]]]), set()),
    "double-invoke-stray-completion": ([(":invoke", 0, [[A_, 1, 1]]), (":invoke", 0, [[A_, 1, 2]]), (":ok", 0, [[A_, 1, 2]]), (":ok", 0, [[A_, 1, 9]])], set()),
    "all-fail": (_pair(0, [[A_, 1, 1]], typ=":fail") + _pair(1, [[R_, 1, None]], typ=":fail"), set()),
    "empty": ([], set()),
    "two-kinds": (G2 + _pair(3, [[R_, 3, None]], [[R_, 3, [7]]]), {"G2", "G1a"}),
}
HAND_HS = tuple(E.encode_txn_history(_ops(*ops)) for ops, _ in HAND.values())


def test_hand_made_histories(lib):
    """One history per anomaly, 0 - 8 transactions; the expected bits by name (of the host's record, which the device's must equal).
    `internal` through both paths of the check: no earlier read of the key (tests/test_txn_check_gpu.py:75) and one (line 76's shape with
    the last read nil; line 76 itself is consistent: no bit).  A G2-realtime history
    exists: two anti-dependencies closed by one realtime edge, the version orders shown by a later reader."""
    host = _host(HAND_HS)
    for (name, (_, want)), h in zip(HAND.items(), host):
        assert S._names(h.error_count) == want, (name, S._names(h.error_count), want)
    names = list(HAND)
    assert int(host[names.index("all-fail")].valid) == 2 and int(host[names.index("empty")].valid) == 2
    assert int(host[names.index("info-append-observed")].valid) == 1 and int(host[names.index("G2")].valid) == 0
    for model in MODELS:
        _classified(HAND_HS, "hand-made", model)
    for i, hs in enumerate(HAND_HS):        # each alone as well: the batch's capacities follow from its longest history
        _classified((hs,), names[i])


_SETS = {}


def _faulted_hs():
    if "faulted" not in _SETS:
        _SETS["faulted"] = tuple(E.encode_txn_history(ops) for _, ops in S._faulted_set())
    return _SETS["faulted"]


def test_faulted_random_set_stays_on_the_device(lib):
    """tests/test_txn_check_synthetic_gpu.py's 104 histories with one fault each: msim_check_txn_batch hands nearly all of them to the
    host; here none is"""
    hs = _faulted_hs()
    assert len(hs) == 104 and sum(int(h.error_count) != 0 for h in _host(hs)) >= 80
    _classified(hs, "the faulted random set")


def no_isolation(seed, W, K, n_txn, p_fail=0.05, p_info=0.05, sticky=0.0, p_append=0.45):
    """S.generate's scheme on a store WITHOUT isolation: every micro-op takes effect at its own random instant between its transaction's
    invocation and its completion (demo/clojure/txn_rw_register_no_isolation.clj's idea for lists).  :fail has no effect, :info all or none.
    `sticky`: how likely the scheduler stays with a worker that is in the middle of a transaction — 0 interleaves every transaction with
    every other (ww cycles everywhere: all G0), near 1 few micro-ops fall between another transaction's, and the weaker classes show."""
    rnd = random.Random(seed)
    last = None
    ops, lists, nxt = [], {}, {}
    proc = list(range(W))
    cur = [None] * W          # [request, completed micro-ops so far, fate, takes effect?]
    started = 0
    while started < n_txn or any(c is not None for c in cur):
        w = last if last is not None and cur[last] is not None and rnd.random() < sticky else rnd.randrange(W)
        last = w
        c = cur[w]
        if c is None:
            if started == n_txn:
                continue
            mops = []
            for _ in range(rnd.randint(1, 8)):
                k = rnd.randrange(K)
                if rnd.random() < p_append and nxt.get(k, 0) < 254:
                    nxt[k] = nxt.get(k, 0) + 1
                    mops.append([A_, k, nxt[k]])
                else:
                    mops.append([R_, k, None])
            x = rnd.random()
            fate = ":fail" if x < p_fail else ":info" if x < p_fail + p_info else ":ok"
            cur[w] = [mops, [], fate, fate == ":ok" or (fate == ":info" and rnd.random() < 0.5)]
            ops.append({"type": ":invoke", "f": ":txn", "process": proc[w], "value": [list(m) for m in mops]})
            started += 1
        elif c[3] and len(c[1]) < len(c[0]):
            f, k, v = c[0][len(c[1])]
            if f == A_:
                lists.setdefault(k, []).append(v)
                c[1].append([f, k, v])
            else:
                c[1].append([f, k, list(lists[k]) if k in lists else None])
        else:
            if not (c[2] == ":info" and rnd.random() < 0.3):          # (else the completion never arrives)
                ops.append({"type": c[2], "f": ":txn", "process": proc[w], "value": c[1] if c[2] == ":ok" else [list(m) for m in c[0]]})
            if c[2] == ":info":
                proc[w] += W
            cur[w] = None
    return ops


# cycles that need a realtime edge and nothing stronger beside them are rare in such a store (about one history in a hundred at three
# workers and ten keys): these (seed, W, K, transactions, sticky, p_append) were found by a search with the host analysis
REALTIME_ONLY = [(106, 3, 10, 102, 0.98, 0.12), (277, 3, 10, 189, 0.99, 0.12), (421, 3, 10, 77, 0.995, 0.25)]
G2_ONLY = [(162, 17, 10, 94, 0.98, 0.12), (450, 17, 10, 190, 0.995, 0.12)]   # likewise: two anti-dependencies and no weaker cycle beside them
WIDE_SINGLE = [(414, 17, 10, 138, 0.99, 0.25), (486, 17, 10, 82, 0.98, 0.12)]  # G-single in a component of 35 / 37: the question the matrix answers


def _no_isolation_ops():
    """64 histories: W from (3, 8, 17), K from (1, 3, 10), 40 .. 200 transactions; the scheduler's stickiness and the share of appends
    vary so that every cycle class is some history's strongest one"""
    if "noiso-ops" not in _SETS:
        rnd = random.Random(4242)
        shapes = [(7000 + i, (3, 8, 17)[i % 3], (1, 3, 10)[(i // 3) % 3], rnd.randint(40, 200), (0.0, 0.9, 0.99, 0.995)[(i // 9) % 4], (0.45, 0.12)[i // 36])
                  for i in range(57)] + REALTIME_ONLY + G2_ONLY + WIDE_SINGLE
        _SETS["noiso-ops"] = [no_isolation(seed, W, K, n, sticky=st, p_append=pa) for seed, W, K, n, st, pa in shapes]
    return _SETS["noiso-ops"]


def _no_isolation_hs():
    if "noiso" not in _SETS:
        _SETS["noiso"] = tuple(E.encode_txn_history(ops) for ops in _no_isolation_ops())
    return _SETS["noiso"]


def test_store_without_isolation(lib):
    """64 histories, W in (3, 8, 17) x K in (1, 3, 10), 40 - 200 transactions: every cycle class and realtime-only cycles occur.  Under
    MSIM_DEV_FLAGS bit 0x2000 (test_children) the components beyond 16 transactions are the host's and the records still equal."""
    hs = _no_isolation_hs()
    host = _host(hs)
    census = {n: sum(bool(int(h.error_count) & BITS[n]) for h in host) for n in BITS}
    print("anomalies of the set without isolation:", census, "largest component:", max(int(h.stale_count) for h in host))
    for n in ("G0", "G1c", "G-single", "G2", "realtime"):
        assert census[n] > 0, census
    assert max(int(h.stale_count) for h in host) > 64 and max(int(h.attempt_count) for h in host) > 128
    # (only G-single against G2 asks what reaches what inside a component: a G0 or G1c history never needs the matrix, however large)
    assert any(int(h.stale_count) > 16 and S._names(h.error_count) & {"G-single", "G2"} for h in host)
    _, handed = _classified(hs, "no isolation", n_host=None)
    assert (handed > 0) if TINY else (handed == 0), handed


def _chain(k):
    """k single-append transactions one after the other on distinct keys, then a read of the first's key as nil: one component of k + 1"""
    ops = []
    for i in range(k):
        ops += _pair(0, [[A_, i, 1]])
    ops += _pair(1, [[R_, 0, None]]) + _pair(2, [[R_, 0, None]], [[R_, 0, [1]]])   # (the last reader shows key 0's version order; it follows the cycle)
    return E.encode_txn_history(_ops(*ops))


CHAINS = tuple(_chain(s - 1) for s in (16, 17, 255, 256, 257, 600))


def test_component_sizes_around_the_matrix(lib):
    """a realtime chain closed by one anti-dependency: components of 16, 17 (the tiny matrix of bits 0x2000 / 0x20000), 255, 256, 257
    (the matrix of 256) and 600 transactions, G-single-realtime each"""
    host = _host(CHAINS)
    for h, s in zip(host, (16, 17, 255, 256, 257, 600)):
        assert S._names(h.error_count) == {"G-single", "realtime"} and int(h.stale_count) == s, (s, S._names(h.error_count), int(h.stale_count))
    _, handed = _classified(CHAINS, "chains", n_host=None)
    assert handed == (5 if TINY else 0), handed
    for hs in CHAINS[:2]:
        _classified((hs,), "a chain alone", n_host=None)


def _open_calls(n_open):
    """n_open calls open at once (S.test_open_calls), one read corrupted with an element nobody appended"""
    s = S.Store()
    for p in range(n_open):
        s.invoke(p, [s.append(p % 5), [R_, (p + 1) % 5, None]])
    for p in reversed(range(n_open)):
        s.complete(p)
    read = next(m for o in s.ops if o["type"] == ":ok" for m in o["value"] if m[0] == R_ and m[2])
    read[2].append(250)
    return s.encode()


def _long_key_stale():
    """a key of 254 elements read at every length mod 4 (S._long_key), then once more 252 elements long: a stale read"""
    s = S._long_key(set(range(0, 10)) | {251, 252, 253, 254})
    s.ops += _ops(*_pair(2, [[R_, 1, None]], [[R_, 1, list(range(1, 253))]]))
    return s.encode()


def test_sizes(lib):
    """1, 63, 64, 65 and 129 transactions (blocks of 64 lanes); 64 calls open at once, the pairing table's width; a list of 254 elements
    read at lengths 0 .. 9 and 251 .. 254 (four elements to a word)"""
    hs = [E.encode_txn_history(_ops(*_pair(0, [[A_, 1, 1], [R_, 1, None]])))]
    hs += [E.encode_txn_history(no_isolation(300 + n, 3, 3, n)) for n in (63, 64, 65, 129)]
    hs += [_open_calls(64), _long_key_stale()]
    hs = tuple(hs)
    host = _host(hs)
    assert [int(h.attempt_count) for h in host[:5]] == [1, 63, 64, 65, 129] and all(int(h.error_count) for h in host), [S._names(h.error_count) for h in host]
    assert S._names(host[6].error_count) == {"G-single", "realtime"}
    _classified(hs, "sizes", n_host=None if TINY else 0)
    for i in range(len(hs)):
        _classified((hs[i],), ("sizes, alone", i), n_host=None if TINY else 0)


@pytest.mark.parametrize("model", MODELS)
def test_models(lib, model):
    """the faulted set and the set without isolation under each consistency model: `valid` by msim_violated_anomalies, the rest unchanged"""
    for name, hs in (("faulted", _faulted_hs()), ("no isolation", _no_isolation_hs())):
        dev, _ = _classified(hs, name, model, n_host=None if TINY else 0)
        if model == "read-uncommitted":
            assert (dev["valid"] == 1).sum() > (np.asarray([int(h.valid) for h in _host(hs)]) == 1).sum(), name   # the weakest model accepts more


def _twice_appended():
    return E.encode_txn_history(_ops(*(_pair(0, [[A_, 1, 1]]) + _pair(1, [[A_, 1, 1]]) + _pair(2, [[R_, 1, None]], [[R_, 1, [1]]]))))


def _payload_outside():
    rows, pay = E.encode_txn_history(_ops(*(_pair(0, [[A_, 1, 1]]) + _pair(1, [[R_, 1, None]], [[R_, 1, [1]]]))))
    rows["value"][3] = len(pay) + 5
    return rows, pay


def _invocations_only():
    return E.encode_txn_history(_ops(*[(":invoke", i % 8, [[A_, i % 3, i // 3 + 1], [R_, 0, None]]) for i in range(200)]))


def _edges_beyond(n=600, reads=17):
    """an append and `reads` reads of the key per transaction: a wr and a rw edge per read, 36 edges per transaction > 32 (n + 65)"""
    s = S.Store()
    for i in range(n):
        s.pair(0, [s.append(i % 3)] + [[R_, i % 3, None]] * reads)
    return s.encode()


HAND_OFF = {
    "a (key, element) appended twice": _twice_appended,
    "a payload outside the area": _payload_outside,
    "key 4096 (KMAX)": lambda: S._keys_and_elements(4096, 1).encode(),
    "key 4095, element 16 (WMAX)": lambda: S._keys_and_elements(4095, 16).encode(),
    "65 open calls": lambda: _open_calls(65),
    "more transactions than rows / 2 + 65": _invocations_only,
    "more than 32 edges per transaction": _edges_beyond,
}


@pytest.mark.parametrize("shape", list(HAND_OFF))
def test_hand_off(lib, shape):
    """the shapes that are the host's, a batch each (a batch's capacities follow from its longest history): n_host counts the history
    and the record is the host's"""
    hs = (HAND_OFF[shape](),)
    _classified(hs, shape, n_host=1)
    if shape == "more than 32 edges per transaction":
        assert int(_host(hs)[0].lost_count) > 32 * (600 + 65)


def test_capacities_at_their_edge_stay_on_the_device(lib):
    """one below each of test_hand_off's table capacities, unclean, in a batch each: none goes to the host"""
    def unclean(s):
        s.ops += _ops(*_pair(9, [[R_, 0, None]], [[R_, 0, [250]]]))
        return s.encode()
    for name, hs in (("key 4095, element 15", unclean(S._keys_and_elements(4095, 15))), ("64 open calls", _open_calls(64))):
        hs = (hs,)
        assert int(_host(hs)[0].error_count) != 0
        _classified(hs, name)


def test_elle_doc_vectors(lib):
    """the reference documentation's transactions (tests/test_elle_reference_vectors.py) through the new entry"""
    hs = tuple(E.encode_txn_history(v["history"]) for v in V.VECTORS)
    dev, _ = _classified(hs, "elle doc vectors")
    assert (dev["valid"] == 0).all()


def test_engine_check_classify(lib):
    """Engine.check(classify=True) on a txn-list-append context: msim_set_check_classify accepts it and the records are check()'s, byte
    for byte, with nothing handed to the host.  The built-in nodes are strict-serializable and produce no unclean history, so this
    covers the switch and the unchanged clean records only; the unclean route is the batch entry's, through the same txn_dev_run."""
    cfg = E.test_config("txn-list-append", node_count=3, rate=80.0, time_limit=5.0, latency=5, seed=11)
    with E.Engine(cfg) as eng:
        eng.run(0, 16)
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


CHILDREN = {
    "0x20000": (dict(MSIM_DEV_FLAGS="0x20000"), "not children"),         # a matrix of 16: small components take the search
    "0x2000": (dict(MSIM_DEV_FLAGS="0x2000"), "store_without_isolation or component_sizes"),   # and no search: the host finishes them
    "0x10000": (dict(MSIM_DEV_FLAGS="0x10000"), "not children"),         # at most 7 histories per launch
    "poison": (dict(MSIM_POISON="0xA5"), "not children"),                # device allocations filled: nothing read before it is written
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
