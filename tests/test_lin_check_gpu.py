"""The lin-kv linearizability search on the device (csrc/lin_check_dev.hip) where it is hard: histories of a Raft cluster under
partitions, whose timed-out writes and cas stay pending for the rest of their key — more than 64 configurations while one call returns,
the keys pass 1's registers give up on.  Passes 2 and 3 (a workgroup per history, the configurations in an LDS hash table) and the host
search (csrc/lin_check.cpp) for what is left must report, field by field, what the host search alone reports — on the valid histories
and on copies with one read changed (mostly not linearizable).  With MSIM_DEV_FLAGS bit 13 (0x2000) the pools are small enough that
every level is reached, the host included.  The batch entry reads that switch from the environment once per process, so the cases
that need it run this file's own tests again in a child process that has the variable before the library is loaded, one child after
the other; with bit 12 (0x1000, the developer trace: the `[lin-check]` lines on stderr) the child also asserts which level took which
history.  The trace keeps its timings in otherwise unused fields of the records, so a traced run compares ROUTE_FIELDS only and the
untraced one every field.  tests/linearizable_ref.py (an independent search without the dominance / symmetry pruning) confirms
the verdict on the changed keys.  tests/test_hipemu_parity.py runs this file on the host wavefront emulator in the CPU suite."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import oracle_lib as O

pytestmark = pytest.mark.gpu
FIELDS = ("valid", "attempt_count", "error_count", "op_count", "ok_count", "fail_count", "info_count", "stable_count", "lost_count", "stale_count",
          "never_read_count", "duplicated_count")
ROUTE_FIELDS = ("valid", "attempt_count", "error_count", "op_count", "ok_count", "fail_count", "info_count")   # what a traced run leaves alone
DEV_FLAGS = int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0)   # of this process: what the batch entry will read
TRACED, TINY = bool(DEV_FLAGS & 0x1000), bool(DEV_FLAGS & 0x2000)


def _host(rows):
    res = A.CheckResult()
    rows = np.ascontiguousarray(rows)
    assert A.load().msim_check_lin_kv_rows(rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(res)) == 0
    return res


def _histories(n, time_limit=40, payloads=False):
    cfg = E.test_config("lin-kv", bin="raft", node_count=5, rate=30, time_limit=time_limit, latency=10, nemesis=["partition"], nemesis_interval=10, seed=99)
    ora = O.run(cfg, 0, n)
    assert (ora.meta["flags"] == 0).all()
    if payloads:
        return [(ora.history(i)[0].copy(), ora.history(i)[1].copy()) for i in range(n)]
    return [ora.history(i)[0].copy() for i in range(n)]


def _with_one_read_changed(rows, rng):
    """a copy with the value of one :ok read (of the busier second half, where the partitions are) replaced"""
    rows = rows.copy()
    packed = rows["packed"]
    idx = np.nonzero(((packed & 3) == A.T_OK) & (((packed >> 2) & 31) == A.F_READ))[0]
    idx = idx[idx > len(rows) // 3]
    i = int(idx[rng.integers(len(idx))])
    v = int(rows["value"][i])
    old = (v >> 8) & 0xFF
    new = (old + 1 + int(rng.integers(3))) % 5 if old != 0xFF else int(rng.integers(5))
    rows["value"][i] = (v & ~0xFF00) | (new << 8)
    return rows


def _same_as_host(dev, hs, what=""):
    for i, rows in enumerate(hs):
        h = _host(rows)
        for f in (ROUTE_FIELDS if TRACED else FIELDS):
            assert int(dev[i][f]) == int(getattr(h, f)), (what, i, f, int(dev[i][f]), int(getattr(h, f)))


def _routes(err):
    """what the developer trace of ONE msim_check_lin_kv_batch call says: histories that claimed a pool in pass 1, still open after it, moved on to an HBM pool in
    pass 2, still open after pass 2, given to the host search, and of those the ones with more than 23 calls pending on a key"""
    assert err.count("[lin-check] done at") == 1, err
    m = re.search(r"pass 1 \(.*?(\d+) histories claimed a pool, (\d+) of (\d+) still open", err)
    r = {"pool1": int(m.group(1)), "open1": int(m.group(2)), "n": int(m.group(3)), "grown": 0, "open2": 0, "host": 0, "slots": 0}
    m = re.search(r"pass 2 \(.*?(\d+) histories moved on to an HBM pool of \d+\) done at [\d.]+ ms, (\d+) histories still open", err)
    if m:
        r["grown"], r["open2"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"(\d+) histories needed the host search \((\d+) of them", err)
    if m:
        r["host"], r["slots"] = int(m.group(1)), int(m.group(2))
    assert (r["open1"] == 0) == (re.search(r"pass 2 \(", err) is None), err
    return r


def _batch(hs, capfd):
    """check_lin_kv_batch and, in a traced process, what its trace says (else None)"""
    capfd.readouterr()
    dev = E.check_lin_kv_batch(hs)
    err = capfd.readouterr().err
    assert TRACED == ("[lin-check]" in err), err
    return dev, (_routes(err) if TRACED else None)


def _in_child(flags, test):
    """this file's `test` (a node id's tail) in a process of its own under MSIM_DEV_FLAGS = flags"""
    assert DEV_FLAGS == 0
    env = dict(os.environ, MSIM_DEV_FLAGS=hex(flags))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__) + "::" + test],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("flags", [0, 0x2000, 0x3000])
def test_wide_keys_device_equals_host(lib, flags, capfd):
    """[0]: under the switches this process has.  [8192] (0x2000): case [0] in a child with the small pools, every field; [12288]
    (0x3000): the same with the trace, which must show histories at every level: open after pass 1, moved on to an HBM pool, open after
    pass 2, given to the host search."""
    if flags:
        return _in_child(flags, "test_wide_keys_device_equals_host[0]")
    rng = np.random.default_rng(5)
    good = _histories(40)
    hs = good + [_with_one_read_changed(h, rng) for h in good]
    dev, routes = _batch(hs, capfd)
    _same_as_host(dev, hs)
    n_invalid = sum(int(dev[i]["valid"]) == 0 for i in range(len(hs)))
    assert all(int(dev[i]["valid"]) == 1 for i in range(len(good)))
    assert n_invalid >= len(good) // 2   # a changed read is almost always a register value nobody wrote in time
    if routes:
        print("lin-kv routes of the 80 wide-key histories:", routes)
        assert routes["n"] == len(hs) and routes["open1"] > 0, routes
        if TINY:
            assert routes["grown"] > 0 and routes["open2"] > 0 and routes["host"] > 0, routes


def test_changed_reads_agree_with_the_independent_search(lib):
    import linearizable_ref as L
    rng = np.random.default_rng(6)
    good = _histories(6, time_limit=20, payloads=True)
    hs = [_with_one_read_changed(h, rng) for h, _ in good]
    dev = E.check_lin_kv_batch(hs)
    for rows, (_, pay), d in zip(hs, good, dev):
        ref = L.check(E.decode_history(rows, pay, 5, A.WL_LIN_KV))
        assert int(d["attempt_count"]) == len(ref) and int(d["error_count"]) == sum(1 for ok in ref.values() if not ok)


def _synthetic(seed, n_ops, keys, workers, p_overlap, p_wrong, p_fail, p_info, odd=0.0):
    """A lin-kv history built by hand: mostly operations that complete before the next begins (the runs the device's pair paths of
    round 6 take in one step: pair_rows / search_key in csrc/lin_check_dev.hip), with — at the given rates — operations that overlap,
    results no register ever held, :fail and :info completions, and (`odd`) rows no client produces: a completion without an invocation,
    a process that invokes twice."""
    import random
    rnd = random.Random(seed)
    ops, open_ops = [], []     # open: (process, key, f, v1, v2)
    reg = {}
    t = 0
    free = list(range(workers))
    done = 0
    while done < n_ops or open_ops:
        t += rnd.randrange(1, 2_000_000)
        start = done < n_ops and free and (not open_ops or rnd.random() < p_overlap)
        if start:
            p = free.pop(rnd.randrange(len(free)))
            k = rnd.choice(keys)
            f = rnd.choice([":read", ":write", ":cas"])
            v1, v2 = rnd.randrange(5), rnd.randrange(5)
            val = [k, None] if f == ":read" else ([k, v1] if f == ":write" else [k, [v1, v2]])
            ops.append({"type": ":invoke", "f": f, "process": p, "value": val, "time": t})
            open_ops.append((p, k, f, v1, v2)); done += 1
            if rnd.random() < odd:   # the same process again, before its completion
                ops.append({"type": ":invoke", "f": f, "process": p, "value": val, "time": t + 1})
            continue
        if not open_ops:
            continue
        p, k, f, v1, v2 = open_ops.pop(rnd.randrange(len(open_ops)))
        x = rnd.random()
        cur = reg.get(k)
        if x < p_fail or (f == ":cas" and cur != v1 and rnd.random() >= p_wrong):
            typ = ":fail"
        elif x < p_fail + p_info:
            typ = ":info"
        else:
            typ = ":ok"
        if typ == ":info" and f != ":read" and rnd.random() < 0.5:   # an indeterminate write / cas may have happened
            if f == ":write": reg[k] = v1
            elif cur == v1: reg[k] = v2
        if typ == ":ok":
            if f == ":write": reg[k] = v1
            elif f == ":cas": reg[k] = v2
            else:
                v1 = cur if rnd.random() >= p_wrong else rnd.randrange(5)
        val = [k, v1] if f != ":cas" else [k, [v1, v2]]
        ops.append({"type": typ, "f": f, "process": p, "value": val, "time": t})
        if rnd.random() < odd:   # a completion nobody invoked
            ops.append({"type": ":ok", "f": ":read", "process": 90 + rnd.randrange(5), "value": [k, rnd.randrange(5)], "time": t + 1})
        free.append(p)
    return ops


def test_synthetic_histories_device_equals_host(lib):
    """Sequential runs (the device's pair paths), overlaps, wrong results, :fail / :info, several keys interleaved, rows no client produces:
    field by field what the host search reports."""
    import random
    rnd = random.Random(77)
    hs = []
    for i in range(60):
        hs.append(_synthetic(1000 + i, n_ops=rnd.randrange(20, 400), keys=list(range(rnd.choice([1, 1, 2, 5]))), workers=rnd.choice([1, 2, 4, 10]),
                             p_overlap=rnd.choice([0.0, 0.05, 0.3]), p_wrong=rnd.choice([0.0, 0.0, 0.01, 0.1]), p_fail=rnd.choice([0.0, 0.1]),
                             p_info=rnd.choice([0.0, 0.0, 0.02]), odd=rnd.choice([0.0, 0.0, 0.02])))
    rows = [E.encode_lin_kv_history(h) for h in hs]
    dev = E.check_lin_kv_batch(rows)
    verdicts = set()
    for i, r in enumerate(rows):
        h = _host(r)
        for f in FIELDS:
            assert int(dev[i][f]) == int(getattr(h, f)), (i, f, int(dev[i][f]), int(getattr(h, f)))
        verdicts.add(int(dev[i]["valid"]))
    assert {0, 1} <= verdicts


def _info_then_pairs(reads, f_info="write", completion="end", second_key=False):
    """Key 0 holds 1; process 0's write of 3 (or cas 1 -> 3) never returns — an :info row right after it, at the end, or none — and
    process 1 then runs clean invoke / :ok pairs on key 0 (the device's pair fast path once nothing is pending): reads of `reads` (a list
    of values), then a cas from the last value read and reads of what it wrote.  `second_key`: process 2's clean pairs on key 1 in between."""
    ops, t = [], [0]

    def op(typ, p, f, val):
        t[0] += 1000
        ops.append({"type": typ, "f": f, "process": p, "value": val, "time": t[0]})

    def pair(p, f, val, out=None):
        op(":invoke", p, f, val if f != ":read" else [val[0], None])
        op(":ok", p, f, out if out is not None else val)

    def other(j):
        if second_key:
            pair(2, ":write", [1, j % 7]) if j % 3 == 0 else pair(2, ":read", [1, None], [1, (j - j % 3) % 7])

    pair(1, ":write", [0, 1])
    info = [0, 3] if f_info == "write" else [0, [1, 3]]
    op(":invoke", 0, ":" + f_info, info)
    if completion == "early":
        op(":info", 0, ":" + f_info, info)
    for j, v in enumerate(reads):
        pair(1, ":read", [0, None], [0, v])
        other(j)
    last = reads[-1]
    pair(1, ":cas", [0, [last, 4]])
    for j in range(40):
        pair(1, ":read", [0, None], [0, 4])
        other(len(reads) + j)
    if completion == "end":
        op(":info", 0, ":" + f_info, info)
    return ops


@pytest.mark.parametrize("second_key", [False, True])
@pytest.mark.parametrize("completion", ["early", "end", "none"])
@pytest.mark.parametrize("f_info", ["write", "cas"])
def test_info_call_then_clean_pairs_device_equals_host_and_reference(lib, f_info, completion, second_key):
    """the pair fast path of the device search (csrc/lin_check_dev.hip) runs only while no call is open; an :info write / cas
    never returns, so it stays open for the rest of its key.  Long runs of clean pairs after one: reads consistent only if it took effect
    (at once, or only after many reads of the old value), only if it did not, and reads that see it and then the old value again (not
    linearizable) — device, host search and tests/linearizable_ref.py agree on every key."""
    import linearizable_ref as L
    shapes = {"took": ([3] * 60, True), "took-late": ([1] * 60 + [3] * 60, True), "not": ([1] * 120, True),
              "back": ([3] * 30 + [1] * 30, False), "late-back": ([1] * 30 + [3] * 30 + [1], False)}
    hs = {name: _info_then_pairs(reads, f_info, completion, second_key) for name, (reads, _) in shapes.items()}
    rows = [E.encode_lin_kv_history(h) for h in hs.values()]
    dev = E.check_lin_kv_batch(rows)
    for i, (name, h) in enumerate(hs.items()):
        host = _host(rows[i])
        for f in FIELDS:
            assert int(dev[i][f]) == int(getattr(host, f)), (name, f, int(dev[i][f]), int(getattr(host, f)))
        ref = L.check(h)
        want = shapes[name][1]
        assert ref[0] is want, (name, ref)
        assert all(ref[k] for k in ref if k != 0), (name, ref)
        assert int(dev[i]["attempt_count"]) == len(ref) and int(dev[i]["error_count"]) == sum(1 for ok in ref.values() if not ok), (name, dev[i], ref)
        assert int(dev[i]["valid"]) == int(all(ref.values())), (name, dev[i], ref)


def _pending_on_one_key(n_info, n_ok, reads, info_rows=True):
    """Key 0 holds 1.  `n_info` processes invoke writes of 10, 11, ... that never return (their :info rows at the very end), then `n_ok`
    processes invoke writes of 100, 101, ... and only then complete :ok one after the other: n_info + n_ok calls of one key pending at
    once while the first of them returns (with n_ok = 7 its closure has more than a thousand configurations: the pool's).  Then process
    1 runs clean read pairs over `reads`."""
    ops, t = [], [0]

    def op(typ, p, f, val):
        t[0] += 1000
        ops.append({"type": typ, "f": f, "process": p, "value": val, "time": t[0]})

    op(":invoke", 1, ":write", [0, 1]); op(":ok", 1, ":write", [0, 1])
    for i in range(n_info):
        op(":invoke", 10 + i, ":write", [0, 10 + i])
    for j in range(n_ok):
        op(":invoke", 100 + j, ":write", [0, 100 + j])
    for j in range(n_ok):
        op(":ok", 100 + j, ":write", [0, 100 + j])
    for v in reads:
        op(":invoke", 1, ":read", [0, None]); op(":ok", 1, ":read", [0, v])
    if info_rows:
        for i in range(n_info):
            op(":info", 10 + i, ":write", [0, 10 + i])
    return ops


@pytest.mark.parametrize("flags", [0, 0x1000])
def test_pending_calls_on_one_key(lib, flags, capfd):
    """22, 23 and 24 calls of one key pending at once.  A configuration in a pool is one word with 23 bits for the calls it has linearized
    (csrc/lin_check_dev.hip: P_LIN; search_key's `pending >> 23`): a closure that needs the pool with 24 calls pending is the host's, with
    23 and fewer it is not; the registers and the host search hold 64.
      * writes only: n never-returning writes, then clean read pairs.  Dominance leaves n + 1 configurations, so the registers answer
        all three: no history claims a pool or stays open after pass 1 (the limit of 23 is the pool's, not the key's);
      * 7 of the n calls return :ok after all were invoked: the first return's closure outgrows the registers and every history claims
        a pool in pass 1.  24 -> open after pass 1 and pass 2 and given to the host search, counted by the trace under "more than 23
        calls pending on a key"; 22 and 23 -> answered in a pool of pass 1 or pass 2, no history for the host.
    The verdict by construction (tests/linearizable_ref.py has no pruning: 2^22 configurations): every write that returned did so before
    the reads began, so a read sees the last of those (106) or what a never-returning write wrote — each of those values by exactly one
    write, so reading 12, then 14, then 12 again is not linearizable, and neither is a value nobody wrote.
    [0]: every field against the host search, here.  [4096] (0x1000): case [0] in a child with the trace: the routes."""
    if flags:
        return _in_child(flags, "test_pending_calls_on_one_key[0]")
    shapes = {"last ok write": ([106] * 3, 1), "one pending write": ([106, 12, 12, 12], 1), "two, in turn": ([12, 12, 14, 14], 1), "none of them": ([12, 7], 0),
              "back again": ([12, 14, 12], 0), "back to the ok write": ([12, 106], 0)}
    for n in (22, 23, 24):
        for n_ok in (0, 7):
            if n_ok == 0:
                shapes_n = {k: ([v if v != 106 else 1 for v in reads], want) for k, (reads, want) in shapes.items()}   # (no :ok write but the first: 1)
            else:
                shapes_n = shapes
            for info_rows in (True, False):
                hs = [E.encode_lin_kv_history(_pending_on_one_key(n - n_ok, n_ok, reads, info_rows)) for reads, _ in shapes_n.values()]
                dev, routes = _batch(hs, capfd)
                _same_as_host(dev, hs, (n, n_ok, info_rows))
                for d, (name, (_, want)) in zip(dev, shapes_n.items()):
                    assert (int(d["valid"]), int(d["attempt_count"]), int(d["error_count"])) == (want, 1, 1 - want), (n, n_ok, info_rows, name, d)
                if routes:
                    want = (0, 0, 0) if n_ok == 0 else (len(hs), 0, 0) if n < 24 else (len(hs),) * 3
                    assert (routes["pool1"], routes["host"], routes["slots"]) == want, (n, n_ok, routes)
                    # (whether pass 1's pool of 2048 holds the closure of 22 / 23 calls depends on how many dominated configurations are
                    # admitted in the same instant: pass 1 or pass 2 answers them; with 24 neither does, with writes only the registers do)
                    assert n_ok == 0 and routes["open1"] == 0 or n_ok and (n < 24 or routes["open1"] == routes["open2"] == len(hs)), (n, n_ok, routes)


def _sequential_pairs(n_rows):
    """n_rows rows of clean pairs, one process, three keys in turn: write v, read v, cas v -> v + 1, read v + 1 ...; an odd count ends
    with an invocation that never returns"""
    rows = np.zeros(n_rows, dtype=E.OP_DT)
    i = np.arange(n_rows)
    pair = i // 2
    key, step = pair % 3, pair // 3
    kind = step % 4                       # write a, read a, cas a -> b, read b
    a, b = (step // 4 * 2) % 200, (step // 4 * 2 + 1) % 200
    f = np.choose(kind, [A.F_WRITE, A.F_READ, A.F_CAS, A.F_READ])
    v1 = np.choose(kind, [a, a, a, b])
    v2 = np.choose(kind, [0xFF, 0xFF, b, 0xFF])
    inv = i % 2 == 0
    v1 = np.where(inv & (f == A.F_READ), 0xFF, v1)
    rows["time_len"] = i * 1000
    rows["packed"] = np.where(inv, A.T_INVOKE, A.T_OK) | (f << 2) | (3 << 12)
    rows["value"] = key | (v1 << 8) | (v2 << 16)
    return rows


@pytest.mark.parametrize("flags", [0, 0x1000])
def test_row_count_at_the_outcome_table(lib, flags, capfd):
    """The LDS table of the calls' outcomes covers 24 * 1024 rows (lin_check_dev_run: table_cap): a history of exactly that many rows is
    the device's, one row more is the host's and comes back with the host's record; each also with one read changed (not linearizable).
    [0]: every field against the host search.  [4096] (0x1000): case [0] in a child with the trace: the routes."""
    if flags:
        return _in_child(flags, "test_row_count_at_the_outcome_table[0]")
    cap = 24 * 1024
    for n in (cap, cap + 1):
        good = _sequential_pairs(n)
        assert len(good) == n and E.check_lin_kv_history(good[:3000])["valid?"] is True
        bad = good.copy()
        j = n // 2 * 2 - 3              # the completion of a late pair ...
        while (int(bad["packed"][j]) >> 2) & 31 != A.F_READ or int(bad["packed"][j]) & 3 != A.T_OK:
            j -= 2
        bad["value"][j] = int(bad["value"][j]) ^ (0x55 << 8)   # ... reads a value nobody wrote
        for rows, want in ((good, 1), (bad, 0)):
            dev, routes = _batch([rows], capfd)
            _same_as_host(dev, [rows], n)
            assert (int(dev[0]["valid"]), int(dev[0]["attempt_count"]), int(dev[0]["error_count"])) == (want, 3, 1 - want), (n, dev[0])
            assert int(dev[0]["op_count"]) == (n + 1) // 2 and int(dev[0]["ok_count"]) == n // 2
            if routes:
                assert (routes["open1"], routes["host"]) == ((1, 1) if n > cap else (0, 0)), (n, routes)
