"""txn-list-append's device pass (csrc/txn_check_dev.hip: txn_check_lds_kernel, a workgroup per history with its tables in LDS, and
txn_check_kernel, a wavefront per history with its tables in HBM) on histories no engine run produces: random ones from a generator
of its own and hand-shaped ones that cross each capacity of the two kernels.  Every record is compared field by field with the host
analysis (msim_check_txn_rows; the fields of tests/test_txn_check_gpu.py), histories of at most 300 transactions also with
tests/elle_ref.py (written independently) through test_txn_list_append._agree, so that the host code is not the only judge.

Which level answered a history is read from the library's developer trace (MSIM_DEV_FLAGS bit 12, 0x1000: the `[txn-check]` lines on
stderr), never assumed: how many histories of a batch the LDS kernel passed on ("do not fit"), how many the HBM-table kernel took, how
many went to the host.  The batch entry reads its switches from the environment once per process, so this process compares the records
under the switches it was started with (none: the LDS kernel first), and test_module_again_in_a_child runs the whole module again under
0x1000 (the trace: the routes of the default selection) and 0x3000 (bit 13: every history on the HBM-table kernel, records and routes) in
child processes, one after the other.  The list-append trace leaves the records alone, so a traced run compares every field too.  A
batch's capacities (nmax, emax, the LDS of a workgroup) follow from its longest history, so every group of shaped histories that is meant
to take one route is a batch of its own.

tests/test_hipemu_parity.py runs this module on the host wavefront emulator in the CPU suite — also on a build of txn_check_dev.hip with
-DTC_NO_POTENTIAL, where Kahn's queue (F2) decides every history the LDS kernel keeps: how many sweeps of the potential (F1) a history
needs is not observable from outside, so on the device F2 is only known to run for the two chains of test_kahns_queue."""
import copy
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import test_txn_list_append as T
from test_txn_check_gpu import FIELDS

pytestmark = pytest.mark.gpu

DEV_FLAGS = int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0)   # of this process: what the batch entry will read
TRACED, HBM_ONLY = bool(DEV_FLAGS & 0x1000), bool(DEV_FLAGS & 0x2000)
A_, R_ = ":append", ":r"
CLASSES = ("cycle", "G1a", "G1b", "internal", "incompatible-order", "duplicate-elements", "dirty-update", "realtime")   # what _agree compares


def _host(rows, pay):
    res = A.CheckResult()
    rows = np.ascontiguousarray(rows); pay = np.ascontiguousarray(pay, dtype=np.uint32)
    if len(pay) == 0:
        pay = np.zeros(1, dtype=np.uint32)
    assert A.load().msim_check_txn_rows(rows.ctypes.data_as(C.c_void_p), len(rows), pay.ctypes.data_as(C.c_void_p), len(pay), C.byref(res)) == 0
    return res


def _names(bits):
    return {n for b, n in A.ANOMALIES.items() if int(bits) & b}


def _batch(hs, capfd, what, unfit=None, host=None):
    """One msim_check_txn_batch call over `hs` ((rows, payload) each): every record = the host analysis; in a traced process the routes:
    `unfit` histories leave the LDS kernel for the HBM-table kernel (all of them under bit 13, where the LDS kernel does not run),
    `host` histories go to the host.  Returns (device records, host records)."""
    capfd.readouterr()
    dev = E.check_txn_batch(hs)
    err = capfd.readouterr().err
    hosts = [_host(r, p) for r, p in hs]
    for i, h in enumerate(hosts):
        for f in FIELDS:
            assert int(dev[i][f]) == int(getattr(h, f)), (what, i, f, int(dev[i][f]), int(getattr(h, f)))
    assert TRACED == ("[txn-check]" in err), err
    if TRACED:
        m = re.search(r"LDS pass \(.*?(\d+) of (\d+) histories do not fit", err)
        assert (m is None) == HBM_ONLY, err
        got_unfit = len(hs) if HBM_ONLY else int(m.group(1))
        m = re.search(r"HBM-table pass over (\d+) histories", err)
        assert (int(m.group(1)) if m else 0) == got_unfit, err
        m = re.search(r"device passes: [\d.]+ ms, (\d+) of (\d+) histories for the host", err)
        assert int(m.group(2)) == len(hs), err
        got_host = int(m.group(1))
        print(f"routes of {what}: {len(hs)} histories, {got_unfit} on the HBM-table kernel, {got_host} for the host")
        if unfit is not None and not HBM_ONLY:
            assert got_unfit == unfit, (what, got_unfit, unfit, err)
        if host is not None:
            assert got_host == host, (what, got_host, host, err)
    return dev, hosts


@pytest.mark.parametrize("flags", [0x1000, 0x3000])
def test_module_again_in_a_child(lib, flags):
    """every other test of this module in a process of its own under MSIM_DEV_FLAGS = flags: 4096 (0x1000) the routes of the default
    kernel selection, 12288 (0x3000) records and routes with every history on the HBM-table kernel"""
    assert DEV_FLAGS == 0
    env = dict(os.environ, MSIM_DEV_FLAGS=hex(flags))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not in_a_child"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- a strict-serializable store and its clients ----------------------------------------------------------------------------------------

class Store:
    """The rows of a history as its clients see a strict-serializable list-append store: a transaction takes effect atomically when
    `apply` is called, somewhere between `invoke` and `complete`, so the history is clean by construction whatever the interleaving."""

    def __init__(self):
        self.ops, self.lists, self.next, self.open, self.junk = [], {}, {}, {}, []

    def append(self, k):
        """a micro-op appending the key's next element (unique per key, 1 .. 254)"""
        self.next[k] = self.next.get(k, 0) + 1
        assert self.next[k] <= 254
        return [A_, k, self.next[k]]

    def invoke(self, p, mops):
        self.ops.append({"type": ":invoke", "f": ":txn", "process": p, "value": [[f, k, None if f == R_ else v] for f, k, v in mops]})
        self.open[p] = [mops, None]

    def apply(self, p):
        done = []
        for f, k, v in self.open[p][0]:
            if f == A_:
                self.lists.setdefault(k, []).append(v)
                done.append([f, k, v])
            else:
                done.append([f, k, list(self.lists[k]) if k in self.lists else None])
        self.open[p][1] = done

    def complete(self, p, typ=":ok"):
        mops, done = self.open.pop(p)
        if typ == ":ok" and done is None:
            self.open[p] = [mops, None]; self.apply(p); done = self.open.pop(p)[1]
        self.ops.append({"type": typ, "f": ":txn", "process": p, "value": done if typ == ":ok" else [[f, k, None if f == R_ else v] for f, k, v in mops]})

    def pair(self, p, mops, typ=":ok"):
        self.invoke(p, mops); self.complete(p, typ)

    def other_row(self, kind):
        """a row that is not a transaction's: the nemesis', or a client's with another f (patched into `packed` by `encode`)"""
        self.junk.append((len(self.ops), kind))
        self.ops.append({"type": ":info" if kind == "nemesis" else ":ok", "f": ":txn", "process": 3, "value": []})

    def encode(self):
        rows, pay = E.encode_txn_history(self.ops)
        for i, kind in self.junk:
            if kind == "nemesis":
                rows["packed"][i] = (int(rows["packed"][i]) & 0xFFF) | (A.PROCESS_NEMESIS << 12)
            else:
                rows["packed"][i] = (int(rows["packed"][i]) & ~(31 << 2)) | (A.F_READ << 2)
        return rows, pay

    def client_ops(self):
        skip = {i for i, _ in self.junk}
        return [o for i, o in enumerate(self.ops) if i not in skip]


def generate(seed, W, K, n_txn, p_fail=0.05, p_info=0.05):
    """W worker threads over K keys, n_txn transactions of 1 .. 8 micro-ops; each takes effect at a random instant between its invocation
    and its completion; :fail has no effect, :info may or may not, and its thread goes on under a new process id (+ W, as Jepsen's)."""
    rnd = random.Random(seed)
    s = Store()
    proc = list(range(W))
    state = [0] * W           # 0 idle, 1 invoked, 2 took effect (or will not)
    fate = [":ok"] * W
    started = 0
    while started < n_txn or any(state):
        w = rnd.randrange(W)
        if state[w] == 0:
            if started == n_txn:
                continue
            mops = []
            for _ in range(rnd.randint(1, 8)):
                k = rnd.randrange(K)
                mops.append(s.append(k) if rnd.random() < 0.45 and s.next.get(k, 0) < 254 else [R_, k, None])
            s.invoke(proc[w], mops)
            x = rnd.random()
            fate[w] = ":fail" if x < p_fail else ":info" if x < p_fail + p_info else ":ok"
            state[w] = 1; started += 1
        elif state[w] == 1:
            if fate[w] == ":ok" or (fate[w] == ":info" and rnd.random() < 0.5):
                s.apply(proc[w])
            state[w] = 2
        else:
            if fate[w] == ":info" and rnd.random() < 0.3:
                s.open.pop(proc[w])          # (the completion never arrives)
            else:
                s.complete(proc[w], fate[w])
            if fate[w] == ":info":
                proc[w] += W
            state[w] = 0
    return s


SHAPES = [(W, K) for W in (1, 3, 16, 17, 40) for K in (1, 3, 50)]
_CLEAN = []


def _clean_set():
    """105 clean histories, seven of each (W, K), 20 .. 600 transactions (generated once per process)"""
    if not _CLEAN:
        rnd = random.Random(2024)
        out = []
        for i in range(105):
            W, K = SHAPES[i % len(SHAPES)]
            n = rnd.choice([rnd.randint(20, 80), rnd.randint(80, 300), rnd.randint(300, 600)])
            if K == 1:
                n = min(n, 110)      # (one key holds 254 elements)
            out.append(generate(5000 + i, W, K, n))
        _CLEAN.append(out)
    return _CLEAN[0]


def test_random_clean_histories(lib, capfd):
    """the host analysis finds nothing in any of them (the generator's claim, asserted) and neither kernel hands one to the host; 17 and
    40 workers put more than 16 processes into a block of 64 rows: those histories are the HBM-table kernel's"""
    stores = _clean_set()
    hs = [s.encode() for s in stores]
    dev, hosts = _batch(hs, capfd, "the clean random set", host=0)
    for i, h in enumerate(hosts):
        assert int(h.error_count) == 0 and int(h.valid) == 1 and int(h.stale_count) == 0, (i, SHAPES[i % len(SHAPES)], _names(h.error_count))
    assert max(int(h.attempt_count) for h in hosts) > 500 and sum(int(h.info_count) > 0 for h in hosts) > 50


def test_random_clean_histories_agree_with_the_python_restatement(lib):
    if DEV_FLAGS:
        return   # (host code against Python: nothing a switch of the device pass changes)
    n = 0
    for s in _clean_set():
        if sum(o["type"] == ":invoke" for o in s.ops) <= 300:
            assert T._agree(s.ops)["valid?"] is True
            n += 1
    assert n >= 40


FAULTS = ("pop", "swap", "dup", "unwritten", "nil", "later-state", "failed-append", "intermediate")


def _inject(s, how, rnd):
    """a copy of the store's ops with one read of an :ok transaction corrupted; None where the history has no read to corrupt that way"""
    ops = copy.deepcopy(s.ops)
    reads = [(oi, mi) for oi, o in enumerate(ops) if o["type"] == ":ok" for mi, m in enumerate(o["value"]) if m[0] == R_ and m[2] and len(m[2]) >= 2]
    if not reads:
        return None
    oi, mi = rnd.choice(reads)
    k = ops[oi]["value"][mi][1]
    lst = ops[oi]["value"][mi][2]
    if how == "pop":
        lst.pop()                                   # one version behind
    elif how == "swap":
        lst[0], lst[-1] = lst[-1], lst[0]           # incompatible order
    elif how == "dup":
        lst.append(lst[0])                          # duplicate element
    elif how == "unwritten":
        lst.append(s.next[k] + 1 if s.next[k] < 254 else 0)   # an element nobody appended
    elif how == "nil":
        ops[oi]["value"][mi][2] = None              # sees nothing although elements were visible
    elif how == "later-state":                      # the key's final list, in an early read of it
        final = s.lists[k]
        early = [(a, b) for a, b in reads if ops[a]["value"][b][1] == k and len(ops[a]["value"][b][2]) + 2 <= len(final)]
        if not early:
            return None
        oi, mi = early[0]
        ops[oi]["value"][mi][2] = list(final)
    elif how == "failed-append":                    # an element a :fail transaction would have appended, in a read's list
        failed = [(m[1], m[2]) for o in ops if o["type"] == ":fail" for m in o["value"] if m[0] == A_]
        cand = [(a, b) for a, b in reads for fk, _ in failed if ops[a]["value"][b][1] == fk]
        if not cand:
            return None
        oi, mi = rnd.choice(cand)
        k = ops[oi]["value"][mi][1]
        lst = ops[oi]["value"][mi][2]
        lst.insert(rnd.randrange(len(lst) + 1), rnd.choice([v for fk, v in failed if fk == k]))
    elif how == "intermediate":                     # a read that ends between two appends of one transaction to the key
        cand = []
        for o in ops:
            if o["type"] != ":ok":
                continue
            for kk in {m[1] for m in o["value"] if m[0] == A_}:
                vs = [m[2] for m in o["value"] if m[0] == A_ and m[1] == kk]
                if len(vs) >= 2:
                    cand += [(a, b, vs[0]) for a, b in reads if ops[a] is not o and ops[a]["value"][b][1] == kk and vs[-1] in ops[a]["value"][b][2]]
        if not cand:
            return None
        oi, mi, v0 = rnd.choice(cand)
        lst = ops[oi]["value"][mi][2]
        del lst[lst.index(v0) + 1:]
    return ops


_FAULTED = []


def _faulted_set():
    if not _FAULTED:
        rnd = random.Random(77)
        out = []
        i = 0
        while len(out) < 104:
            how = FAULTS[len(out) % len(FAULTS)]
            W, K = [(3, 3), (16, 3), (3, 1), (17, 3), (5, 50), (40, 3)][i % 6]
            s = generate(9000 + i, W, K, rnd.randint(20, 110 if K == 1 else 280), p_fail=0.12)
            i += 1
            ops = _inject(s, how, rnd)
            if ops is not None:
                out.append((how, ops))
        _FAULTED.append(out)
    return _FAULTED[0]


def test_random_histories_with_one_fault(lib, capfd):
    """13 of each fault.  Whatever the host calls anomalous reached the host (the device never decides an unclean history): the records
    are the host's and the trace counts exactly those histories; every class of anomaly test_txn_list_append._agree compares occurs."""
    fs = _faulted_set()
    hs = [E.encode_txn_history(ops) for _, ops in fs]
    hosts = [_host(r, p) for r, p in hs]
    unclean = sum(int(h.error_count) != 0 for h in hosts)
    assert all(int(h.valid) == 1 for h in hosts if int(h.error_count) == 0)
    _batch(hs, capfd, "the faulted random set", host=unclean)
    census = {c: 0 for c in CLASSES}
    for h in hosts:
        names = _names(h.error_count)
        for c in CLASSES:
            census[c] += bool(names & T.CYCLES) if c == "cycle" else c in names
    print("anomaly classes of the faulted random set:", census, "unclean:", unclean, "of", len(hs),
          {how: sum(int(h.error_count) != 0 for (w, _), h in zip(fs, hosts) if w == how) for how in FAULTS})
    assert all(census.values()), census
    assert unclean >= 80, unclean


def test_random_histories_with_one_fault_agree_with_the_python_restatement(lib):
    if DEV_FLAGS:
        return
    n_bad = 0
    for _, ops in _faulted_set():
        n_bad += T._agree(ops)["valid?"] is False
    assert n_bad >= 80


# ---- shaped histories: one capacity each --------------------------------------------------------------------------------------------------

def _serial(s, p, n_pairs, k, reads=True):
    """n_pairs transactions of process p one after the other: append to key k, and read it"""
    for _ in range(n_pairs):
        s.pair(p, [s.append(k)] + ([[R_, k, None]] if reads else []))


def _agree_small(stores):
    if not DEV_FLAGS:
        for s in stores:
            T._agree(s.client_ops())


def test_processes_per_block(lib, capfd):
    """a block of 64 rows with exactly 16 distinct processes stays in the LDS kernel (TC_PROCS entries per block); with 17 the history
    leaves it for the HBM-table kernel, which decides it"""
    def shape(n_procs):
        s = Store()
        for i in range(64):                 # 128 rows: two blocks, the same processes in both
            s.pair(i % n_procs, [s.append(i % 3), [R_, (i + 1) % 3, None]])
        return s
    for n_procs, unfit in ((16, 0), (17, 1)):
        s = shape(n_procs)
        assert len({o["process"] for o in s.ops[:64]}) == n_procs and len(s.ops) == 128
        dev, _ = _batch([s.encode()], capfd, f"{n_procs} processes in a block", unfit=unfit, host=0)
        assert int(dev[0]["valid"]) == 1 and int(dev[0]["attempt_count"]) == 64
        _agree_small([s])


def test_open_calls(lib, capfd):
    """64 calls open at once are what the HBM-table kernel's pairing table holds (a lane each); the 65th sends the history to the host.
    (The LDS kernel passes both on: 64 processes in a block.)"""
    for n_open, host in ((64, 0), (65, 1)):
        s = Store()
        for p in range(n_open):
            s.invoke(p, [s.append(p % 5), [R_, (p + 1) % 5, None]])
        for p in reversed(range(n_open)):
            s.complete(p)
        dev, _ = _batch([s.encode()], capfd, f"{n_open} open calls", unfit=1, host=host)
        assert int(dev[0]["valid"]) == 1 and int(dev[0]["ok_count"]) == n_open
        _agree_small([s])


def test_pairing_across_block_boundaries(lib, capfd):
    """the LDS kernel pairs a completion with the previous row of its process: inside the block of 64 rows, or through the per-block
    lists of the processes' last rows"""
    stores = []
    s = Store(); stores.append(s)               # an invocation in row 63 completed in row 64; another silent for three blocks in between
    _serial(s, 0, 31, 0)
    s.invoke(1, [s.append(1), [R_, 0, None]])   # row 62
    s.invoke(2, [s.append(2), [R_, 1, None]])   # row 63
    assert len(s.ops) == 64
    s.complete(2)                               # row 64
    _serial(s, 0, 100, 3)                       # rows 65 .. 264: blocks 1 .. 4
    s.complete(1)                               # row 265, block 4: three whole blocks without a row of process 1
    _serial(s, 4, 5, 4)
    s = Store(); stores.append(s)               # a second invocation of an open process beyond a boundary: the first call never completes
    _serial(s, 0, 31, 0)
    s.invoke(1, [s.append(1)])                  # row 62
    s.ops.append({"type": ":invoke", "f": ":txn", "process": 5, "value": [[R_, 9, None]]})   # row 63: process 5 never returns
    s.ops.append(dict(s.ops[62]))               # row 64: process 1 invokes the same again
    s.ops[-1]["value"] = [[A_, 1, 7]]
    _serial(s, 0, 40, 3)
    s.ops.append({"type": ":ok", "f": ":txn", "process": 1, "value": [[A_, 1, 7]]})          # completes the SECOND invocation, two blocks later
    s.lists.setdefault(1, []).append(7)
    s.pair(6, [[R_, 1, None]])
    s = Store(); stores.append(s)               # stray completions: after a completed call of an earlier block; of a process never seen
    _serial(s, 0, 30, 0)
    s.pair(1, [s.append(1)])                    # rows 60, 61
    _serial(s, 0, 1, 0)                         # rows 62, 63
    s.ops.append({"type": ":ok", "f": ":txn", "process": 1, "value": [[A_, 1, 9]]})          # row 64: process 1 has nothing open
    s.ops.append({"type": ":fail", "f": ":txn", "process": 8, "value": [[A_, 2, 9]]})        # row 65: nor has process 8
    _serial(s, 0, 40, 3)
    s.ops.append({"type": ":info", "f": ":txn", "process": 1, "value": [[A_, 1, 10]]})       # and again, two blocks later
    s.pair(1, [[R_, 1, None], s.append(1)])
    hs = [s.encode() for s in stores]
    dev, hosts = _batch(hs, capfd, "pairing across blocks", unfit=0, host=0)
    assert [int(d["valid"]) for d in dev] == [1, 1, 1]
    assert int(dev[0]["info_count"]) == 0 and int(dev[0]["ok_count"]) == int(dev[0]["attempt_count"]) == 31 + 2 + 100 + 5
    assert int(dev[1]["attempt_count"]) - int(dev[1]["ok_count"]) == 2      # the replaced invocation and process 5's
    assert int(dev[2]["ok_count"]) == int(dev[2]["attempt_count"]) and int(dev[2]["fail_count"]) == 0 and int(dev[2]["info_count"]) == 0   # strays count nowhere
    _agree_small(stores)


def test_row_counts(lib, capfd):
    """0, 1, 63, 64, 65 and 128 rows, among them the nemesis' rows and clients' rows with another f, which are no transaction's"""
    stores = []
    for n in (0, 1, 63, 64, 65, 128):
        for junk in (False, True):
            s = Store()
            while len(s.ops) < n:
                i = len(s.ops)
                if junk and i % 5 in (1, 3):
                    s.other_row("nemesis" if i % 5 == 1 else "other-f")   # (also between an invocation and its completion)
                elif 7 in s.open:
                    s.complete(7)
                else:
                    s.invoke(7, [s.append(i % 2), [R_, 0, None], [R_, 1, None]])
            assert len(s.ops) == n
            stores.append(s)
    hs = [s.encode() for s in stores]
    dev, _ = _batch(hs, capfd, "row counts", unfit=0, host=0)
    for s, d in zip(stores, dev):
        n_inv = sum(o["type"] == ":invoke" for o in s.client_ops())
        n_ok = sum(o["type"] == ":ok" for o in s.client_ops())
        assert (int(d["attempt_count"]), int(d["ok_count"])) == (n_inv, n_ok) and int(d["valid"]) == (1 if n_ok else 2), (len(s.ops), d)
    # each alone as well: the batch's capacities follow from its longest history
    for s in stores:
        _batch([s.encode()], capfd, f"{len(s.ops)} rows alone", unfit=0, host=0)
    _agree_small(stores)


def _many(n_txn, tail=()):
    """n_txn transactions of one process, one after the other, 200 per key"""
    s = Store()
    for i in range(n_txn):
        s.pair(0, [s.append(i // 200), [R_, i // 200, None]] if i % 50 == 0 else [s.append(i // 200)])
    return s


def test_transaction_counts(lib, capfd):
    """The LDS kernel's writer table has 13-bit transaction numbers: 8190 is the last count it accepts, 8191 goes to the HBM-table kernel
    (A2).  With a workgroup's 78 KiB the tables of more than about 5700 transactions do not fit either way, so the trace shows both
    histories on the HBM-table kernel; what is held here is that both are decided on the device, valid, with the host's edge count."""
    for n in (8190, 8191):
        s = _many(n)
        dev, hosts = _batch([s.encode()], capfd, f"{n} transactions", unfit=1, host=0)
        assert int(dev[0]["valid"]) == 1 and int(dev[0]["attempt_count"]) == n and int(dev[0]["lost_count"]) == int(hosts[0].lost_count) > n


def test_more_transactions_than_rows_allow_for(lib, capfd):
    """invocations only: more transactions than nmax = rows / 2 + 65 of the batch entry — the host's"""
    s = Store()
    for i in range(200):
        s.ops.append({"type": ":invoke", "f": ":txn", "process": i % 8, "value": [[A_, i % 3, i // 3 + 1], [R_, 0, None]]})
    dev, _ = _batch([s.encode()], capfd, "200 invocations in 200 rows", host=1)
    assert int(dev[0]["valid"]) == 2 and int(dev[0]["attempt_count"]) == 200 and int(dev[0]["info_count"]) == 0
    s = Store()
    for i in range(130):                       # 130 <= 130 / 2 + 65: the device's
        s.ops.append({"type": ":invoke", "f": ":txn", "process": i % 8, "value": [[A_, i % 3, i // 3 + 1], [R_, 0, None]]})
    dev, _ = _batch([s.encode()], capfd, "130 invocations in 130 rows", unfit=0, host=0)
    assert int(dev[0]["valid"]) == 2 and int(dev[0]["attempt_count"]) == 130


def _keys_and_elements(max_key, max_el):
    """a short clean history whose highest key is max_key and highest element max_el (elements need not be dense: 1 and max_el)"""
    s = Store()
    s.pair(0, [s.append(0), [R_, max_key, None]])
    s.next[max_key] = max_el - 1
    s.pair(1, [s.append(max_key), [R_, max_key, None]])
    s.pair(0, [[R_, max_key, None], [R_, 0, None], s.append(0)])
    return s


def test_keys_and_the_writer_table(lib, capfd):
    """keys up to 4095 (KMAX) and a writer table of (highest key + 1) x (highest element + 1) <= 65536 entries (WMAX) are the
    HBM-table kernel's (the LDS kernel has no room for such a table); one beyond either is the host's"""
    fits = {"key 4095, element 15": (4095, 15), "key 256, element 254": (256, 254), "key 4095, element 1": (4095, 1)}
    beyond = {"key 4096": (4096, 1), "key 4095, element 16": (4095, 16), "key 257, element 254": (257, 254), "key 32767": (32767, 1)}
    for name, (k, e) in fits.items():
        assert (k + 1) * (e + 1) <= 65536
        dev, _ = _batch([_keys_and_elements(k, e).encode()], capfd, name, unfit=1, host=0)
        assert int(dev[0]["valid"]) == 1
    assert (4095 + 1) * (15 + 1) == 65536
    for name, (k, e) in beyond.items():
        assert k >= 4096 or (k + 1) * (e + 1) > 65536
        dev, _ = _batch([_keys_and_elements(k, e).encode()], capfd, name, unfit=1, host=1)
        assert int(dev[0]["valid"]) == 1
    _agree_small([_keys_and_elements(k, e) for k, e in list(fits.values()) + list(beyond.values())])


def _long_key(reads_at):
    """one key appended 254 times, one transaction each, and read by another process when it holds `reads_at` elements"""
    s = Store()
    s.pair(1, [[R_, 1, None], [R_, 2, None]])
    for i in range(255):
        if i in reads_at:
            s.pair(1, [[R_, 1, None]])
        if i < 254:
            s.pair(0, [s.append(1)])
    return s


def test_read_lists_of_every_length_mod_4(lib, capfd):
    """a read's list is packed four elements to a word: lengths 0 .. 9 and 251 .. 254; nil (the key was never written) against the
    empty list (a value the binary layout can hold and no store returns: the same to both sides)"""
    s = _long_key(set(range(0, 10)) | {251, 252, 253, 254})
    dev, _ = _batch([s.encode()], capfd, "read lists of every length", unfit=0, host=0)
    assert int(dev[0]["valid"]) == 1 and int(dev[0]["attempt_count"]) == 254 + 15
    _agree_small([s])
    empty = copy.deepcopy(s)
    assert empty.ops[1]["value"] == [[R_, 1, None], [R_, 2, None]] and empty.ops[3]["value"] == [[R_, 1, None]]
    empty.ops[1]["value"] = [[R_, 1, []], [R_, 2, None]]
    empty.ops[3]["value"] = [[R_, 1, []]]
    dev, _ = _batch([empty.encode()], capfd, "the empty list for nil", unfit=0, host=0)
    assert int(dev[0]["valid"]) == 1


def test_duplicate_elements_in_each_word_of_the_set(lib, capfd):
    """the duplicates of a read are found with four 64-bit sets: an element twice at 63, 64, 127, 128, 191, 192 and 254, and 1"""
    hs = []
    for x in (1, 63, 64, 127, 128, 191, 192, 254):
        s = _long_key({254})
        read = s.ops[-1]
        assert read["type"] == ":ok" and read["value"][0][2] == list(range(1, 255))
        read["value"][0][2] = list(range(1, 254)) + [x]        # (254 elements still: x in place of the last)
        if x == 254:
            read["value"][0][2] = [254] + list(range(2, 255))
        hs.append(s.encode())
    dev, hosts = _batch(hs, capfd, "duplicate elements", unfit=0, host=len(hs))
    for h in hosts:
        assert "duplicate-elements" in _names(h.error_count) and int(h.valid) == 0


def test_edge_counts(lib, capfd):
    """more dependency edges than the LDS kernel's adjacency holds (what is left of 78 KiB beside the tables of 4000 transactions: about
    three per transaction; these have nine): the HBM-table kernel decides.  More edges than emax = 16 nmax (transactions of an append
    and eight reads of one long key: 18 each): the host's."""
    s = Store()
    for i in range(4000):             # five keys at a time, eight elements each: an append to one, reads of the other four (wr and rw each)
        base = i // 40 * 5
        s.pair(0, [s.append(base + i % 5)] + [[R_, base + (i + j) % 5, None] for j in range(1, 5)])
    dev, hosts = _batch([s.encode()], capfd, "nine dependency edges per transaction", unfit=1, host=0)
    assert int(dev[0]["valid"]) == 1 and 8 * 4000 < int(dev[0]["lost_count"]) <= 16 * (4000 + 65)
    s = Store()
    for i in range(750):
        k = i % 3
        s.pair(0, [s.append(k)] + [[R_, k, None]] * 8)
    dev, hosts = _batch([s.encode()], capfd, "eighteen edges per transaction", host=1)
    assert int(dev[0]["valid"]) == 1 and int(dev[0]["lost_count"]) > 16 * (750 + 65)


@pytest.mark.parametrize("order", ["index", "reversed"])
def test_kahns_queue(lib, capfd, order):
    """Sixty indeterminate single-append transactions on one key among the first 64, observed by one :ok read in the order of their
    numbers (or the reverse): a chain of sixty ww edges between transactions that all start at position 0.  In lockstep a sweep of
    the potential (F1) moves the chain on by one link, 48 sweeps do not settle it, and Kahn's queue (F2) proves it acyclic."""
    s = Store()
    for i in range(60):
        s.invoke(i % 8, [[A_, 1, i + 1]])
        s.ops.append({"type": ":info", "f": ":txn", "process": i % 8, "value": [[A_, 1, i + 1]]})
        s.open.pop(i % 8)
    seen = list(range(1, 61)) if order == "index" else list(range(60, 0, -1))
    s.ops.append({"type": ":invoke", "f": ":txn", "process": 9, "value": [[R_, 1, None]]})
    s.ops.append({"type": ":ok", "f": ":txn", "process": 9, "value": [[R_, 1, seen]]})
    _serial(s, 10, 3, 2)
    dev, hosts = _batch([s.encode()], capfd, f"a chain of sixty in {order} order", unfit=0, host=0)
    assert int(dev[0]["valid"]) == 1 and int(dev[0]["info_count"]) == 60 and int(dev[0]["lost_count"]) >= 60
    _agree_small([s])
