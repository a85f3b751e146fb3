"""The net journal's messages on the device (journal_messages_kernel, csrc/journal_dev.hip) through E.journal_messages_batch and
Engine.journal_messages, against the host entry (msim_journal_messages_rows; tests/test_journal_messages.py holds that to the contract's
Python restatement): summary and the whole record slab byte for byte, and exactly the journals that are not well-formed handed to the
host walk."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import journal_cases as K
from test_journal_messages import ACK_RETRY, CASES, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = "_emu" in os.path.basename(A.LIB_PATH)
if not EMU:
    import torch   # before the engine's library is loaded, as in bench.py: the process then holds one HIP runtime, torch's


def _same(got_summary, got_slab, events, cap, what, n_nodes=K.N, slots=K.SLOTS, flags=0):
    w_sum, w_slab = host(events, cap, n_nodes, slots)
    w_sum = w_sum.copy()
    w_sum["flags"] |= flags
    assert got_summary.tobytes() == w_sum.tobytes(), (what, cap, got_summary, w_sum)
    assert got_slab.tobytes() == w_slab.tobytes(), (what, cap, got_slab[:4], w_slab[:4])


def test_batch_equals_the_host_entry(lib):
    """every case in ONE launch, for four capacities of the record slab: roomy, none, one, and one record short of a case's sends"""
    names = list(CASES)
    n_msgs = [int(host(CASES[n][0], 0)[0]["n_msgs"]) for n in names]
    for cap in (max(n_msgs) + 3, 0, 1, n_msgs[names.index("W + 1 events")] - 1):
        summ, msgs, handed = E.journal_messages_batch([CASES[n][0] for n in names], K.N, K.SLOTS, cap, with_n_host=True)
        for i, n in enumerate(names):
            _same(summ[i], msgs.slab[i], CASES[n][0], cap, n)
        assert handed == sum(CASES[n][1] for n in names) == len(K.malformed())


def test_single_journals(lib):
    """a launch of one journal, the empty one too"""
    for n in ("empty", "a lone send", "2W + 1 events", "a double recv"):
        summ, msgs, handed = E.journal_messages_batch([CASES[n][0]], K.N, K.SLOTS, 8, with_n_host=True)
        _same(summ[0], msgs.slab[0], CASES[n][0], 8, n)
        assert handed == CASES[n][1]


_CHUNKS = """
import sys
sys.path.insert(0, {tests!r})
from maelstrom_amd import engine as E
import journal_cases as K
from test_journal_messages import CASES, host
big = [n for n in CASES if len(CASES[n][0]) > 200]
names = [n for n in big if not CASES[n][1]][:11] + [n for n in big if CASES[n][1]][:4]   # (the hand-overs in the last, partial launch)
assert len(names) == 15
summ, msgs, handed = E.journal_messages_batch([CASES[n][0] for n in names], K.N, K.SLOTS, 300, with_n_host=True)
for i, n in enumerate(names):
    w_sum, w_slab = host(CASES[n][0], 300)
    assert summ[i].tobytes() == w_sum.tobytes() and msgs.slab[i].tobytes() == w_slab.tobytes(), n
assert handed == sum(CASES[n][1] for n in names)
"""


def test_chunked_launches(lib):
    """15 journals at 7 a launch (MSIM_DEV_FLAGS bit 16, read once per process: a child): three launches over one workspace, the last
    partial, first > 0"""
    env = dict(os.environ, MSIM_DEV_FLAGS="0x11000")
    r = subprocess.run([sys.executable, "-c", _CHUNKS.format(tests=os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "journal_messages_kernel over 15 journals (3 launches)" in r.stderr, r.stderr[-2000:]


def _engine_equals_host(eng, cfg, got, cap, flags):
    eng.fetch()
    slots = max(cfg.concurrency, cfg.n_nodes)
    for i, (summ, msgs) in enumerate(got):
        ev = eng.raw_journal(i)
        assert len(ev) == min(eng.meta(i).n_events, cfg.journal_capacity)
        _same(summ, got.slab[i], ev, cap, i, cfg.n_nodes, slots, flags)
        assert int(summ["valid"]) == 1 and len(msgs) == min(int(summ["n_msgs"]), cap)


def test_engine_journals_where_they_lie(lib):
    """broadcast-ack-retry under partitions: the journals of a run analysed in HBM, whole — and capped at 1000 events, where the run is
    flagged and the prefix is analysed"""
    for capacity, cap, flags in ((100000, 2000, 0), (1000, 700, A.JOURNAL_TRUNCATED), (1000, 100, A.JOURNAL_TRUNCATED)):
        cfg = E.test_config(**ACK_RETRY, journal_capacity=capacity)
        with E.Engine(cfg) as eng:
            eng.run(0, 8)
            got = eng.journal_messages(cap)
            assert len(got) == 8
            _engine_equals_host(eng, cfg, got, cap, flags)
            assert all(bool(eng.meta(i).flags & A.FLAG_JOURNAL_OVERFLOW) == bool(flags) for i in range(8))
            s = got[0][0]
            assert int(s["undelivered"][2]) > 0 and E.journal_analysis(*got[0])["delivery"]["truncated"] == bool(flags)


def _poke(ptr, data):
    """writes `data` into the engine's device memory at ptr (the emulator's device memory is host memory)"""
    if EMU:
        C.memmove(ptr, data, len(data))
        return
    class _W:
        pass
    w = _W()
    w.__cuda_array_interface__ = {"shape": (len(data),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    torch.as_tensor(w, device=torch.device("cuda", 0)).copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()


def test_a_damaged_journal_of_a_run_goes_to_the_host_walk(lib):
    """the engine writes no malformed journal, so one is made: the first :send of instance 2 and its :recv change places in the slab
    on the device.  That journal — and no other — comes back as the host walk's: not valid, one orphan recv, every record the walk's"""
    cfg = E.test_config("echo", node_count=2, rate=20, time_limit=3, seed=6, journal_capacity=1000)
    with E.Engine(cfg) as eng:
        eng.run(0, 4)
        eng.fetch()
        ev = eng.raw_journal(2).copy()
        k = int(np.flatnonzero((ev["msg"] >> 8 == ev["msg"][0] >> 8) & (ev["msg"] & 0x80 != 0))[0])
        assert not int(ev["msg"][0]) & 0x80 and k > 0
        db = eng.device_buffers()
        at = db.journal + 2 * cfg.journal_capacity * 16
        _poke(at, ev[k:k + 1].tobytes())
        _poke(at + k * 16, ev[0:1].tobytes())
        ev[[0, k]] = ev[[k, 0]]
        got = eng.journal_messages(600)
        slots = max(cfg.concurrency, cfg.n_nodes)
        for i, (summ, msgs) in enumerate(got):
            _same(summ, got.slab[i], ev if i == 2 else eng.raw_journal(i), 600, i, cfg.n_nodes, slots)
            assert int(summ["valid"]) == (0 if i == 2 else 1) and int(summ["orphan_recvs"]) == (1 if i == 2 else 0)


def test_behind_an_asynchronous_launch(lib):
    """straight behind msim_run_async, nothing waited for in between: the analysis is ordered behind the context's stream"""
    cfg = E.test_config(**ACK_RETRY, journal_capacity=100000)
    with E.Engine(cfg) as eng:
        eng.run_async(0, 8)
        got = eng.journal_messages(2000)
        _engine_equals_host(eng, cfg, got, 2000, 0)
        eng.run_async(8, 5)   # the slabs and the workspace again, fewer journals
        got = eng.journal_messages(0)
        assert len(got) == 5
        _engine_equals_host(eng, cfg, got, 0, 0)


def test_the_check_is_untouched(lib):
    """not a check: msim_check's records and its time stay, and a check queued behind the next run is still taken by msim_check"""
    cfg = E.test_config("broadcast", node_count=5, rate=20, time_limit=5, seed=8, journal_capacity=20000)
    with E.Engine(cfg) as eng:
        eng.run(0, 8)
        eng.check()   # (arms the context: the next launch queues its check)
        plain, ms = eng.check_results().tobytes(), eng.kernel_ms()[1]
        got = eng.journal_messages(64)
        assert eng.check_results().tobytes() == plain and eng.kernel_ms()[1] == ms and eng.check_host_rechecks() == 0
        eng.run_async(0, 8)
        again = eng.journal_messages(64)
        eng.check()
        assert eng.check_results().tobytes() == plain
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, again))


def test_refusals(lib):
    L = A.load()
    summ = np.zeros(4, dtype=E.JOURNAL_SUMMARY_DT)
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        eng.run(0, 2)
        assert L.msim_journal_messages(eng._ctx, summ.ctypes.data, None, 0, 2) == A.E_UNSUPPORTED   # journal off
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1, journal_capacity=2000)) as eng:
        assert L.msim_journal_messages(eng._ctx, summ.ctypes.data, None, 0, 2) == A.E_RANGE   # before msim_run
        eng.run(0, 2)
        assert L.msim_journal_messages(eng._ctx, summ.ctypes.data, None, 0, 1) == A.E_RANGE   # arrays shorter than the run
        assert L.msim_journal_messages(eng._ctx, summ.ctypes.data, None, 1, 2) == A.E_INVALID
        assert L.msim_journal_messages(eng._ctx, None, None, 0, 2) == A.E_INVALID
        assert L.msim_journal_messages(eng._ctx, summ.ctypes.data, None, 0, 2) == 0 and int(summ[0]["valid"]) == 1 and int(summ[1]["n_events"]) > 0


def test_the_kernel_keeps_no_private_memory():
    from maelstrom_amd import _abi
    if "libmaelsim_emu" in _abi.LIB_PATH:
        return   # (the host emulator's library has no code objects)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "private_memory_audit.py"), _abi.LIB_PATH], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.split()[0]) > 150
    assert not [ln for ln in r.stdout.splitlines()[1:] if "journal_messages_kernel" in ln], r.stdout
    assert b"journal_messages_kernel" in open(_abi.LIB_PATH, "rb").read()


def test_poisoned_allocations(lib):
    """this module again in a process of its own with every device allocation filled with 0xA5 first (MSIM_POISON is read once per
    process): no table word, record or summary is read before it is written"""
    if os.environ.get("MSIM_POISON"):
        return
    env = dict(os.environ, MSIM_POISON="165")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not poisoned and not private and not chunked"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
