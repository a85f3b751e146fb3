"""What tests/test_pipeline_gpu.py (on the device, and through tests/test_pipeline_hipemu.py on the host wavefront emulator) shares: the
configurations of the pipelined launch path, the oracle of a batch (computed once per (configuration, first, n), on a thread pool, and
left unchanged), the comparison of a fetched batch with it, one helper that reads device memory, and the benchmark's step / retire / drain
loop.  TEST INFRASTRUCTURE ONLY.

The emulator is synchronous: it holds the state machine of the path (fetched / fetch_pending / checked, the pinned mirrors that are
regrown, the compaction kernels) on a machine without a GPU; the ordering itself — a check or a copy that runs ahead of its simulation,
launches in flight that disturb each other — is the device run's job.  Every comparison is exact."""
import concurrent.futures as cf
import ctypes as C
import math
import os
import re
import time

import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
from launch_digests import digest_engine, digest_oracle
import oracle_lib as O
from test_large_launch_gpu import _records

EMU = "_emu" in os.path.basename(A.LIB_PATH)
if not EMU:
    import torch   # before the engine's library is loaded, as in bench.py: the process then holds one HIP runtime, torch's
TRACE = 0x1000
SEED = 99
# Batches of a pipeline's steps; an odd size gives the two-clusters-per-wavefront kernel a half-filled last wavefront.  On the device
# 192 / 256 / 131.  The reference of the headline shape's records is the Python restatement of set-full (tests/setfull_ref.py behind
# engine.decode_history), 7 to 18 ms per history of that shape on one host core (some 300 elements, decoded from about 175 reads):
# seven steps of that size would spend 9 to 23 s there, so the headline's batches are half as large — its shape, the seven steps and the
# depth are not, and every record is still held against its reference.
_SIZES = {"headline": (96, 128, 67)}


def sizes(name):
    return (4, 6, 3) if EMU else _SIZES.get(name, (192, 256, 131))


def headline(seed=SEED):
    """bench.headline_config with the simulated time shortened (3 s; the emulator at half the rate): every other option is read from
    the benchmark's own configuration."""
    import bench
    full = bench.headline_config(E, seed)
    assert (full.workload, full.node_program, full.latency_dist, full.topology) == (A.WL_BROADCAST, A.NODE_BCAST_FF, A.LAT_CONSTANT, A.TOPO_GRID)
    return E.test_config("broadcast", bin="broadcast-ff", node_count=full.n_nodes, rate=50 if EMU else full.rate_mhz / 1000, time_limit=3,
                         latency=full.latency_mean_ms, latency_dist="constant", topology="grid", seed=seed, inbox_capacity=full.inbox_capacity)


def _t(emu, gpu):
    return emu if EMU else gpu


# name: (configuration, the kernel its launches take at these batch sizes)
CONFIGS = {
    "headline": (headline, "duo"),
    "bcast25-exp": (lambda: E.test_config("broadcast", node_count=25, rate=_t(20, 50), time_limit=_t(2, 3), latency=100, latency_dist="exponential", seed=SEED), "duo"),
    "ack25-partitions": (lambda: E.test_config("broadcast", bin="broadcast-ack-retry", node_count=25, rate=_t(10, 20), time_limit=_t(3, 5), latency=10,
                                               nemesis=["partition"], nemesis_interval=_t(1, 2), seed=SEED), "general_c"),
    "raft-partitions": (lambda: E.test_config("lin-kv", bin="raft", node_count=5, rate=30, time_limit=_t(4, 8), latency=10, nemesis=["partition"],
                                              nemesis_interval=2, seed=SEED), "raft4"),
    "txn-partitions": (lambda: E.test_config("txn-list-append", node_count=5, rate=_t(60, 100), time_limit=_t(3, 5), latency=5, nemesis=["partition"],
                                             nemesis_interval=2, seed=SEED), "txn8"),
    "gset100": (lambda: E.test_config("g-set", node_count=100, rate=_t(20, 50), time_limit=_t(2, 3), latency=100, latency_dist="exponential", seed=SEED), "wide_gset"),
    "kafka5": (lambda: E.test_config("kafka", node_count=5, rate=_t(60, 100), time_limit=_t(3, 5), latency=5, seed=SEED), "kafka1"),
}
_CFG = {}


def config(name):
    if name not in _CFG:
        _CFG[name] = CONFIGS[name][0]()
    return _CFG[name]


# ---- the oracle of a batch ------------------------------------------------------------------------------------------------------------
class Batch:
    """Oracle outputs of instances first .. first + n - 1, by launch-relative index."""

    def __init__(self, cfg, first, n, runs):
        self.cfg, self.first, self.n = cfg, first, n
        self._at = {}
        for s, ora in runs:
            for k in range(ora.n):
                self._at[s + k] = (ora, k)
        self._digests = {}

    def digest(self, i):
        if i not in self._digests:
            ora, k = self._at[i]
            self._digests[i] = digest_oracle(ora, k)
        return self._digests[i]

    def history(self, i):
        ora, k = self._at[i]
        return ora.history(k)

    def meta(self, i):
        ora, k = self._at[i]
        return ora.meta[k]

    def stats(self, i):
        ora, k = self._at[i]
        return ora.stats[k]

    def events(self, i):
        ora, k = self._at[i]
        return ora.events(k)


_ORACLE = {}


def oracle(cfg, first, n):
    """The oracle's batch (first, n) of cfg, in chunks over a thread pool (the oracle is C, the GIL is released during the call); computed
    once per (cfg, first, n)."""
    key = (bytes(cfg), first, n)
    if key not in _ORACLE:
        chunk = max(1, min(8, -(-n // 16)))
        groups = [(s, min(chunk, n - s)) for s in range(0, n, chunk)]
        with cf.ThreadPoolExecutor(max_workers=8) as ex:
            runs = list(ex.map(lambda g: (g[0], O.run(cfg, first + g[0], g[1])), groups))
        _ORACLE[key] = Batch(cfg, first, n, runs)
    return _ORACLE[key]


def compare_batch(eng, cfg, first, n, what, journal=False):
    """The fetched batch of `eng` — rows, payload, net stats, counts, flags, rounds of every instance (and its journal) — against the oracle
    of (first, n).  Returns the oracle's batch."""
    assert eng.n == n, what
    ref = oracle(cfg, first, n)
    bad = [i for i in range(n) if digest_engine(eng, i) != ref.digest(i)]
    assert not bad, f"{what}: {len(bad)} of {n} instances differ from the oracle, launch-relative: {bad[:8]} (first_instance {first})"
    if journal:
        bad = [i for i in range(n) if eng.raw_journal(i).tobytes() != ref.events(i).tobytes()]
        assert not bad, f"{what}: the journals of {len(bad)} of {n} instances differ from the oracle's: {bad[:8]} (first_instance {first})"
    return ref


def compare_records(eng, cfg, res, what):
    """Every record of the fetched batch against the host checker / the Python restatements (test_large_launch_gpu._records)."""
    assert len(res) == eng.n, what
    _records(eng, cfg, res, list(range(eng.n)))


# ---- device memory ---------------------------------------------------------------------------------------------------------------------
def device_bytes(ptr, nbytes):
    """nbytes of the engine's device memory at ptr as a numpy u8 array (a copy): a torch view through __cuda_array_interface__ on the
    device, as bench.py takes it; the emulator's device memory is host memory."""
    if EMU:
        return np.frombuffer(C.string_at(ptr, int(nbytes)), dtype=np.uint8).copy()
    return _torch_view(ptr, nbytes).cpu().numpy()


def _torch_view(ptr, nbytes):
    class _W:
        pass
    w = _W()
    w.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(w, device=torch.device("cuda", 0))


def bench_sums(eng):
    """The five sums bench.py's retire() adds up from its views of device_buffers(): messages sent, valid histories, flagged instances,
    rows, payload words."""
    db = eng.device_buffers()
    if EMU:
        stats = device_bytes(db.stats, db.stats_bytes).view(np.int64).reshape(-1, 6)
        meta = device_bytes(db.meta, db.meta_bytes).view(np.int32).reshape(-1, 8)
        chk = device_bytes(db.check, db.check_bytes).view(np.int32).reshape(-1, 17)
        return [int(stats[:, 0].sum()), int((chk[:, 0] == 1).sum()), int((meta[:, 2] != 0).sum()), int(meta[:, 0].sum(dtype=np.int64)), int(meta[:, 1].sum(dtype=np.int64))]
    stats = _torch_view(db.stats, db.stats_bytes).view(torch.int64).view(-1, 6)
    meta = _torch_view(db.meta, db.meta_bytes).view(torch.int32).view(-1, 8)
    chk = _torch_view(db.check, db.check_bytes).view(torch.int32).view(-1, 17)
    return [int(x) for x in torch.stack([stats[:, 0].sum(), (chk[:, 0] == 1).sum(), (meta[:, 2] != 0).sum(),
                                         meta[:, 0].sum(dtype=torch.int64), meta[:, 1].sum(dtype=torch.int64)]).cpu()]


# ---- launches ---------------------------------------------------------------------------------------------------------------------------
def layout(capfd):
    return re.findall(r"^\[layout\] (\S+) (\d+)$", capfd.readouterr().err, re.M)


def launch_async(eng, capfd, first, n, kernel, stream=None):
    """run_async with the kernel it took read from its `[layout]` line (developer flag bit 12, set around the launch only: the same bit
    makes the checkers time their passes)."""
    capfd.readouterr()
    eng.set_dev_flags(TRACE)
    try:
        eng.run_async(first, n, stream)
    finally:
        eng.set_dev_flags(0)
    got = layout(capfd)
    assert got == [(kernel, str(n))], (kernel, n, got)


def finite_ms(eng, what):
    sim, chk = eng.kernel_ms()
    assert math.isfinite(sim) and sim > 0, f"{what}: kernel_ms {sim} after an asynchronous launch"
    assert math.isfinite(chk) and chk >= 0, f"{what}: check_ms {chk}"
    return sim, chk


class Pipeline:
    """bench.py's timed loop: `depth` engine contexts, each with its own stream; step k launches on context k % depth after retiring what
    that context still holds; drain retires the rest in step order.  Retiring checks straight after the asynchronous launch, with no
    synchronisation in between, and holds everything the context then has against the oracle and the reference checkers."""

    def __init__(self, names, capfd):
        self.names, self.capfd = list(names), capfd
        self.depth = len(self.names)
        self.pending = [None] * self.depth
        self.acc, self.want = [0] * 5, [0] * 5
        self.ms, self.retired = [], []

    def batch(self, k):
        """distinct instances for every step; the sizes shift by one every round, so that a context's batch grows and shrinks"""
        return 1000 * k + 7, sizes(self.names[k % self.depth])[(k + k // self.depth) % 3]

    def retire(self, j):
        k = self.pending[j]
        e, name = self.engs[j], self.names[j]
        cfg = config(name)
        first, n = self.batch(k)
        what = f"step {k} ({name}, context {j}, first {first}, n {n})"
        e.check()                      # straight after run_async: nothing else waits for the simulation
        sums = bench_sums(e)           # (what bench.py reads here)
        res = e.check_results()
        sim, chk = finite_ms(e, what)
        e.fetch()
        ref = compare_batch(e, cfg, first, n, what)
        compare_records(e, cfg, res, what)
        # the benchmark's bookkeeping from the oracle and the records just held against the reference checkers
        want = [sum(int(ref.stats(i)["all_send"]) for i in range(n)), int((res["valid"] == 1).sum()), sum(int(ref.meta(i)["flags"]) != 0 for i in range(n)),
                sum(int(ref.meta(i)["n_rows"]) for i in range(n)), sum(int(ref.meta(i)["n_payload_words"]) for i in range(n))]
        assert sums == want, f"{what}: the sums of the device views {sums} are not the oracle's / the reference checker's {want}"
        self.acc = [a + b for a, b in zip(self.acc, sums)]
        self.want = [a + b for a, b in zip(self.want, want)]
        self.ms.append((k, n, sim, chk))
        self.retired.append(k)
        self.pending[j] = None

    def step(self, k):
        j = k % self.depth
        if self.pending[j] is not None:
            self.retire(j)
        first, n = self.batch(k)
        launch_async(self.engs[j], self.capfd, first, n, CONFIGS[self.names[j]][1])
        self.pending[j] = k

    def drain(self):
        for k, j in sorted((k, j) for j, k in enumerate(self.pending) if k is not None):
            self.retire(j)

    def run(self, steps):
        t0 = time.perf_counter()
        for name in set(self.names):   # (the oracle first, so that the launches follow each other as closely as the benchmark's)
            for k in range(steps):
                if self.names[k % self.depth] == name:
                    oracle(config(name), *self.batch(k))
        t1 = time.perf_counter()
        self.engs = [E.Engine(config(name)) for name in self.names]
        try:
            for k in range(steps):
                self.step(k)
            self.drain()
        finally:
            for e in self.engs:
                e.close()
        assert self.retired == list(range(steps))
        self.oracle_s, self.wall_s = t1 - t0, time.perf_counter() - t0
        return self

    def line(self, title):
        per = ", ".join(f"{k}:{n}x{sim:.2f}+{chk:.2f}" for k, n, sim, chk in self.ms)
        return (f"[pipeline] {title}: depth {self.depth}, {len(self.ms)} steps, step:n x kernel_ms sim+check {per}; wall {self.wall_s:.1f} s "
                f"(oracle {self.oracle_s:.1f} s)")
