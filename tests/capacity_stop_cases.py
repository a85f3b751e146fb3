"""The cases that take every simulation kernel layout to a capacity stop in a launch where some clusters stop and their
neighbours run on — shared by tests/test_capacity_stops_gpu.py (the device) and, through it, tests/test_capacity_stops_hipemu.py (the host
emulator).

No capacity is written down here.  A case names the capacity it lowers; `capped()` derives the value from an oracle run of the same shape
with the capacities `msim_config_finalize` derives (the "ample" run): the median over the instances of what that run used
(`sorted(x)[n // 2]`), so that about half of the launch stops.  `capped()` asserts on the oracle alone, before any kernel runs, that the
ample run carries no flag and that the lowered run has flagged AND unflagged instances among the clusters that share the first lane group
of the packed layouts (the first eight; the first four for the 16-lane kernels) — a case cannot pass without mixing.

The seeds: 7 wherever it mixes; where it does not, the first seed upwards from 7 (or a launch of up to 19 clusters) whose oracle runs
satisfy both conditions.  Each case was seen, once, to take the kernel it is named for (MSIM_DEV_FLAGS bit 12's [layout] line); the test
asserts the line again on every run."""
import functools

import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import oracle_lib as O
import one_cluster_cases

N = 11   # a full 8-lane group plus a partial one; two full 16-lane wavefronts plus a partial one

# Why a payload stop of the kafka kernels is not the capped oracle's: a round's payload requests (the :invoke maps of the polls, the poll_ok
# blocks, the :assign lists) get their offsets from one prefix sum over the group and are granted all or nothing against
# max_payload_words (kafka8.hip, sim_kernel_kafka.inc), where the oracle's payload_alloc grants them one by one in row order: in the
# overflow round a request that still fits after one that does not is granted by the oracle and refused by the kernels, and the histories
# differ from that row on.  The transactional kernels (txn8, mk8, dt8, hat8 and their one-cluster forms) grant a round's completions the
# same way; on these shapes they equal the capped oracle in full, and their cases assert it.
KAFKA_GRANT = "a round's payload requests are granted all or nothing, the oracle's one by one: rows differ from the overflow round on"

_TXN = dict(workload="txn-list-append", node_count=5, rate=100, time_limit=3, latency=5)

# id, engine.test_config keywords, kernel taken with dev flags 0x400 / with 0x200, clusters per lane group of the packed kernel,
# the capacities to lower, payload_exact (true unless given: a payload stop equals the capped oracle in full; false comes with its reason)
SHAPES = [
    dict(id="uid8", kw=dict(workload="unique-ids", node_count=3, rate=300, time_limit=3, latency=5), kernels=("uid8", "general_a"), caps=("rows",)),
    dict(id="echo", kw=dict(workload="echo", node_count=5, rate=200, time_limit=3, latency=2, p_loss=0.1), kernels=("uid8", "general_a"), caps=("rows",)),
    dict(id="crdt8-gset", kw=dict(workload="g-set", node_count=5, rate=100, time_limit=6, latency=10), kernels=("crdt8", "general_a"), caps=("rows", "payload", "values")),
    dict(id="crdt8-pn", kw=dict(workload="pn-counter", node_count=5, rate=100, time_limit=6, latency=20), kernels=("crdt8", "general_a"), caps=("rows",)),
    dict(id="bcast8", kw=dict(workload="broadcast", bin="broadcast-ack-retry", node_count=5, rate=60, time_limit=4, latency=10, p_loss=0.1), kernels=("bcast8", "general_c"),
         caps=("rows", "payload", "values"), values_kw=dict(p_loss=0.0)),   # (with loss the workers wait out timeouts: fewer values than max_values' granule of 32)
    dict(id="txn8", kw=_TXN, kernels=("txn8", "txn1"), caps=("rows", "payload", "values")),
    dict(id="mk8", kw=dict(_TXN, bin="multi-key-txn", rate=60), kernels=("mk8", "mk1"), caps=("rows", "payload")),
    dict(id="dt8", kw=dict(_TXN, bin="datomic", rate=60), kernels=("dt8", "dt1"), caps=("rows", "payload")),
    dict(id="hat8", kw=dict(workload="txn-rw-register", node_count=2, rate=100, time_limit=3), kernels=("hat8", "hat1"), caps=("rows", "payload")),
    dict(id="kafka8", kw=dict(workload="kafka", node_count=5, rate=80, time_limit=3, latency=5), kernels=("kafka8", "kafka1"), caps=("rows", "payload", "values"),
         payload_exact=False, reason=KAFKA_GRANT),
    dict(id="raft4", kw=dict(workload="lin-kv", bin="raft", node_count=3, rate=50, time_limit=5, latency=5), kernels=("raft4", "raft1"), group=4, caps=("rows",)),
    dict(id="svc4", kw=dict(workload="lin-kv", bin="lin-kv-proxy", proxy_service="lin-kv", node_count=5, concurrency=10, rate=60, time_limit=3, latency=5),
         kernels=("svc4", "svc1"), group=4, caps=("rows",)),
]


def _many(k, **over):
    return dict(one_cluster_cases.KERNELS[k], rate=100, time_limit=4, latency=5, **over)


# several workers per node (a lane per endpoint): four clusters per wavefront where such a kernel exists, else the one-cluster kernel twice
SHAPES += [
    dict(id="txng", kw=_many("txng"), kernels=("txng4", "txng"), group=4, caps=("rows", "payload")),
    dict(id="dtg", kw=_many("dtg"), kernels=("dtg4", "dtg"), group=4, caps=("rows", "payload")),
    dict(id="mkg", kw=_many("mkg"), kernels=("mkg", "mkg"), caps=("rows", "payload")),
    dict(id="hatg", kw=_many("hatg"), kernels=("hatg", "hatg"), caps=("rows", "payload")),
    dict(id="kafkag", kw=_many("kafkag"), kernels=("kafkag", "kafkag"), caps=("rows", "payload"), payload_exact=False, reason=KAFKA_GRANT),
    dict(id="general", kw=_many("general"), kernels=("general_a", "general_a"), caps=("rows",)),
]
# clusters wider than 32 nodes (sim_kernel_wide<>): no packed form, one launch
SHAPES += [
    dict(id="wide", kw=dict(workload="g-set", node_count=40, rate=40, time_limit=6, latency=50, latency_dist="exponential", p_loss=0.05), kernels=(None, "wide_gset"),
         caps=("rows",)),
]
# The values stops (max_values moves in steps of 32, so the median rounded up sits above most of the launch): g-set 320 values, instance 2
# stops; bcast8 128, instance 6; txn8 32 keys, instance 5 — one stopped cluster among seven running ones each time.  kafka8:
# msim_config_finalize fixes max_values, the capacity that runs out is the pool of 8 keys, reached by retiring keys early
# (max_writes_per_key, see capped()): every instance but the first stops, so the launch still mixes.
SHAPE = {s["id"]: s for s in SHAPES}
FIELD = {"rows": "max_rows", "payload": "max_payload_words", "values": "max_values"}
FLAG = {"rows": A.FLAG_ROWS_OVERFLOW, "payload": A.FLAG_PAYLOAD_OVERFLOW, "values": A.FLAG_VALUES_OVERFLOW}

# (shape id, its values shape?) -> (seed, clusters) where seed 7 / 11 clusters do not satisfy the conditions of capped().
# bcast8's values shape: the median of seed 7 (129) rounds up to 160, above every instance; seed 8 stops instances 8 and 9 only; seed 9
# (median 121 -> 128) stops instance 6 among the first eight.
SEEDS = {("bcast8", True): (9, N)}


def seed_of(shape_id, values=False):
    """(seed, clusters); `values`: for the shape's own values keywords (values_kw), where it has some"""
    return SEEDS.get((shape_id, values and "values_kw" in SHAPE[shape_id]), (7, N))


def cases():
    """(id, shape id, capacity, dev flags, expected kernel) for every shape x capacity x layout."""
    out = []
    for s in SHAPES:
        assert s.get("payload_exact", True) or s["reason"]
        for cap in s["caps"]:
            for fl, kernel in zip((0x400, 0x200), s["kernels"]):
                if kernel is not None:
                    out.append((f"{s['id']}-{cap}-{'packed' if fl == 0x400 else 'one'}", s["id"], cap, fl, kernel))
    return out


def workers(cfg):
    return int(cfg.concurrency)


def _values_created(cfg, rows, payload):
    """how many values (broadcast / g-set: elements; txn-list-append: keys) the history's generator handed out"""
    typ, f = rows["packed"] & 3, (rows["packed"] >> 2) & 31
    if cfg.workload in (A.WL_BROADCAST, A.WL_G_SET):
        return int(((typ == A.T_INVOKE) & ((f == A.F_BROADCAST) | (f == A.F_ADD))).sum())
    if cfg.workload == A.WL_TXN_LIST_APPEND:
        top = 0
        for r in rows[(typ == A.T_INVOKE) & (f == A.F_TXN)]:   # an :invoke holds its micro-ops' header words only: key in bits 1-15
            n, off = int(r["time_len"] >> np.uint64(48)), int(r["value"])
            top = max(top, int(((payload[off:off + n] >> 1) & 0x7FFF).max()) + 1)
        return top
    raise ValueError("no values capacity for this workload")


def ample(shape_id, cap="rows"):
    """(config, oracle run) with the capacities msim_config_finalize derives; no instance may carry a flag"""
    if cap != "values" or "values_kw" not in SHAPE[shape_id]:
        return _ample(shape_id, False)
    return _ample(shape_id, True)


def keywords(shape_id, values):
    s = SHAPE[shape_id]
    return dict(s["kw"], **(s.get("values_kw", {}) if values else {}))


@functools.lru_cache(maxsize=None)
def _ample(shape_id, values):
    seed, n = seed_of(shape_id, values)
    cfg = E.test_config(seed=seed, **keywords(shape_id, values))
    ora = O.run(cfg, 0, n)
    assert not ora.meta["flags"].any(), f"{shape_id}: the ample oracle run is flagged: {ora.meta['flags']}"
    return cfg, ora


@functools.lru_cache(maxsize=None)
def capped(shape_id, cap):
    """(config, oracle run, capacity value) with one capacity lowered to the ample run's median use; flagged and unflagged instances share
    the first lane group"""
    seed, n = seed_of(shape_id, cap == "values")
    s = SHAPE[shape_id]
    acfg, aora = ample(shape_id, cap)
    if cap == "values" and s["kw"]["workload"] == "kafka":
        # msim_config_finalize fixes kafka's max_values; what runs out is the pool of 8 keys, a key retired after max_writes_per_key sends.
        # Lowered to an eighth of the median number of sends, so that the ninth key is asked for around the middle of the launch.
        sends = sorted(int((((aora.history(i)[0]["packed"] & 3) == A.T_INVOKE) & (((aora.history(i)[0]["packed"] >> 2) & 31) == A.F_SEND)).sum()) for i in range(n))
        value, over = max(1, sends[n // 2] // 8), dict(max_writes_per_key=max(1, sends[n // 2] // 8))
    elif cap == "values":
        used = sorted(_values_created(acfg, *aora.history(i)) for i in range(n))
        value = (used[n // 2] + 31) // 32 * 32    # as msim_config_finalize rounds max_values
        over = dict(max_values=value)
    else:
        used = sorted(int(x) for x in aora.meta["n_rows" if cap == "rows" else "n_payload_words"])
        value = used[n // 2]
        over = {FIELD[cap]: value}
    cfg = E.test_config(seed=seed, **dict(keywords(shape_id, cap == "values"), **over))
    ora = O.run(cfg, 0, n)
    group = ora.meta["flags"][:s.get("group", 8)]
    flagged = int(((group & FLAG[cap]) != 0).sum())
    if cap == "values":   # (the granularity of 32 may not allow a mix: at least one stop, the case's comment says which it is)
        assert flagged > 0, f"{shape_id}-{cap}: no instance of the first lane group stops at {over}: {ora.meta['flags']}"
    else:
        assert 0 < flagged < len(group) and (group == 0).any(), f"{shape_id}-{cap}: the first lane group does not mix at {over}: {ora.meta['flags']}"
    return cfg, ora, value
