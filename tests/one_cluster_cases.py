"""The cases that take every one-cluster-per-wavefront kernel sharing csrc/group64_*.inc through all four of its <NEM, NET_RANDOM>
instantiations — shared by tests/test_parity_gpu.py (the device) and tests/test_hipemu_parity.py (the host emulator).

Two clusters: below every threshold of csrc/layout_thresholds.h.  raft4, txn8 and mk8 have no launch-size floor — with the journal off
they take a three-node cluster at any launch size — so the raft, txn and mk cases carry MSIM_DEV_FLAGS bit 9 (DEV_FLAGS), which keeps the
one-cluster kernels; the others run with no flag.  Every case was seen, once, to take the kernel it is named for (bit 12's [layout]
line: general_a twice, raft1, svc1, txn1, txng, mk1, mkg, dt1, dtg, hat1, hatg, kafka1, kafkag).  Three nodes; the kernels with a lane
per endpoint get two nodes with three workers each (unequal numbers of node and client lanes).  Four simulated seconds."""

SEED = 7   # (tools/emu_compare.py's default): every case ends without an overflow flag and with rows, checked on the oracle
CLUSTERS = 2

# kernels that a packed layout would otherwise take at this size: MSIM_DEV_FLAGS bit 9 keeps the one-cluster kernel
DEV_FLAGS = {"raft": 0x200, "txn": 0x200, "mk": 0x200}

# kernel -> engine.test_config keywords that select it
KERNELS = {
    "general": dict(workload="echo", node_count=3, concurrency=6),          # concurrency != node count: a lane per endpoint
    "colo": dict(workload="g-set", node_count=3),                           # node i and its client on lane i
    "raft": dict(workload="lin-kv", bin="raft", node_count=3),
    "svc": dict(workload="lin-kv", bin="lin-kv-proxy", proxy_service="seq-kv", node_count=3),
    "txn": dict(workload="txn-list-append", node_count=3),
    "txng": dict(workload="txn-list-append", node_count=2, concurrency=6),
    "mk": dict(workload="txn-list-append", bin="multi-key-txn", node_count=3),
    "mkg": dict(workload="txn-list-append", bin="multi-key-txn", node_count=2, concurrency=6),
    "dt": dict(workload="txn-list-append", bin="datomic", node_count=3),
    "dtg": dict(workload="txn-list-append", bin="datomic", node_count=2, concurrency=6),
    "hat": dict(workload="txn-rw-register", node_count=3),
    "hatg": dict(workload="txn-rw-register", node_count=2, concurrency=6),
    "kafka": dict(workload="kafka", node_count=3),
    "kafkag": dict(workload="kafka", node_count=2, concurrency=6),
}

# <NEM, NET_RANDOM>.  An interval of one second gives several start / stop pairs in four, the grudge drawn per start.  With both on the
# journal is kept too (the events carry jwrite's and arrive's fields) and an endpoint's queue has two LDS slots, so that pushes spill
# and recv! scans the spill area.  Observed on the emulator (a print in lds_push, not kept), seed 7: the spill area is used by raft, svc,
# txng, mk, mkg, hat, hatg, kafka and kafkag (one to three entries deep); txn, dt and dtg never have three envelopes waiting at one endpoint
# at this size with any of the seeds 1..24 (three nodes with one transaction each, or the node's lock), nor can echo's nodes: their
# spills are test_txn_list_append_deep_service_queue_parity's, test_datomic_txn_parity's and test_deep_queues_spill_to_hbm's.
VARIANTS = {
    "plain": dict(latency=5),
    "random": dict(latency=20, latency_dist="exponential", p_loss=0.05),
    "nemesis": dict(latency=5, nemesis=["partition"], nemesis_interval=1),
    "nemesis-random-journal-spill": dict(latency=20, latency_dist="exponential", p_loss=0.05, nemesis=["partition"], nemesis_interval=1,
                                         journal_capacity=8192, inbox_capacity=2),
}


def cases():
    """(id, engine.test_config keywords, dev flags) for every kernel x variant."""
    return [(f"{k}-{v}", dict(KERNELS[k], rate=100, time_limit=4, **VARIANTS[v]), DEV_FLAGS.get(k, 0)) for k in KERNELS for v in VARIANTS]
