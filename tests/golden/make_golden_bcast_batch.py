#!/usr/bin/env python3
"""Records tests/golden/bcast_batch_digests.json: digests (tests/bcast_batch_ref.py digest: normalised history, net stats, round count,
journal events where recorded) of the batched-gossip model (the reference's demo/python/broadcast.py as a state machine on the process
bridge's scheduler) for
  * "pinned": the shapes tests/test_bcast_batch_replay.py runs, journal on;
  * "bench": the last instances of a 4096-cluster launch at cfg2's shape (tools/bench_configs.py rows "broadcast-batch n=25 grid lat0 /
    lat100", seed 99), which tests/test_bcast_batch_gpu.py holds the device's slabs to.

    MAELSTROM_REFERENCE=<reference tree> python tests/golden/make_golden_bcast_batch.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bcast_batch_ref as M  # noqa: E402
import bcast_batch_replay as R  # noqa: E402

PINNED = [
    dict(node_count=5, rate=30, time_limit=10, latency=30, latency_dist="exponential", p_loss=0.1, seed=31),
    dict(node_count=9, rate=20, time_limit=8, latency=20, nemesis=["partition"], nemesis_interval=2, seed=32),
    dict(node_count=6, rate=20, time_limit=5, latency=50, topology="line", seed=33),
]
BENCH = [dict(node_count=25, rate=100, time_limit=20), dict(node_count=25, rate=100, time_limit=20, latency=100)]
BENCH_INSTANCES = [4094, 4095]


def main():
    out = {"pinned": [], "bench": []}
    for kw in PINNED:
        digests = []
        for i in range(2):
            b, nodes, st = R.replay(kw, instance=i)   # raises unless the real program printed what the model emitted
            print("pinned", kw, i, st, flush=True)
            digests.append(M.model_digest(b, nodes))
        out["pinned"].append({"kw": kw, "instances": [0, 1], "digests": digests})
    for kw in BENCH:
        digests = []
        for i in BENCH_INSTANCES:
            b, nodes = M.run_model(journal=False, instance=i, seed=99, **kw)
            assert not b.errors, b.errors
            digests.append(M.model_digest(b, nodes))
        out["bench"].append({"kw": kw, "seed": 99, "instances": BENCH_INSTANCES, "digests": digests})
    with open(os.path.join(HERE, "bcast_batch_digests.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
