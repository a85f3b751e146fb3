#!/usr/bin/env python3
"""Developer tool (GPU box): the sim kernel's time on the library MSIM_LIB names, for the sweep of the duo kernel's wait cap DUO_PAIR_WAIT
(variants: tools/variant_lib.sh w3 duo.hip -DDUO_PAIR_WAIT=3 ...).  Prints one JSON line per shape: the headline
shape (25 nodes, grid) and the long-flood shape the cap is for (a line of 24 nodes), 4096 instances each, the median of RUNS launches.
    MSIM_LIB=maelstrom_amd/libmaelsim_w3.so python tools/duo_pair_wait_sweep.py w3 >> profiles/r13_pair_wait_sweep.jsonl"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maelstrom_amd import engine as E  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("MSIM_LIB", "product"))
n, runs = int(os.environ.get("N", "4096")), int(os.environ.get("RUNS", "7"))
SHAPES = {"headline grid 25": dict(node_count=25), "line 24": dict(node_count=24, topology="line")}
for name, extra in SHAPES.items():
    cfg = E.test_config(workload="broadcast", bin="broadcast-ff", rate=100, time_limit=20, latency=0, inbox_capacity=6, seed=2026, **extra)
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(0x400)
        ms = []
        for k in range(runs + 1):
            eng.run(k * n, n)
            ms.append(eng.kernel_ms()[0])
        ms = sorted(ms[1:])   # (the first launch warms up)
        eng.fetch()
        flagged = sum(1 for i in range(n) if eng.meta(i).flags != 0)
    print(json.dumps({"lib": tag, "shape": name, "instances": n, "sim_ms_median": round(ms[len(ms) // 2], 4), "sim_ms_min": round(ms[0], 4), "sim_ms_max": round(ms[-1], 4), "flagged": flagged}), flush=True)
