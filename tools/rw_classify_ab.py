"""The txn-rw-register check (csrc/rw_check_dev.hip) of two builds of libmaelsim side by side: one JSON line per (library, shape, model,
classify), the lines of profiles/r23_rw_classify_ab.jsonl and profiles/r29_rw_large_components.jsonl.

    python tools/rw_classify_ab.py parent=/path/to/parent/libmaelsim.so new=maelstrom_amd/libmaelsim.so [--repeats 5] [--scale 1.0] > lines.jsonl

Every line is measured in a process of its own that loads its library through MSIM_LIB: a warm-up run + check, then `--repeats` runs +
checks of fresh seeds (the same seeds for every library).  check_ms is msim_check as the engine times it; verdict_sha / records_sha are
over the verdicts / the whole records of the last repeat, so that two libraries can be compared byte for byte; host_rechecks is the
host's share of that check; the census and the transactions in cycles come from its records.  With MSIM_DEV_FLAGS bit 12 (0x1000) in the
environment the children print the check's `[rw-check]` trace lines (time per pass) on stderr.  A child that fails ends the run.

Shapes: the two serializable configurations and the classify configuration of tools/bench_configs.py, the same two under
read-committed (the first pass alone), and a classify line for n=5."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {2: (dict(node_count=2), 16384), 5: (dict(node_count=5, latency=5), 4096)}
LINES = [(2, "serializable", False), (2, "read-committed", False), (2, "read-committed", True),
         (5, "serializable", False), (5, "read-committed", False), (5, "read-committed", True)]


def one(label, nodes, model, classify, repeats, scale):
    import numpy as np
    from maelstrom_amd import engine as E
    kw, n = SHAPES[nodes]
    n = max(1, int(n * scale))
    cfg = E.test_config(seed=99, workload="txn-rw-register", rate=100, time_limit=30, nemesis=["partition"], nemesis_interval=10, consistency_model=model, **kw)
    sim, chk = [], []
    with E.Engine(cfg) as eng:
        eng.run(0, n)
        eng.check(classify=classify)
        for r in range(repeats):
            eng.run((r + 1) * n, n)
            eng.check(classify=classify)
            s, c = eng.kernel_ms()
            sim.append(s); chk.append(c)
        res = eng.check_results()
        host = eng.check_host_rechecks()
    out = {"lib": label, "nodes": nodes, "n": n, "model": model, "classify": classify, "sim_ms": sim, "check_ms": chk,
           "check_ms_median": float(np.median(chk)), "check_ms_spread": float(max(chk) - min(chk)), "host_rechecks": host,
           "invalid": int((res["valid"] == 0).sum()),
           "verdict_sha": hashlib.sha256(np.ascontiguousarray(res["valid"]).tobytes()).hexdigest()[:16],
           "records_sha": hashlib.sha256(res.tobytes()).hexdigest()[:16],
           "census": E.anomaly_census(res), "cycle_txns_max": int(res["stale_count"].max()), "cycle_txns_mean": float(res["stale_count"].mean()),
           "txns_mean": float(res["attempt_count"].mean()), "edges_mean": float(res["lost_count"].mean())}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs="*", help="label=path of a libmaelsim.so")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each shape's histories (a quick look)")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds a line's process may take")
    ap.add_argument("--one", nargs=4, metavar=("LABEL", "NODES", "MODEL", "CLASSIFY"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], int(a.one[1]), a.one[2], a.one[3] == "1", a.repeats, a.scale)
    if not a.libs:
        ap.error("name at least one library: label=path")
    libs = [x.split("=", 1) for x in a.libs]
    for nodes, model, classify in LINES:
        for label, path in libs:
            env = dict(os.environ, MSIM_LIB=os.path.abspath(path))
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--scale", str(a.scale),
                   "--one", label, str(nodes), model, "1" if classify else "0"]
            r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=a.timeout)
            if r.returncode != 0:
                sys.exit(f"{label} n={nodes} {model} classify={classify}: exit status {r.returncode}")


if __name__ == "__main__":
    main()
