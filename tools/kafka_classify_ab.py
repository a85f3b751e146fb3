"""Unclean kafka histories through the two routes of the device check, side by side in one process: E.check_kafka_batch (the device
proves the clean ones clean, the host checker classifies the others: one copy across PCIe and one check_kafka per history) and
E.classify_kafka_batch (kafka_classify_kernel names the anomalies on the device).  One JSON line, the line of
profiles/<round>_kafka_classify_ab.jsonl.

    python tools/kafka_classify_ab.py --round r34 [--copies 56] [--repeats 5] [--out lines.jsonl]

The histories are the 72 corrupted oracle histories of tests/kafka_classify_cases.py (1 - 3 mutations each of a 3-node run), `--copies`
times over (56: 4032 histories).  Each route is warmed up once and then timed `--repeats` times, alternating; the time is the whole
call (the copies of the rows to the device included, which both routes make).  The records of the two routes must be identical; the
line carries their hash, the histories each route gave to the host, and the anomaly census."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--round", default="dev", help="the label in the file name under profiles/")
    ap.add_argument("--copies", type=int, default=56)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", help="append the line here instead of profiles/<round>_kafka_classify_ab.jsonl")
    a = ap.parse_args()
    import numpy as np
    from maelstrom_amd import engine as E
    import kafka_classify_cases as K
    family = list(K.corrupted_family())
    hs = family * a.copies
    routes = {"check": E.check_kafka_batch, "classify": E.classify_kafka_batch}
    ms = {name: [] for name in routes}
    last = {}
    for rep in range(a.repeats + 1):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            last[name] = fn(hs, 3)
            if rep:                                # (the first round loads the code and warms the allocator)
                ms[name].append((time.perf_counter() - t0) * 1e3)
    (rec_a, host_a), (rec_b, host_b) = last["check"], last["classify"]
    same = rec_a.tobytes() == rec_b.tobytes()
    out = {"tool": "kafka_classify_ab", "round": a.round, "histories": len(hs), "family": len(family), "rows_mean": float(np.mean([len(r) for r, _ in family])),
           "unclean": int((rec_b["error_count"] != 0).sum()), "check_ms": ms["check"], "classify_ms": ms["classify"],
           "check_ms_median": float(np.median(ms["check"])), "classify_ms_median": float(np.median(ms["classify"])),
           "check_n_host": int(host_a), "classify_n_host": int(host_b), "records_identical": same,
           "records_sha": hashlib.sha256(rec_b.tobytes()).hexdigest()[:16], "census": E.kafka_anomaly_census(rec_b)}
    line = json.dumps(out)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, "profiles", f"{a.round}_kafka_classify_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")
    if not same:
        sys.exit("the two routes' records differ")


if __name__ == "__main__":
    main()
