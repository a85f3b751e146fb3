"""Unclean kafka histories explained by two routes, side by side in one process: E.explain_kafka_batch (kafka_explain_kernel writes the
findings on the device) and the route a caller had without that kernel — E.classify_kafka_batch for the records, then the host entry
(msim_explain_kafka_rows, through E.explain_kafka_history) on every history whose record names an anomaly, on the granted host
threads.  One JSON line, the line of profiles/<round>_kafka_explain_ab.jsonl.

    python tools/kafka_explain_ab.py --round r43 [--copies 56] [--repeats 5] [--max-findings 64] [--threads N] [--out lines.jsonl]

The histories are those of tools/kafka_classify_ab.py: the 72 corrupted oracle histories of tests/kafka_classify_cases.py, `--copies`
times over (56: 4032 histories).  Each route is warmed up once and then timed `--repeats` times, alternating; the time is the whole
call (the copies of the rows to the device included, which both routes make).  `--threads` defaults to MSIM_HOST_THREADS, then
OMP_NUM_THREADS, then the CPUs this process may run on.  Records, headers and findings of the two routes must be identical; the line
carries their hash and the findings per anomaly."""
import argparse
import concurrent.futures as cf
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
    ap.add_argument("--max-findings", type=int, default=64)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("MSIM_HOST_THREADS") or os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))))
    ap.add_argument("--out", help="append the line here instead of profiles/<round>_kafka_explain_ab.jsonl")
    a = ap.parse_args()
    import numpy as np
    from maelstrom_amd import _abi as A
    from maelstrom_amd import engine as E
    import kafka_classify_cases as K
    family = list(K.corrupted_family())
    hs = family * a.copies
    cap = a.max_findings
    pool = cf.ThreadPoolExecutor(max_workers=a.threads)   # (the entry runs outside the interpreter's lock)

    def device():
        out, hdr, fs, n_host = E.explain_kafka_batch(hs, 3, max_findings=cap)
        return out, hdr, fs.slab, n_host

    def host():
        out, n_host = E.classify_kafka_batch(hs, 3)
        hdr = np.zeros(len(hs), dtype=E.KAFKA_EXPLAIN_DT)
        slab = np.zeros((len(hs), max(cap, 1)), dtype=E.KAFKA_FINDING_DT)

        def one(i):
            _, hdr[i], found = E.explain_kafka_history(*hs[i], max_findings=cap)
            slab[i, :len(found)] = found

        list(pool.map(one, [i for i in range(len(hs)) if out[i]["error_count"]]))
        return out, hdr, slab[:, :cap], n_host

    routes = {"device": device, "host": host}
    ms = {name: [] for name in routes}
    last = {}
    for rep in range(a.repeats + 1):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            last[name] = fn()
            if rep:                                # (the first round loads the code and warms the allocator)
                ms[name].append((time.perf_counter() - t0) * 1e3)
    dev, ref = last["device"], last["host"]
    same = all(x.tobytes() == y.tobytes() for x, y in zip(dev[:3], ref[:3]))
    count = dev[1]["count"].sum(axis=0)
    out = {"tool": "kafka_explain_ab", "round": a.round, "histories": len(hs), "family": len(family), "rows_mean": float(np.mean([len(r) for r, _ in family])),
           "unclean": int((dev[0]["error_count"] != 0).sum()), "max_findings": cap, "host_threads": a.threads,
           "device_ms": ms["device"], "host_ms": ms["host"], "device_ms_median": float(np.median(ms["device"])), "host_ms_median": float(np.median(ms["host"])),
           "device_n_host": int(dev[3]), "host_n_host": int(ref[3]), "identical": same, "truncated": int(dev[1]["truncated"].sum()),
           "sha": hashlib.sha256(b"".join(x.tobytes() for x in dev[:3])).hexdigest()[:16],
           "findings": {name: int(count[b.bit_length() - 1]) for b, name in A.KAFKA_ANOMALIES.items()}}
    line = json.dumps(out)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, "profiles", f"{a.round}_kafka_explain_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")
    if not same:
        sys.exit("the two routes' records, headers or findings differ")


if __name__ == "__main__":
    main()
