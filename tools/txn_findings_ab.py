"""The non-cycle findings of the transactional checkers (msim_explain_txn_findings_batch; txn_findings_kernel / rw_findings_kernel)
measured against the only route to the same records without them: msim_classify_txn_batch / msim_classify_rw_batch, then
msim_explain_txn_findings_rows for every history whose record carries a non-cycle bit, on `--threads` host threads (a history
without one has the zero header, which the classification's record already says).  One JSON line per set, the lines of
profiles/r49_txn_findings_ab.jsonl.

    python tools/txn_findings_ab.py [--repeats 5] [--scale 1.0] [--threads 16] > lines.jsonl

Both routes run alternating in this one process, after a warm-up call of each: wall time of the calls, uploads included; min / median /
max in milliseconds.  The two routes' headers and slabs are compared byte for byte (a difference ends the run).

Sets, a few thousand histories each: "noiso" — list-append histories of a store without isolation (tools/txn_explain_ab.py's: 256
seeds of tests/test_txn_classify_gpu.no_isolation, each eight times); "faulted" — tests/test_txn_check_synthetic_gpu.py's 104
histories with one fault each, twenty times; "rw5" — the five-node txn-rw-register shape of tools/rw_classify_ab.py (partitions,
read-committed), 2048 histories of a run fetched to the host; "rwfuture" — tests/test_rw_classify_gpu.py's 240 histories with reads
from the future, eight times."""
import argparse
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
NON_CYCLE = 2 | 4 | 64 | 128 | 256 | 1024 | 2048


def _stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 3), "median_ms": round(ms[len(ms) // 2], 3), "max_ms": round(ms[-1], 3), "runs": [round(x, 3) for x in ms]}


def histories(name, scale):
    from maelstrom_amd import engine as E
    if name == "noiso":
        import test_txn_classify_gpu as T
        seeds = max(1, int(256 * scale))
        return [E.encode_txn_history(T.no_isolation(9000 + i, (3, 8, 17)[i % 3], (1, 3, 10)[(i // 3) % 3], 60 + (i * 37) % 140,
                                                    sticky=(0.0, 0.9, 0.99, 0.995)[(i // 9) % 4], p_append=(0.45, 0.12)[(i // 36) % 2])) for i in range(seeds)] * 8
    if name == "faulted":
        import test_txn_classify_gpu as T
        return list(T._faulted_hs()) * max(1, int(20 * scale))
    if name == "rwfuture":
        import test_rw_classify_gpu as RWT
        return list(RWT._random_hs()) * max(1, int(8 * scale))
    n = max(1, int(2048 * scale))
    cfg = E.test_config(seed=99, workload="txn-rw-register", rate=100, time_limit=30, nemesis=["partition"], nemesis_interval=10,
                        consistency_model="read-committed", node_count=5, latency=5)
    with E.Engine(cfg) as eng:
        eng.run(0, n)
        eng.fetch()
        return [tuple(a.copy() for a in eng.raw_history(i)) for i in range(n)]


def measure(name, repeats, scale, threads, max_findings):
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    from maelstrom_amd import engine as E
    rw = name.startswith("rw")
    workload, model = ("txn-rw-register", "read-committed") if rw else ("txn-list-append", "strict-serializable")
    hs = histories(name, scale)
    n = len(hs)

    def device():
        t0 = time.perf_counter()
        out, hdr, fs, handed = E.explain_txn_findings_batch(hs, workload, model, max_findings=max_findings, with_n_host=True)
        return (time.perf_counter() - t0) * 1e3, out, hdr, fs.slab, handed

    def host():
        t0 = time.perf_counter()
        out, handed = (E.classify_rw_batch if rw else E.classify_txn_batch)(hs, model)
        t1 = time.perf_counter()
        todo = [i for i in range(n) if int(out[i]["error_count"]) & NON_CYCLE]
        hdr = np.zeros(n, dtype=E.TXN_EXPLAIN_DT)
        slab = np.zeros((n, max_findings), dtype=E.TXN_FINDING_DT)

        def explain(i):
            _, h, recs = E.explain_txn_findings_history(hs[i][0], hs[i][1], workload, model, max_findings)
            hdr[i] = h
            slab[i, :len(recs)] = recs
        with ThreadPoolExecutor(threads) as ex:      # (the entry runs outside the interpreter lock)
            list(ex.map(explain, todo))
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, out, hdr, slab, handed, (t1 - t0) * 1e3, len(todo)

    device(); host()                                 # warm: the library loaded, the device awake, the allocator's pools filled
    dev_ms, host_ms, classify_ms = [], [], []
    for _ in range(repeats):
        d = device()
        h = host()
        dev_ms.append(d[0]); host_ms.append(h[0]); classify_ms.append(h[5])
        if d[1].tobytes() != h[1].tobytes() or d[2].tobytes() != h[2].tobytes() or d[3].tobytes() != h[3].tobytes():
            sys.exit(f"{name}: the two routes' records differ")
    hdr = d[2]
    print(json.dumps({"set": name, "workload": workload, "model": model, "n": n, "max_findings": max_findings, "threads": threads,
                      "rows_mean": float(np.mean([len(r) for r, _ in hs])), "with_findings": h[6], "findings": int(hdr["count"].sum()),
                      "findings_per_anomaly": {name_: int(hdr["count"][:, bit.bit_length() - 1].sum()) for bit, name_ in E.A.ANOMALIES.items() if bit & NON_CYCLE},
                      "device_n_host": d[4], "classify_n_host": h[4],
                      "device": _stats(dev_ms), "classify_then_host": _stats(host_ms), "of_which_classify": _stats(classify_ms),
                      "records_sha": hashlib.sha256(d[2].tobytes() + d[3].tobytes()).hexdigest()[:16]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each set's histories (a quick look)")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the host route's explanations")
    ap.add_argument("--max-findings", type=int, default=64)
    ap.add_argument("--sets", default="noiso,faulted,rw5,rwfuture")
    a = ap.parse_args()
    for name in a.sets.split(","):
        measure(name, a.repeats, a.scale, a.threads, a.max_findings)


if __name__ == "__main__":
    main()
