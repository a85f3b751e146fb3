"""The lin-kv check of one ensemble, plain and explaining, side by side in one process: Engine.check() (msim_check), Engine.explain_lin_kv()
(msim_explain_lin_kv: the explaining kernels of csrc/lin_check_dev.hip write a record per key) and the same records from the host search
on all host threads (developer switch 0x800, after the histories were fetched).  One JSON line, the line of
profiles/<round>_lin_explain_ab.jsonl.

    python tools/lin_explain_ab.py --round r36 [--instances 8192] [--repeats 5] [--max-keys 64] [--plain-only] [--label this] [--out lines.jsonl]

The ensemble is BASELINE configs[3] with partitions (lin-kv over Raft, 5 nodes, rate 30, 60 s, latency 10, a partition every 10 s).  Each
route is warmed up once and then timed `--repeats` times, alternating; a time is the whole call.  --plain-only times Engine.check() alone
and uses nothing this tool's commit added, so the same file runs against a checkout of the parent commit (--label parent): that pair of
lines, taken alternately, is the "plain check unchanged" measurement."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--round", default="dev", help="the label in the file name under profiles/")
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-keys", type=int, default=64)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library to load")
    ap.add_argument("--out", help="append the line here instead of profiles/<round>_lin_explain_ab.jsonl")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    from maelstrom_amd import engine as E
    cfg = E.test_config("lin-kv", bin="raft", node_count=5, rate=30, time_limit=60, latency=10, nemesis=["partition"], nemesis_interval=10)
    n = a.instances
    out = {"tool": "lin_explain_ab", "round": a.round, "label": a.label, "histories": n, "config": "cfg4 lin-kv raft + partitions lat10"}
    ms = {"check": [], "explain": []}
    with E.Engine(cfg) as eng:
        eng.run(0, n)
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            eng.check()
            if rep:                                # (the first round loads the code and warms the allocator)
                ms["check"].append((time.perf_counter() - t0) * 1e3)
            if a.plain_only:
                continue
            t0 = time.perf_counter()
            res = eng.explain_lin_kv(max_keys=a.max_keys)
            if rep:
                ms["explain"].append((time.perf_counter() - t0) * 1e3)
        plain = eng.check_results()
        out.update(check_ms=ms["check"], check_ms_median=float(np.median(ms["check"])), check_n_host=eng.check_host_rechecks(),
                   invalid=int((plain["valid"] == 0).sum()), check_sha=hashlib.sha256(plain.tobytes()).hexdigest()[:16])
        if not a.plain_only:
            n_host = eng.check_host_rechecks()
            t0 = time.perf_counter()
            eng.fetch()
            fetch_ms = (time.perf_counter() - t0) * 1e3
            eng.set_dev_flags(0x800)               # the checkers on the host cores: the same entry, the host search on all host threads
            host_ms = []
            for rep in range(2):
                t0 = time.perf_counter()
                host = eng.explain_lin_kv(max_keys=a.max_keys)
                host_ms.append((time.perf_counter() - t0) * 1e3)
            eng.set_dev_flags(0)
            same = all(dk.tobytes() == hk.tobytes() and int(dr["valid"]) == int(hr["valid"]) for (dr, dk), (hr, hk) in zip(res, host))
            keys = np.concatenate([k for _, k in res])
            out.update(max_keys=a.max_keys, explain_ms=ms["explain"], explain_ms_median=float(np.median(ms["explain"])), explain_n_host=n_host,
                       fetch_ms=fetch_ms, host_explain_ms=host_ms, host_threads=os.cpu_count() if not os.environ.get("MSIM_HOST_THREADS") else int(os.environ["MSIM_HOST_THREADS"]),
                       records_identical=same, key_records=int(len(keys)), keys_max=int(max(len(k) for _, k in res)), invalid_keys=int((keys["valid"] == 0).sum()),
                       unknown_keys=int((keys["valid"] == 2).sum()), keys_sha=hashlib.sha256(keys.tobytes()).hexdigest()[:16])
    line = json.dumps(out)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, "profiles", f"{a.round}_lin_explain_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")
    if not a.plain_only and not out["records_identical"]:
        sys.exit("the device's and the host's key records differ")


if __name__ == "__main__":
    main()
