"""Unclean pn-counter, unique-ids and echo histories explained by two routes, side by side in one process: the device explanation
(E.explain_{pn,unique,echo}_batch: pn_explain_kernel, unique_explain_*_kernel, echo_explain_kernel) and the route a caller had without
those kernels — the plain device check (E.check_pn_batch / check_unique_batch / check_set_full_batch) for the records, then the host
entry (msim_explain_*_rows) on every history, on the granted host threads.  One JSON line per workload, the lines of
profiles/<round>_small_explain_ab.jsonl.

    python tools/small_explain_ab.py --round r46 [--histories 4096] [--repeats 5] [--threads N] [--out lines.jsonl]

The histories are the engine's own at the bench shapes of tools/bench_configs.py (cfg1 echo; the pn-counter and the unique-ids shape),
`--histories` of them, each corrupted: a pn-counter history has every fourth :ok add turned into an :info and its first final read
moved by 100000, out of every window; a unique-ids history has every 40th acknowledged id repeated from the row 17 rows before; an echo history has every
fifth :ok answer changed.  Each route is warmed up once and then timed `--repeats` times, alternating; the time is the whole call (the
copies of the rows to the device included, which both routes make).  Records, headers and slabs of the two routes must be identical."""
import argparse
import concurrent.futures as cf
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"pn": "pn-counter n=5 rate100 20s lat100 exponential", "unique": "unique-ids n=3 rate1000 10s lat5 + partitions", "echo": "cfg1 echo n=3"}


def histories(E, kw, n):
    cfg = E.test_config(**kw, seed=46)
    with E.Engine(cfg) as eng:
        eng.run(0, n)
        eng.fetch()
        return cfg, [eng.raw_history(i)[0].copy() for i in range(n)]


def corrupt(A, name, rows):
    import numpy as np
    typ, f = rows["packed"] & 3, (rows["packed"] >> 2) & 31
    client = (rows["packed"] >> 12) != A.PROCESS_NEMESIS
    if name == "pn":
        adds = ((f == A.F_ADD) & (typ == A.T_OK) & client).nonzero()[0][::4]
        rows["packed"][adds] = (rows["packed"][adds] & np.uint32(0xFFFFFFFC)) | np.uint32(A.T_INFO)
        finals = ((typ == A.T_OK) & (((rows["packed"] >> 11) & 1) == 1) & client).nonzero()[0][:1]
        rows["value"][finals] += 100000
    elif name == "unique":
        oks = ((f == A.F_GENERATE) & (typ == A.T_OK) & client).nonzero()[0]
        for k in range(40, len(oks), 40):
            rows["value"][oks[k]] = rows["value"][oks[k - 17]]
    else:
        oks = ((f == A.F_ECHO) & (typ == A.T_OK) & client).nonzero()[0][::5]
        rows["value"][oks] += 1000
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--round", default="dev", help="the label in the file name under profiles/")
    ap.add_argument("--histories", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("MSIM_HOST_THREADS") or os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))))
    ap.add_argument("--out", help="append the lines here instead of profiles/<round>_small_explain_ab.jsonl")
    a = ap.parse_args()
    import numpy as np
    from maelstrom_amd import _abi as A
    from maelstrom_amd import engine as E
    import bench_configs as B
    pool = cf.ThreadPoolExecutor(max_workers=a.threads)   # (the entries run outside the interpreter's lock)
    path = a.out or os.path.join(ROOT, "profiles", f"{a.round}_small_explain_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    differ = []
    for name, shape in SHAPES.items():
        cfg, hs = histories(E, B.CONFIGS[shape][0], a.histories)
        hs = [corrupt(A, name, h) for h in hs]
        conc = int(cfg.concurrency)
        cap = {"pn": 256, "unique": 512, "echo": 64}[name]
        hdr_dt, rec_dt = {"pn": (E.PN_EXPLAIN_DT, E.PN_READ_DT), "unique": (E.UNIQUE_EXPLAIN_DT, E.UNIQUE_DUP_DT), "echo": (E.ECHO_EXPLAIN_DT, E.ECHO_ERROR_DT)}[name]
        entry = f"msim_explain_{name}_rows"
        lib = A.load()

        def device():
            if name == "pn":
                out, hdr, recs, n_host = E.explain_pn_batch(hs, max_records=cap, with_n_host=True)
            elif name == "unique":
                out, hdr, recs, n_host = E.explain_unique_batch(hs, max_dups=cap, with_n_host=True)
            else:
                out, hdr, recs, n_host = E.explain_echo_batch(hs, conc, max_errors=cap, with_n_host=True)
            return out, hdr, recs.slab, n_host

        def host():
            if name == "pn":
                out = E.check_pn_batch(hs)
            elif name == "unique":
                out = E.check_unique_batch(hs)
            else:
                out = E.check_set_full_batch([(h, np.zeros(1, dtype=np.uint32)) for h in hs], conc, workload=A.WL_ECHO)
            hdr = np.zeros(len(hs), dtype=hdr_dt)
            slab = np.zeros((len(hs), cap), dtype=rec_dt)
            rec = np.zeros(len(hs), dtype=E.CHECK_DT)
            extra = (conc,) if name == "echo" else ()

            def one(i):
                rc = getattr(lib, entry)(hs[i].ctypes.data, len(hs[i]), *extra, rec[i:i + 1].ctypes.data_as(A._res), hdr[i:i + 1].ctypes.data, slab[i].ctypes.data, cap)
                assert rc == 0, rc

            list(pool.map(one, range(len(hs))))
            return out, hdr, slab, 0

        routes = {"device": device, "host": host}
        ms = {r: [] for r in routes}
        last = {}
        for rep in range(a.repeats + 1):
            for r, fn in routes.items():
                t0 = time.perf_counter()
                last[r] = fn()
                if rep:                                # (the first round loads the code and warms the allocator)
                    ms[r].append((time.perf_counter() - t0) * 1e3)
        dev, ref = last["device"], last["host"]
        same = all(x.tobytes() == y.tobytes() for x, y in zip(dev[:3], ref[:3]))
        line = json.dumps({"tool": "small_explain_ab", "round": a.round, "workload": name, "shape": shape, "histories": len(hs), "rows_mean": float(np.mean([len(h) for h in hs])),
                           "unclean": int((dev[0]["valid"] != 1).sum()), "capacity": cap, "host_threads": a.threads, "device_ms": ms["device"], "host_ms": ms["host"],
                           "device_ms_median": float(np.median(ms["device"])), "host_ms_median": float(np.median(ms["host"])), "device_n_host": int(dev[3]),
                           "identical": same, "truncated": int(dev[1]["truncated"].sum()), "sha": hashlib.sha256(b"".join(x.tobytes() for x in dev[:3])).hexdigest()[:16]})
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")
        if not same:
            differ.append(name)
    if differ:
        sys.exit(f"the two routes' records, headers or slabs differ: {differ}")


if __name__ == "__main__":
    main()
