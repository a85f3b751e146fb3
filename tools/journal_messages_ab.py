"""The net journals of a run analysed by two routes, side by side in one process: A, msim_journal_messages over the journal slab where
it lies in HBM (journal_messages_kernel); B, the route a caller had without it — msim_fetch, then the host walk
(msim_journal_messages_rows) over every instance on the granted host threads.  One JSON line per shape, the lines of
profiles/<round>_journal_messages_ab.jsonl.

    python tools/journal_messages_ab.py --round r48 [--instances 1024] [--echo-instances 16384] [--repeats 3] [--threads 16] [--out lines.jsonl]

Shapes: the headline broadcast (n=25, rate 100, 20 s, latency 0: about 1.2e5 events a journal, where the bytes matter) and many short
echo journals (about 200 events, where the launch shape matters).  journal_capacity is sized from a probe run so that no instance is
flagged.  Every repeat runs the simulation anew (not timed), then times A with the summaries alone (max_msgs 0) and with every record
(max_msgs = the most sends of a journal), then B: the fetch and the two walks, each on its own clock; A and B alternate in order.  The
first repeat warms up and is dropped.  The summaries and the records of the two routes must be identical.  The device route's bytes are
16 B per event read in each of its two sweeps plus 32 B per record written; over its time they are set against the HBM peak."""
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

HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s (specification)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--round", default="dev", help="the label in the file name under profiles/")
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--echo-instances", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("MSIM_HOST_THREADS") or os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))))
    ap.add_argument("--out", help="append the lines here instead of profiles/<round>_journal_messages_ab.jsonl")
    a = ap.parse_args()
    import numpy as np
    from maelstrom_amd import _abi as A
    from maelstrom_amd import engine as E
    import bench_configs as B
    lib = A.load()
    pool = cf.ThreadPoolExecutor(max_workers=a.threads)   # (the entries run outside the interpreter's lock)
    path = a.out or os.path.join(ROOT, "profiles", f"{a.round}_journal_messages_ab.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    shapes = {"headline broadcast n=25 rate100 20s lat0": (B.CONFIGS["cfg2 broadcast n=25 grid lat0"][0], a.instances),
              "echo n=2 rate10 5s": (dict(workload="echo", node_count=2, rate=10, time_limit=5), a.echo_instances)}
    differ = []
    for shape, (kw, n) in shapes.items():
        # the probe: the longest journal of the first instances -> a capacity no instance overflows (checked below on the whole run)
        with E.Engine(E.test_config(**kw, seed=48, journal_capacity=1)) as eng:
            eng.run(0, min(n, 64))
            eng.fetch()
            longest = max(eng.meta(i).n_events for i in range(min(n, 64)))
        cfg = E.test_config(**kw, seed=48, journal_capacity=int(longest * 1.25) + 64)
        slots = max(cfg.concurrency, cfg.n_nodes)
        ms = {k: [] for k in ("device_summary", "device_records", "fetch", "walk_summary", "walk_records")}
        with E.Engine(cfg) as eng:
            eng.run(0, n)
            eng.fetch()
            metas = [eng.meta(i) for i in range(n)]
            assert not any(m.flags for m in metas), "an instance is flagged: the capacity is too small"
            n_ev = np.array([m.n_events for m in metas], dtype=np.int64)
            d_sum, h_sum = np.zeros(n, dtype=E.JOURNAL_SUMMARY_DT), np.zeros(n, dtype=E.JOURNAL_SUMMARY_DT)
            rc = lib.msim_journal_messages(eng._ctx, d_sum.ctypes.data, None, 0, n)
            assert rc == 0, rc
            cap = int(d_sum["n_msgs"].max())
            d_rec, h_rec = np.zeros((n, cap), dtype=E.JOURNAL_MSG_DT), np.zeros((n, cap), dtype=E.JOURNAL_MSG_DT)

            def device(with_records):
                t0 = time.perf_counter()
                rc = lib.msim_journal_messages(eng._ctx, d_sum.ctypes.data, d_rec.ctypes.data if with_records else None, cap if with_records else 0, n)
                assert rc == 0, rc
                return (time.perf_counter() - t0) * 1e3

            def walk(journals, with_records):
                def one(i):
                    ev = journals[i]
                    rc = lib.msim_journal_messages_rows(ev.ctypes.data, len(ev), cfg.n_nodes, slots, h_sum[i:i + 1].ctypes.data, h_rec[i].ctypes.data if with_records else None,
                                                        cap if with_records else 0)
                    assert rc == 0, rc
                t0 = time.perf_counter()
                list(pool.map(one, range(n), chunksize=max(1, n // (a.threads * 8))))
                return (time.perf_counter() - t0) * 1e3

            def route_a():
                ms_s, ms_r = device(False), device(True)
                return {"device_summary": ms_s, "device_records": ms_r}

            def route_b():
                t0 = time.perf_counter()
                eng.fetch()
                f = (time.perf_counter() - t0) * 1e3
                journals = [eng.raw_journal(i) for i in range(n)]
                w_r = walk(journals, True)      # (the records first: the flags of the summaries kept for the comparison are the records run's)
                rec_sum = h_sum.copy()
                w_s = walk(journals, False)
                h_sum[:] = rec_sum
                return {"fetch": f, "walk_summary": w_s, "walk_records": w_r}

            for rep in range(a.repeats + 1):
                eng.run(0, n)   # (a fresh run: msim_fetch of a run already fetched copies nothing)
                got = {}
                for route in ((route_a, route_b) if rep % 2 == 0 else (route_b, route_a)):
                    got.update(route())
                if rep:
                    for k, v in got.items():
                        ms[k].append(v)
            same = d_sum.tobytes() == h_sum.tobytes() and d_rec.tobytes() == h_rec.tobytes()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        events, records = int(n_ev.sum()), int(d_sum["n_msgs"].sum())
        gb_s = (events * 16 * 2) / 1e9 / (med["device_summary"] / 1e3)
        gb_r = (events * 16 * 2 + records * 32) / 1e9 / (med["device_records"] / 1e3)
        line = json.dumps({"tool": "journal_messages_ab", "round": a.round, "shape": shape, "journals": n, "events": events, "events_mean": float(n_ev.mean()),
                           "records": records, "journal_capacity": int(cfg.journal_capacity), "host_threads": a.threads, "ms": ms, "ms_median": med,
                           "host_summary_ms_median": med["fetch"] + med["walk_summary"], "host_records_ms_median": med["fetch"] + med["walk_records"],
                           "device_summary_events_per_s": events / (med["device_summary"] / 1e3), "host_summary_events_per_s": events / ((med["fetch"] + med["walk_summary"]) / 1e3),
                           "device_records_events_per_s": events / (med["device_records"] / 1e3), "host_records_events_per_s": events / ((med["fetch"] + med["walk_records"]) / 1e3),
                           "device_summary_gb_per_s": gb_s, "device_summary_share_of_hbm_peak": gb_s / HBM_PEAK_GBS,
                           "device_records_gb_per_s": gb_r, "device_records_share_of_hbm_peak": gb_r / HBM_PEAK_GBS,
                           "undelivered": int(d_sum["undelivered"][:, 0].sum()), "valid": int((d_sum["valid"] == 1).sum()), "identical": same,
                           "sha": hashlib.sha256(d_sum.tobytes()).hexdigest()[:16]})
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")
        if not same:
            differ.append(shape)
    if differ:
        sys.exit(f"the two routes' summaries or records differ: {differ}")


if __name__ == "__main__":
    main()
