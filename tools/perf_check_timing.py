"""Times msim_check_perf (csrc/perf_check_dev.hip) at the shapes users run, beside two yardsticks on the same launch: the availability
checker (availability_kernel reads exactly the same row bytes: the floor) and the workload checker's check_ms.

    python tools/perf_check_timing.py [headline cfg4 cfg5] [--reps 20] [--out FILE]

Per shape one run of the engine, then — after a warm-up — `--reps` rounds that alternate, in one process, the availability pass, the perf
pass with windows off and the perf pass with 10 s x 8 windows.  Reported per pass: the median and minimum of a host clock around the
blocking call (kernel + the copy of the results) and, for the perf pass, of the kernel's own time (HIP events on the context's stream,
printed by the library under the developer trace bit 0x1000 and read back from stderr here); the history-row bytes per second of the
kernel's median and their share of the HBM peak; one JSON line per shape."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from maelstrom_amd import _abi as A  # noqa: E402
from maelstrom_amd import engine as E  # noqa: E402

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E spec peak (bench.py uses the same figure)
SHAPES = {
    "headline": (dict(workload="broadcast", bin="broadcast-ff", node_count=25, rate=100, time_limit=20, latency=0, inbox_capacity=6), 4096),
    "cfg4": (dict(workload="lin-kv", bin="raft", node_count=5, rate=30, time_limit=60), 8192),
    "cfg5": (dict(workload="txn-list-append", node_count=5, rate=100, time_limit=30, latency=5, nemesis=["partition"], nemesis_interval=10), 32768),
}


class Stderr:
    """collects what the library writes to file descriptor 2"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def measure(name, reps, warmup=3):
    kw, n = SHAPES[name]
    cfg = E.test_config(seed=1, **kw)
    with E.Engine(cfg) as eng:
        eng.run(0, n)
        eng.check()
        sim_ms, check_ms = eng.kernel_ms()
        eng.set_dev_flags(0x1000)
        lib, ctx = eng.lib, eng._ctx
        avail = (A.Availability * n)()
        out = np.zeros(n, dtype=E.PERF_DT)
        win = np.zeros((n, 8, A.PERF_MAX_F, 3), dtype=E.LATENCY_DT)
        passes = {
            "availability": lambda: lib.msim_check_availability(ctx, A.AVAIL_NIL, 0.0, avail, n),
            "perf": lambda: lib.msim_check_perf(ctx, 0, 0, out.ctypes.data, n, None),
            "perf 10 s x 8": lambda: lib.msim_check_perf(ctx, 10_000, 8, out.ctypes.data, n, win.ctypes.data),
        }
        host = {k: [] for k in passes}
        kernel = {k: [] for k in passes}
        for r in range(warmup + reps):
            for k, fn in passes.items():   # alternated: every round takes each pass once
                with Stderr() as err:
                    t0 = time.perf_counter()
                    rc = fn()
                    dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0, (k, rc, lib.msim_last_error(ctx))
                if r >= warmup:
                    host[k].append(dt)
                    m = re.search(r"\[perf-check\] kernel ([0-9.]+) ms", err.text)
                    if m:
                        kernel[k].append(float(m.group(1)))
        assert not (out["flags"] & 1).any()
        # rows the kernel read: every client row (the nemesis adds a handful per history)
        rows = int(out["count"].sum()) + int(out["open_count"].sum()) + int(out["by_f"]["latency"]["count"].sum())
    res = {"shape": name, "config": kw, "instances": n, "max_rows": int(cfg.max_rows), "client_rows": rows, "row_bytes": rows * 16,
           "sim_ms": round(sim_ms, 3), "workload_check_ms": round(check_ms, 3), "reps": reps, "passes": {}}
    for k in passes:
        p = {"host_ms_median": round(statistics.median(host[k]), 4), "host_ms_min": round(min(host[k]), 4)}
        if kernel[k]:
            med = statistics.median(kernel[k])
            gbps = rows * 16 / (med * 1e-3) / 1e9
            p.update(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(kernel[k]), 4), row_gbps=round(gbps, 1), share_of_hbm_peak=round(gbps / HBM_PEAK_GBPS, 4))
        res["passes"][k] = p
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []
    for name in args.shapes:
        res = measure(name, args.reps)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
