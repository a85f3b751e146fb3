"""Times the device analysis of unclean list-append histories (msim_classify_txn_batch: csrc/txn_check_dev.hip, txn_classify_kernel)
beside what the same histories cost without it (msim_check_txn_batch: the clean passes, then the host analysis on the host threads).

    python tools/txn_classify_timing.py [--histories 4096] [--reps 7] [--out profiles/txn_classify_timing.jsonl]

The histories are the set without isolation of tests/test_txn_classify_gpu.py (64 histories, 40 - 200 transactions, every cycle class),
tiled to `--histories`.  Both entries run in one process, alternated round by round after a warm-up; reported per entry: the median and
minimum of a host clock around the blocking call (allocation, the copies to the device, the passes, the copy back — the same work
around both), and from the library's developer trace (MSIM_DEV_FLAGS bit 0x1000, read back from stderr) the medians of where the time
goes: the two clean passes, the classification, the host analysis.  One JSON line per entry, and one for the comparison."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("MSIM_HOST_THREADS", "16")   # the host analysis' threads, stated in the record
os.environ["MSIM_DEV_FLAGS"] = hex(int(os.environ.get("MSIM_DEV_FLAGS", "0"), 0) | 0x1000)   # the batch entries read it once per process
import numpy as np  # noqa: E402

from maelstrom_amd import _abi as A  # noqa: E402
from maelstrom_amd import engine as E  # noqa: E402


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


# the trace's clock starts with the passes: "done at" figures are cumulative
TRACE = {
    "lds_pass_ms": r"\[txn-check\] LDS pass .*?: ([0-9.]+) ms",
    "clean_passes_done_ms": r"\[txn-check\] device passes: ([0-9.]+) ms",
    "classify_done_ms": r"\[txn-classify\] full analysis .*? done at ([0-9.]+) ms",
    "host_done_ms": r"\[txn-check\] host analysis of those: done at ([0-9.]+) ms",
}
COUNTS = {
    "for_classification_or_host": r"\[txn-check\] device passes: [0-9.]+ ms, (\d+) of",
    "for_host_after_classification": r"\[txn-classify\] .*?, (\d+) for the host",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--histories", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    import test_txn_classify_gpu as G
    base = G._no_isolation_hs()
    hs = [base[i % len(base)] for i in range(args.histories)]
    rs = [np.ascontiguousarray(h[0]) for h in hs]
    ps = [np.ascontiguousarray(h[1], dtype=np.uint32) for h in hs]
    ro = np.zeros(len(rs) + 1, dtype=np.uint64); ro[1:] = np.cumsum([len(x) for x in rs])
    po = np.zeros(len(ps) + 1, dtype=np.uint64); po[1:] = np.cumsum([len(x) for x in ps])
    rows, pay = np.concatenate(rs), np.concatenate(ps)
    lib = A.load()
    outs = {k: np.zeros(len(hs), dtype=E.CHECK_DT) for k in ("device", "host")}
    n_host = C.c_uint32()
    entries = {
        "device": lambda: lib.msim_classify_txn_batch(0, rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, len(hs), A.CM_STRICT_SERIALIZABLE,
                                                      outs["device"].ctypes.data, C.byref(n_host)),
        "host": lambda: lib.msim_check_txn_batch(0, rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, len(hs), outs["host"].ctypes.data),
    }
    wall = {k: [] for k in entries}
    trace = {k: {t: [] for t in TRACE} for k in entries}
    counts = {k: {} for k in entries}
    for r in range(args.warmup + args.reps):
        for k, fn in entries.items():   # alternated: every round takes each entry once
            with Stderr() as err:
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (k, rc)
            if r >= args.warmup:
                wall[k].append(dt)
                for t, pat in TRACE.items():
                    m = re.search(pat, err.text)
                    if m:
                        trace[k][t].append(float(m.group(1)))
                for t, pat in COUNTS.items():
                    m = re.search(pat, err.text)
                    if m:
                        counts[k][t] = int(m.group(1))
    assert outs["device"].tobytes() == outs["host"].tobytes(), "the two entries' records differ"
    unclean = int((outs["host"]["error_count"] != 0).sum())
    lines = []
    for k in entries:
        res = {"entry": "msim_classify_txn_batch" if k == "device" else "msim_check_txn_batch", "route": k, "histories": len(hs), "unclean": unclean,
               "transactions": int(outs[k]["attempt_count"].sum()), "edges": int(outs[k]["lost_count"].sum()), "host_threads": int(os.environ["MSIM_HOST_THREADS"]),
               "reps": args.reps, "wall_ms_median": round(statistics.median(wall[k]), 3), "wall_ms_min": round(min(wall[k]), 3)}
        res.update({t: round(statistics.median(v), 3) for t, v in trace[k].items() if v})
        res.update(counts[k])
        if k == "device":
            res["n_host"] = int(n_host.value)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    d, h = statistics.median(wall["device"]), statistics.median(wall["host"])
    lines.append(json.dumps({"comparison": "host wall / device wall", "ratio": round(h / d, 3), "device_faster": d < h}))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
