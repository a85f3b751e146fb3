"""The explaining set-full check (msim_explain_set_full, csrc/set_full_body.inc) measured at the headline shape — bench.py's broadcast
n=25, 4096 histories resident in HBM: what check_kernel costs with the parent's library and with this one (the kernel is meant to be
unchanged: the same body, the same code object), and what set_explain_kernel costs at max_elements 64 and 1408.  One JSON line per
process, the lines of profiles/r41_set_explain_ab.jsonl.

    python tools/set_explain_ab.py parent=/path/to/the/parent's/libmaelsim.so [--repeats 7] [--processes 3] > lines.jsonl

Every line is a process of its own: the run, a warm-up, then `--repeats` timed calls; min / median / max of the kernel's time between
its two events (Engine.kernel_ms()[1], what bench.py reports as roofline.checker), and for the explaining calls also the wall time
of the call (clearing the slabs and copying them to the host included).  The check lines come `--processes` times per library,
alternating; the yardstick for "the plain check did not get slower" is the range of the parent's medians.  A library is named through
MSIM_LIB; the package is this tree's (an older library lacks only the explaining entries).

One line alone:  python tools/set_explain_ab.py --one LABEL check|explain64|explain1408"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def _stats(ms, prefix=""):
    ms = sorted(ms)
    return {prefix + "min_ms": round(ms[0], 4), prefix + "median_ms": round(ms[len(ms) // 2], 4), prefix + "max_ms": round(ms[-1], 4),
            prefix + "runs": [round(x, 4) for x in ms]}


def one(label, what, repeats, n):
    import numpy as np
    import bench
    from maelstrom_amd import engine as E
    out = {"lib": label, "what": what, "n": n}
    ker, wall = [], []
    with E.Engine(bench.headline_config(E, 99)) as eng:
        eng.run(0, n)
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            if what == "check":
                eng.check()
            else:
                got = eng.explain_set_full(int(what[len("explain"):]))
            wall.append((time.perf_counter() - t0) * 1e3)
            ker.append(eng.kernel_ms()[1])
        res = eng.check_results()
    out.update(_stats(ker[1:]))
    out["records_sha"] = hashlib.sha256(np.ascontiguousarray(res).tobytes()).hexdigest()[:16]
    out["stale_mean"] = float(res["stale_count"].mean()); out["lost_mean"] = float(res["lost_count"].mean()); out["never_read_mean"] = float(res["never_read_count"].mean())
    if what != "check":
        out.update(_stats(wall[1:], "wall_"))
        out["records_written_mean"] = float(np.mean([len(g[2]) for g in got])); out["truncated"] = int(sum(int(g[1]["truncated"]) for g in got))
        out["explain_sha"] = hashlib.sha256(b"".join(g[1].tobytes() + g[2].tobytes() for g in got)).hexdigest()[:16]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs="*", help="label=path of an older libmaelsim.so whose check_kernel is timed beside this tree's")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3, help="processes per library for the check lines")
    ap.add_argument("--n", type=int, default=4096, help="histories")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds a line's process may take")
    ap.add_argument("--one", nargs=2, metavar=("LABEL", "WHAT"), help="measure one line in this process")
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], a.repeats, a.n)
    libs = [x.split("=", 1) for x in a.libs] + [["new", ""]]
    lines = [(label, path, "check") for _ in range(a.processes) for label, path in libs] + [("new", "", "explain64"), ("new", "", "explain1408")]
    for label, path, what in lines:
        env = dict(os.environ)
        env.pop("MSIM_LIB", None)
        if path:
            env["MSIM_LIB"] = os.path.abspath(path)
        cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--n", str(a.n), "--one", label, what]
        r = subprocess.run(cmd, env=env, cwd=HERE, timeout=a.timeout)
        if r.returncode != 0:   # nothing more is started on the device after a line that failed
            sys.exit(f"{label} {what}: exit status {r.returncode}")


if __name__ == "__main__":
    main()
