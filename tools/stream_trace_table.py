#!/usr/bin/env python3
"""Developer tool: where the kernels of bench.py's pipelined steps lie in time, per stream, from a rocprofv3 --kernel-trace result.

    rocprofv3 --kernel-trace -d DIR -o t -- python bench.py --gpus 1 --steps 20 --warmup 5 --cpu-sample 0
    tools/stream_trace_table.py DIR [--warmup 5] [--steps 20] [--show 8]

Reads every rocpd database under DIR, takes the process that dispatched the simulation kernel, numbers the first warmup + steps
launches of `sim_kernel` in start order (the warm-up and the timed region: the secondary legs come after them) and pairs every launch
with the first `check_kernel` that starts after it ended on the same hardware queue (one per context's stream).  Prints a table of
start / end times over `--show` steady steps and three figures over the timed steps but the first and last three: how long after its
simulation's end a check starts (in ms and in steps), how many simulation launches are resident on average (summed durations / span)
and the same for the checks."""
import argparse
import glob
import os
import sqlite3
import statistics as st


def table(con, prefix):
    return [r[0] for r in con.execute("select name from sqlite_master where type='table'") if r[0].startswith(prefix)][0]


def dispatches(path):
    con = sqlite3.connect(path)
    try:
        kd, ks = table(con, "rocpd_kernel_dispatch"), table(con, "rocpd_info_kernel_symbol")
    except IndexError:
        return []
    q = f"select s.display_name, d.queue_id, d.stream_id, d.start, d.end from '{kd}' d join '{ks}' s on d.kernel_id = s.id order by d.start"
    return [(n, qid, sid, a, b) for n, qid, sid, a, b in con.execute(q)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--show", type=int, default=8)
    a = ap.parse_args()
    rows = []
    for p in sorted(glob.glob(os.path.join(a.dir, "**", "*.db"), recursive=True)):
        d = dispatches(p)
        if sum("sim_kernel" in r[0] for r in d) > sum("sim_kernel" in r[0] for r in rows):
            rows = d
    sims = [r for r in rows if "sim_kernel" in r[0]][:a.warmup + a.steps]
    checks = [r for r in rows if r[0].startswith("check_kernel") or " check_kernel" in r[0]]
    assert len(sims) == a.warmup + a.steps, f"{len(sims)} simulation launches in the trace"
    by_stream = len({r[2] for r in sims}) > 1   # stream ids are only there when the HIP runtime was traced too: else the hardware queue
    key = (lambda r: r[2]) if by_stream else (lambda r: r[1])
    pairs, used = [], set()
    for k, s in enumerate(sims):
        c = next((i for i, c in enumerate(checks) if i not in used and key(c) == key(s) and c[3] >= s[4]), None)
        if c is not None:
            used.add(c)
        pairs.append((k, s, checks[c] if c is not None else None))
    timed = pairs[a.warmup:]
    step_ms = (timed[-1][1][3] - timed[0][1][3]) / 1e6 / (len(timed) - 1)
    steady = timed[3:-3]
    lo = steady[0][0] + (len(steady) - a.show) // 2 if len(steady) > a.show else steady[0][0]
    shown = [p for p in steady if lo <= p[0] < lo + a.show]
    t0 = shown[0][1][3]
    ms = lambda t: (t - t0) / 1e6
    print(f"# {a.dir}: {len(rows)} dispatches; launches numbered from 0 in start order (warm-up 0..{a.warmup - 1}, timed {a.warmup}..{a.warmup + a.steps - 1}); "
          f"times in ms from the start of launch {shown[0][0]}'s simulation; {'stream' if by_stream else 'queue'} = the {'HIP stream' if by_stream else 'hardware queue'} of the launch")
    print(f"{'launch':>6s} {'stream' if by_stream else 'queue':>6s} {'sim start':>10s} {'sim end':>10s} {'sim ms':>8s} {'chk start':>10s} {'chk end':>10s} {'chk ms':>8s} {'end->chk ms':>12s} {'in steps':>9s}")
    for k, s, c in shown:
        line = f"{k:6d} {key(s):6d} {ms(s[3]):10.3f} {ms(s[4]):10.3f} {(s[4] - s[3]) / 1e6:8.3f}"
        if c:
            line += f" {ms(c[3]):10.3f} {ms(c[4]):10.3f} {(c[4] - c[3]) / 1e6:8.3f} {(c[3] - s[4]) / 1e6:12.3f} {(c[3] - s[4]) / 1e6 / step_ms:9.2f}"
        print(line)
    gaps = [(c[3] - s[4]) / 1e6 for _, s, c in steady if c]
    span = (steady[-1][1][3] - steady[0][1][3]) / 1e6 * len(steady) / (len(steady) - 1)
    sim_res = sum((s[4] - s[3]) / 1e6 for _, s, _ in steady) / span
    chk_res = sum((c[4] - c[3]) / 1e6 for _, _, c in steady if c) / span
    print(f"# launches {steady[0][0]}..{steady[-1][0]}: step (start to start of the simulations) {step_ms:.3f} ms; simulation {st.mean((s[4] - s[3]) / 1e6 for _, s, _ in steady):.3f} ms, "
          f"check {st.mean((c[4] - c[3]) / 1e6 for _, _, c in steady if c):.3f} ms per launch")
    print(f"# a check starts {st.mean(gaps):.3f} ms (median {st.median(gaps):.3f}) = {st.mean(gaps) / step_ms:.2f} steps after its simulation ended; "
          f"simulations resident on average {sim_res:.2f}, checks {chk_res:.2f}")


if __name__ == "__main__":
    main()
