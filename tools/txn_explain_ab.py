"""The witness cycles of the transactional checkers (msim_explain_txn*, csrc/cycle_classify.inc) measured: what the classification costs
in the parent's build and in this one (the classify kernels are meant to be unchanged), and what the witness costs on top — on the device
and by the host entries on `--threads` host threads.  One JSON line per (tree, shape, what), the lines of
profiles/r38_txn_explain_ab.jsonl.

    python tools/txn_explain_ab.py parent=/path/to/a/built/checkout/of/the/parent new=. [--repeats 5] [--scale 1.0] > lines.jsonl

A tree is a checkout with its library built; every line is measured in a process of its own that imports maelstrom_amd from its tree
(the parent's package does not know the new entries): a warm-up, then `--repeats` timed calls; min / median / max in milliseconds.

Shapes: "rw5" — txn-rw-register, five nodes, partitions, 4096 histories resident in HBM (the shape of
profiles/r29_rw_large_components.jsonl): Engine.check(classify=True) against Engine.explain_txn(), each timed as the engine times its
check; "noiso" — 2048 list-append histories of a store without isolation (tests/test_txn_classify_gpu.no_isolation, 256 seeds, each
eight times) given on the host: classify_txn_batch against explain_txn_batch, wall time of the call, upload included.  "host": the host
entries (explain_rw_history / explain_txn_history) over the same histories, wall time.

One line alone, from inside its tree with the tree on PYTHONPATH (how the profile's alternating classify lines were taken):
    python /path/to/tools/txn_explain_ab.py --one LABEL rw5|noiso classify|explain|host"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 3), "median_ms": round(ms[len(ms) // 2], 3), "max_ms": round(ms[-1], 3), "runs": [round(x, 3) for x in ms]}


def _host_twin(fn, hs, model, threads):
    from concurrent.futures import ThreadPoolExecutor
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:      # (the entries run outside the interpreter lock)
        got = list(ex.map(lambda h: fn(h[0], h[1], model, 64), hs))
    return (time.perf_counter() - t0) * 1e3, got


def one(label, shape, what, repeats, scale, threads):
    import numpy as np
    from maelstrom_amd import engine as E
    out = {"tree": label, "shape": shape, "what": what}
    ms = []
    if shape == "rw5":
        n = max(1, int(4096 * scale))
        cfg = E.test_config(seed=99, workload="txn-rw-register", rate=100, time_limit=30, nemesis=["partition"], nemesis_interval=10,
                            consistency_model="serializable", node_count=5, latency=5)
        with E.Engine(cfg) as eng:
            eng.run(0, n)
            for r in range(repeats + 1):
                if what == "classify":
                    eng.check(classify=True)
                    res = eng.check_results()
                    ms.append(eng.kernel_ms()[1])
                elif what == "explain":
                    got = eng.explain_txn(64)
                    res = eng.check_results()
                    ms.append(eng.kernel_ms()[1])
                else:
                    if r == 0:
                        eng.fetch()
                        hs = [tuple(a.copy() for a in eng.raw_history(i)) for i in range(n)]
                    t, got = _host_twin(E.explain_rw_history, hs, "serializable", threads)
                    res = np.asarray([g[0] for g in got])
                    ms.append(t)
            out["host_rechecks"] = eng.check_host_rechecks() if what != "host" else None
    else:
        sys.path.insert(0, os.path.join(HERE, "tests"))
        import test_txn_classify_gpu as T
        seeds = max(1, int(256 * scale))
        base = [E.encode_txn_history(T.no_isolation(9000 + i, (3, 8, 17)[i % 3], (1, 3, 10)[(i // 3) % 3], 60 + (i * 37) % 140,
                                                    sticky=(0.0, 0.9, 0.99, 0.995)[(i // 9) % 4], p_append=(0.45, 0.12)[(i // 36) % 2])) for i in range(seeds)]
        hs = base * 8
        n = len(hs)
        for r in range(repeats + 1):
            t0 = time.perf_counter()
            if what == "classify":
                res, handed = E.classify_txn_batch(hs, "strict-serializable")
            elif what == "explain":
                res, cyc, steps, handed = E.explain_txn_batch(hs, "strict-serializable", max_steps=64)
                got = [(None, c) for c in cyc]
            else:
                t, got = _host_twin(E.explain_txn_history, hs, "strict-serializable", threads)
                res = np.asarray([g[0] for g in got])
                handed = None
            ms.append((time.perf_counter() - t0) * 1e3)
        out["host_rechecks"] = handed
    out.update(_stats(ms[1:]), n=n, threads=threads if what == "host" else None,
               records_sha=hashlib.sha256(np.ascontiguousarray(res).tobytes()).hexdigest()[:16],
               cycle_txns_mean=float(np.mean([int(r["stale_count"]) for r in res])))
    if what != "classify":
        lens = np.asarray([int(g[1]["length"]) for g in got])
        out.update(witnessed=int((lens > 0).sum()), witness_len_mean=float(lens[lens > 0].mean()) if (lens > 0).any() else 0.0, witness_len_max=int(lens.max()),
                   cycles_sha=hashlib.sha256(b"".join(g[1].tobytes() for g in got)).hexdigest()[:16])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trees", nargs="*", help="label=path of a built checkout; the explain and host lines are measured in the LAST one")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each shape's histories (a quick look)")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the host entries' lines")
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds a line's process may take")
    ap.add_argument("--one", nargs=3, metavar=("LABEL", "SHAPE", "WHAT"), help="measure one line in this process")
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], a.one[2], a.repeats, a.scale, a.threads)
    if not a.trees:
        ap.error("name at least one tree: label=path")
    trees = [x.split("=", 1) for x in a.trees]
    for shape in ("rw5", "noiso"):
        lines = [(label, path, "classify") for label, path in trees] + [(trees[-1][0], trees[-1][1], w) for w in ("explain", "host")]
        for label, path, what in lines:
            tree = os.path.abspath(path)
            env = dict(os.environ, PYTHONPATH=tree)
            env.pop("MSIM_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--scale", str(a.scale), "--threads", str(a.threads),
                   "--one", label, shape, what]
            r = subprocess.run(cmd, env=env, cwd=tree, timeout=a.timeout)
            if r.returncode != 0:
                sys.exit(f"{label} {shape} {what}: exit status {r.returncode}")


if __name__ == "__main__":
    main()
