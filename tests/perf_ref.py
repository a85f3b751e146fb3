"""[upstream] jepsen.checker/stats with :by-f (as jepsen.kafka/stats-checker forgives :crash) and the latency numbers behind
jepsen.checker/perf's plots, restated in plain Python over decoded op maps — from the definitions of the :stats / :perf checkers
(include/maelsim.h above msim_check_perf), not from the engine's code.  `perf(history, ...)` gives the record that
maelstrom_amd.engine.decode_perf gives; `rows_of(history)` packs op maps of any :f into history rows.

  client rows   rows whose :process is not :nemesis
  :stats        over client completions: per :f count / ok / fail / info and valid? = ok-count > 0; the totals are the sums; overall
                valid? = every :f but :crash is valid
  pairing       a completion pairs with the LATEST EARLIER UNPAIRED :invoke of the same :process (a stack per process)
  latency       (time(completion) - time(invocation)) // 1000 us, at most 0xFFFFFFFF
  groups        (f, completion type); with windows (window, f, type), window = min(invocation time // window, n_windows - 1)
  quantile q    ascending[min(n - 1, floor(n * q))], n * q a double product"""
import math

import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

QUANTILES = (0, 0.5, 0.95, 0.99, 1)
TYPES = (":ok", ":fail", ":info")
F_NUM = {kw: n for n, kw in E.F_KW.items()}
T_NUM = {kw: n for n, kw in E.TYPE_KW.items()}
MAX_F = 4
CRASH = ":crash"


def f_num(f):
    return F_NUM[f] if f in F_NUM else int(f)


def rows_of(history):
    """op maps {:type :f :process :time} -> OP_DT rows (no payload, :value 0); :f a keyword of E.F_KW or a number below 32"""
    rows = np.zeros(len(history), dtype=E.OP_DT)
    for i, op in enumerate(history):
        process = A.PROCESS_NEMESIS if op["process"] == ":nemesis" else int(op["process"])
        rows[i] = (int(op["time"]), T_NUM[op["type"]] | (f_num(op["f"]) << 2) | (process << 12), 0)
    return rows


def dist(latencies):
    v = sorted(latencies)
    n = len(v)
    if n == 0:
        return {"count": 0, "sum-us": 0, "quantiles-us": {q: 0 for q in QUANTILES}}
    return {"count": n, "sum-us": sum(v), "quantiles-us": {q: v[min(n - 1, math.floor(float(n) * float(q)))] for q in QUANTILES}}


def perf(history, window_s=None, n_windows=0):
    window_ns = int(round(window_s * 1000)) * 1_000_000 if n_windows else None
    open_invokes = {}     # process -> stack of invocation times
    counts, unpaired, lat, wlat = {}, {}, {}, {}
    for op in history:
        if op["process"] == ":nemesis":
            continue
        f, typ, p = f_num(op["f"]), op["type"], op["process"]
        if typ == ":invoke":
            open_invokes.setdefault(p, []).append(op["time"])
            continue
        counts.setdefault(f, {t: 0 for t in TYPES})[typ] += 1
        if open_invokes.get(p):
            t0 = open_invokes[p].pop()
            us = min(max(0, op["time"] - t0) // 1000, 0xFFFFFFFF)
            lat.setdefault((f, typ), []).append(us)
            if n_windows:
                wlat.setdefault((min(t0 // window_ns, n_windows - 1), f, typ), []).append(us)
        else:
            unpaired[f] = unpaired.get(f, 0) + 1
    fs = sorted(counts)
    name = lambda f: E.F_KW.get(f, f)
    rec = {"valid?": all(counts[f][":ok"] > 0 for f in fs if name(f) != CRASH),
           "count": sum(sum(c.values()) for c in counts.values()),
           "ok-count": sum(c[":ok"] for c in counts.values()), "fail-count": sum(c[":fail"] for c in counts.values()),
           "info-count": sum(c[":info"] for c in counts.values()),
           "open-count": sum(len(s) for s in open_invokes.values()), "complete?": len(fs) <= MAX_F, "by-f": {}}
    for f in fs[:MAX_F]:
        c = counts[f]
        rec["by-f"][name(f)] = {"valid?": c[":ok"] > 0, "count": sum(c.values()), "ok-count": c[":ok"], "fail-count": c[":fail"], "info-count": c[":info"],
                                "unpaired": unpaired.get(f, 0), "latency": {t: dist(lat.get((f, t), [])) for t in TYPES}}
    if n_windows:
        rec["windows"] = [{name(f): {t: dist(wlat.get((w, f, t), [])) for t in TYPES} for f in fs[:MAX_F]} for w in range(n_windows)]
    return rec


def assert_windows_sum(rec):
    """every paired op lies in exactly one window: the window counts (and sums) of a group add up to its whole-history record"""
    for f, fs in rec["by-f"].items():
        for t in TYPES:
            assert sum(w[f][t]["count"] for w in rec["windows"]) == fs["latency"][t]["count"], (f, t)
            assert sum(w[f][t]["sum-us"] for w in rec["windows"]) == fs["latency"][t]["sum-us"], (f, t)
