"""The contract of include/maelsim_journal.h restated in plain Python: the reference's viz/messages (net/viz.clj:27-56: every :recv
joined to the :send of its id) and basic-stats (net/checker.clj:28-41) transliterated, plus the delivery rules — the classes by the
client slots, the undelivered records, the latency quantiles, what makes a journal malformed.  TEST INFRASTRUCTURE ONLY: nothing here
calls the library; tests/test_journal_messages.py holds msim_journal_messages_rows to it."""
import math

import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

NO = A.NO_VALUE
QUANTILES = (0.0, 0.5, 0.95, 0.99, 1.0)


def is_client(e, n_nodes, slots):
    return n_nodes <= e < n_nodes + slots


def messages(events, n_nodes, slots):
    """-> (the summary's fields as a dict, the records as a list of dicts: one per :send, in journal order)"""
    n = len(events)
    latest = {}                     # id -> index of the record of the latest send
    ids = [set(), set(), set()]     # all / clients / servers
    recs = []
    send, recv = [0, 0, 0], [0, 0, 0]
    dup = orphan = extra = 0
    endpoints = set()
    in_range = True
    for i in range(n):
        msg, route = int(events["msg"][i]), int(events["route"][i])
        t, ident, src, dest = int(events["time_us"][i]), msg >> 8, route & 0xFF, (route >> 8) & 0xFF
        client = is_client(src, n_nodes, slots) or is_client(dest, n_nodes, slots)
        cls = 1 if client else 2
        endpoints |= {src, dest}
        ids[0].add(ident)
        ids[cls].add(ident)
        in_range &= ident < n
        if not msg & 0x80:
            send[0] += 1
            send[cls] += 1
            dup += ident in latest
            latest[ident] = len(recs)
            recs.append({"id": ident, "send_event": i, "recv_event": NO, "send_time_us": t, "latency_us": NO,
                         "kind": (msg & 0x7F) | (0x80 if client else 0), "route": route, "a": int(events["a"][i]), "cls": cls})
        else:
            recv[0] += 1
            recv[cls] += 1
            if ident not in latest:
                orphan += 1
                continue
            r = recs[latest[ident]]
            if r["recv_event"] != NO:
                extra += 1
                continue
            r["recv_event"], r["latency_us"] = i, max(0, t - r["send_time_us"])
    und = [0, 0, 0]
    lat = {1: [], 2: []}
    for r in recs:
        if r["recv_event"] == NO:
            und[0] += 1
            und[r["cls"]] += 1
        else:
            lat[r["cls"]].append(r["latency_us"])
    dists = []
    for cls in (1, 2):
        v = sorted(lat[cls])
        k = len(v)
        dists.append({"count": k, "sum_us": sum(v), "q_us": [v[min(k - 1, math.floor(float(k) * q))] for q in QUANTILES] if k else [0] * 5})
    bitmap = [0] * 8
    for e in endpoints:
        bitmap[e >> 5] |= 1 << (e & 31)
    summary = {"valid": int(in_range and not (dup or orphan or extra)), "n_events": n, "n_msgs": len(recs), "send_count": send, "recv_count": recv,
               "msg_count": [len(s) for s in ids], "undelivered": und, "dup_sends": dup, "orphan_recvs": orphan, "extra_recvs": extra,
               "n_nodes": n_nodes, "client_slots": slots, "endpoints": bitmap, "latency": dists}
    return summary, recs


def packed(events, n_nodes, slots, max_msgs):
    """what msim_journal_messages_rows writes -> (JOURNAL_SUMMARY_DT record, the whole slab of max_msgs JOURNAL_MSG_DT records)"""
    summary, recs = messages(events, n_nodes, slots)
    s = np.zeros(1, dtype=E.JOURNAL_SUMMARY_DT)
    for k, v in summary.items():
        if k == "latency":
            for c in range(2):
                s[0]["latency"][c]["count"], s[0]["latency"][c]["sum_us"], s[0]["latency"][c]["q_us"] = v[c]["count"], v[c]["sum_us"], v[c]["q_us"]
        else:
            s[0][k] = v
    s[0]["flags"] = A.JOURNAL_TABLE_TRUNCATED if len(recs) > max_msgs else 0
    slab = np.zeros(max_msgs, dtype=E.JOURNAL_MSG_DT)
    for k, r in enumerate(recs[:max_msgs]):
        slab[k] = tuple(r[f] for f in E.JOURNAL_MSG_DT.names)
    return s[0], slab
