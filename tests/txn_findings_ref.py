"""The non-cycle findings of include/maelsim_txn_findings.h, restated in plain Python from that header's text: a walk over the decoded
transactions that produces the records in the contract's order.  Independent of csrc/txn_check.cpp (no tables, no passes: the
definitions as written) — tests/test_txn_findings.py holds the host entry to it byte for byte, tests/test_txn_findings_gpu.py the
device entries to the host entry.

    findings(rows, payload, rw=False) -> (header, records)      numpy records of E.TXN_EXPLAIN_DT / E.TXN_FINDING_DT, untruncated
    truncated(header, records, max_findings) -> (header, slab)  what an entry writes for max_findings
"""
import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

NV = A.NO_VALUE
BIT = {name: bit for bit, name in A.ANOMALIES.items()}
NON_CYCLE = ("G1a", "G1b", "internal", "duplicate-elements", "incompatible-order", "dirty-update", "cyclic-versions")
FIELDS = ("anomaly", "key", "inv_row", "cmp_row", "mop", "other_inv_row", "other_cmp_row", "other_mop", "element", "other_element", "count", "reserved")


class Txn:
    def __init__(self, inv, form):
        self.inv, self.cmp, self.type, self.form = inv, None, A.T_INFO, form

    def rows(self):
        return self.inv, NV if self.cmp is None else self.cmp


def _decode(words, rw):
    """payload words -> [(f, key, value)]: f 1 = append / write; a list read's value is a list, a read of nil None; a list that runs
    past the transaction's words holds the elements that are there"""
    out, i = [], 0
    while i < len(words):
        h = int(words[i]); i += 1
        f, key, x = h & 1, (h >> 1) & 0x7FFF, (h >> 16) & 0xFF
        if f:
            out.append((1, key, x))
        elif x == 0xFF:
            out.append((0, key, None))
        elif rw:
            out.append((0, key, x))
        else:
            out.append((0, key, [(int(words[i + e // 4]) >> (8 * (e % 4))) & 0xFF for e in range(x) if i + e // 4 < len(words)]))
            i += (x + 3) // 4
    return out


def _finding(anomaly, key, subject=None, mop=NV, other=None, other_mop=NV, element=NV, other_element=NV, count=0):
    inv, cmp_ = subject.rows() if subject is not None else (NV, NV)
    oinv, ocmp = other.rows() if other is not None else (NV, NV)
    return dict(anomaly=BIT[anomaly], key=key, inv_row=inv, cmp_row=cmp_, mop=mop, other_inv_row=oinv, other_cmp_row=ocmp, other_mop=other_mop,
                element=element, other_element=other_element, count=count, reserved=0)


def _transactions(rows, payload, rw, found):
    txns, open_ = [], {}
    for i in range(len(rows)):
        packed = int(rows["packed"][i])
        typ, f, proc = packed & 3, (packed >> 2) & 31, packed >> 12
        if proc == A.PROCESS_NEMESIS or f != A.F_TXN:
            continue
        off, n = int(rows["value"][i]), int(rows["time_len"][i]) >> 48
        if off + n > len(payload):
            f_ = _finding("internal", NV)
            f_["cmp_row"] = i
            found.append(f_)
            continue
        if typ == A.T_INVOKE:
            open_[proc] = Txn(i, _decode(payload[off:off + n], rw))
            txns.append(open_[proc])
        elif open_.get(proc) is not None:
            t = open_.pop(proc)
            t.cmp, t.type = i, typ
            if typ == A.T_OK:
                t.form = _decode(payload[off:off + n], rw)
    return txns


def _writers(txns, found):
    """writer(k, v), and the duplicate-elements findings of kind (b)"""
    writer, appenders = {}, {}
    for t in txns:
        for k, (f, key, v) in enumerate(t.form):
            if f:
                writer[(key, v)] = t
                appenders.setdefault((key, v), []).append((t, k))
    for (key, v), who in appenders.items():
        if len(who) > 1:
            found.append(_finding("duplicate-elements", key, who[0][0], who[0][1], who[1][0], who[1][1], element=v, count=len(who)))
    return writer


def _final(t, key):
    """(final(t, key), its micro-op) or (None, NV)"""
    v, at = None, NV
    for k, (f, k2, x) in enumerate(t.form):
        if f and k2 == key:
            v, at = x, k
    return v, at


def _list_append(txns, found):
    writer = _writers(txns, found)
    ok_reads = [(t, k, key, lst or []) for t in txns if t.type == A.T_OK for k, (f, key, lst) in enumerate(t.form) if not f]
    longest = {}
    for t, k, key, lst in ok_reads:
        if key not in longest or len(lst) > len(longest[key][3]):
            longest[key] = (t, k, key, lst)
    for t, k, key, lst in ok_reads:
        # a read holding an element twice
        for b in range(1, len(lst)):
            if lst[b] in lst[:b]:
                found.append(_finding("duplicate-elements", key, t, k, element=lst[b], other_element=b, count=lst.index(lst[b])))
                break
        # the transaction's own test
        prev = max((e for e in range(k) if not t.form[e][0] and t.form[e][1] == key), default=None)
        own = [x for f, k2, x in t.form[(0 if prev is None else prev + 1):k] if f and k2 == key]
        if prev is not None:
            plist = t.form[prev][2] or []
            good = lst == plist + own
        else:
            good = len(lst) >= len(own) and lst[len(lst) - len(own):] == own
        if not good:
            found.append(_finding("internal", key, t, k, t if prev is not None else None, NV if prev is None else prev, element=len(lst),
                                  other_element=NV if prev is None else len(plist), count=len(own)))
        ext = len(lst)
        while ext > 0 and writer.get((key, lst[ext - 1])) is t:
            ext -= 1
        for e in range(ext):
            w = writer.get((key, lst[e]))
            if w is None or w.type == A.T_FAIL:
                found.append(_finding("G1a", key, t, k, w, element=lst[e], count=e))
        if ext > 0:
            x = lst[ext - 1]
            w = writer.get((key, x))
            if w is not None and w is not t:
                fin, at = _final(w, key)
                if fin != x:
                    found.append(_finding("G1b", key, t, k, w, at, element=x, other_element=fin, count=ext - 1))
        # a prefix of the key's order?
        lt, lk, _, order = longest[key]
        if lst != order[:len(lst)] or len(lst) > len(order):
            d = next((i for i in range(min(len(lst), len(order))) if lst[i] != order[i]), min(len(lst), len(order)))
            found.append(_finding("incompatible-order", key, t, k, lt, lk, element=lst[d], other_element=order[d] if d < len(order) else NV, count=d))
    for key, (_, _, _, order) in longest.items():
        for i in range(len(order) - 1):
            a, b = writer.get((key, order[i])), writer.get((key, order[i + 1]))
            if a is not None and b is not None and a.type == A.T_FAIL and b.type != A.T_FAIL:
                found.append(_finding("dirty-update", key, b, NV, a, NV, element=order[i + 1], other_element=order[i], count=i))


def _rw_register(txns, found):
    if any(x is not None and x >= 64 for t in txns for _, _, x in t.form):
        raise ValueError("a register value >= 64: MSIM_E_INVALID")
    writer = _writers(txns, found)
    succ = {}    # key -> {v1: {v2}}
    for t in txns:
        if t.type != A.T_OK:
            continue
        for k, (f, key, v) in enumerate(t.form):
            if f:
                continue
            prev = max((e for e in range(k) if t.form[e][1] == key), default=None)
            if prev is not None:
                if t.form[prev][2] != v:
                    found.append(_finding("internal", key, t, k, t, prev, element=NV if v is None else v,
                                          other_element=NV if t.form[prev][2] is None else t.form[prev][2]))
                continue
            if v is None:
                continue
            w = writer.get((key, v))
            if w is None or w.type == A.T_FAIL:
                found.append(_finding("G1a", key, t, k, w, element=v))
                continue
            if w is not t:
                fin, at = _final(w, key)
                if fin != v:
                    found.append(_finding("G1b", key, t, k, w, at, element=v, other_element=fin))
            fin, _ = _final(t, key)
            if fin is not None and fin != v:
                succ.setdefault(key, {}).setdefault(v, set()).add(fin)
    for key, g in succ.items():   # (nil precedes every version and follows none: it is on no cycle)
        def reaches(src, dst):
            seen, todo = set(), [src]
            while todo:
                for y in g.get(todo.pop(), ()):
                    if y == dst:
                        return True
                    if y not in seen:
                        seen.add(y); todo.append(y)
            return False
        on = sorted(v for v in g if reaches(v, v))
        if on:
            found.append(_finding("cyclic-versions", key, element=on[0], count=len(on)))


def findings(rows, payload, rw=False):
    found = []
    txns = _transactions(rows, np.asarray(payload, dtype=np.uint32), rw, found)
    (_rw_register if rw else _list_append)(txns, found)
    found.sort(key=lambda f: (f["anomaly"].bit_length() - 1, f["key"], f["inv_row"], f["mop"], f["count"]))   # (stable: ties keep their row order)
    recs = np.zeros(len(found), dtype=E.TXN_FINDING_DT)
    for i, f in enumerate(found):
        for name in FIELDS:
            recs[name][i] = f[name]
    hdr = np.zeros(1, dtype=E.TXN_EXPLAIN_DT)
    for f in found:
        hdr["count"][0][f["anomaly"].bit_length() - 1] += 1
    hdr["n_findings"][0] = len(found)
    return hdr[0], recs


def truncated(header, records, max_findings):
    hdr = np.zeros(1, dtype=E.TXN_EXPLAIN_DT)
    hdr[0] = header
    hdr["n_findings"][0] = min(len(records), max_findings)
    hdr["truncated"][0] = 1 if len(records) > max_findings else 0
    slab = np.zeros(max(max_findings, 1), dtype=E.TXN_FINDING_DT)
    slab[:min(len(records), max_findings)] = records[:max_findings]
    return hdr[0], slab[:max_findings]
