"""The contracts of include/maelsim_small_explain.h restated as plain Python walks over decoded ops (E.decode_history; unique-ids decoded
as lin-tso timestamps, so that an op's :value is the packed id): the explained pn-counter / g-counter (workload/pn_counter.clj:84-125),
unique-ids ([upstream] jepsen.checker/unique-ids) and echo (workload/echo.clj:44-63) verdicts.  Written from the header's comments and
the Clojure sources; the host entries, and through them the device kernels, are held to the bytes these give."""
import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

NO = A.NO_VALUE


def _clients(ops):
    return [o for o in ops if o["process"] != ":nemesis"]


def pn(ops):
    """-> (definite sum, [(row, value, process, in_set)] in row order, [(lower, upper)] ascending)"""
    adds = [o for o in _clients(ops) if o["f"] == ":add"]
    definite = sum(o["value"] for o in adds if o["type"] == ":ok")
    acceptable = {definite}
    for o in adds:
        if o["type"] == ":info":
            acceptable |= {v + o["value"] for v in acceptable}
    vals = sorted(acceptable)
    ranges = []
    for v in vals:
        if ranges and ranges[-1][1] == v - 1:
            ranges[-1][1] = v
        else:
            ranges.append([v, v])
    reads = [(o["index"], o["value"], o["process"], int(o["value"] in acceptable)) for o in _clients(ops) if o.get("final?") and o["type"] == ":ok"]
    return definite, reads, [tuple(g) for g in ranges]


def pn_arrays(ops, cap):
    """the header and the slab of `cap` 16-byte records the contract lays out"""
    definite, reads, ranges = pn(ops)
    hdr = np.zeros(1, dtype=E.PN_EXPLAIN_DT)
    slab = np.zeros(max(cap, 1), dtype=E.PN_READ_DT)
    nr = min(len(reads), cap)
    ng = min(len(ranges), cap - nr)
    for i, r in enumerate(reads[:nr]):
        slab[i] = r
    g = slab[nr:nr + ng].view(E.PN_RANGE_DT)
    for i, r in enumerate(ranges[:ng]):
        g[i] = r
    hdr[0] = (nr, ng, int(nr < len(reads) or ng < len(ranges)), 0, definite)
    return hdr[0], slab[:cap]


def unique(ops):
    """-> [(id, count, first_row, second_row)] by count descending, then id descending"""
    rows = {}
    for o in _clients(ops):
        if o["f"] == ":generate" and o["type"] == ":ok":
            rows.setdefault(o["value"], []).append(o["index"])
    dups = [(i, len(r), r[0], r[1]) for i, r in rows.items() if len(r) >= 2]
    return sorted(dups, key=lambda d: (-d[1], -d[0]))


def unique_arrays(ops, cap):
    dups = unique(ops)
    hdr = np.zeros(1, dtype=E.UNIQUE_EXPLAIN_DT)
    slab = np.zeros(max(cap, 1), dtype=E.UNIQUE_DUP_DT)
    n = min(len(dups), cap)
    for i, d in enumerate(dups[:n]):
        slab[i] = d
    hdr[0] = (n, int(n < len(dups)))
    return hdr[0], slab[:cap]


def _echo_value(v):
    """the number of "Please echo N" / {"type": "echo_ok", "echo": "Please echo N"}"""
    return int((v["echo"] if isinstance(v, dict) else v).rsplit(" ", 1)[1])


def echo(ops, rows, concurrency):
    """-> [(invoke_row, complete_row, expected, received)] ascending; `rows` for the value a :fail / :info row carries (not looked at)"""
    open_, errs = {}, []
    for o in _clients(ops):
        if o["f"] != ":echo":
            continue
        th = o["process"] % concurrency
        if o["type"] == ":invoke":
            open_[th] = o
            continue
        inv = open_.pop(th, None)
        if inv is None:
            continue
        want = _echo_value(inv["value"])
        if o["type"] != ":ok":
            errs.append((inv["index"], NO, want, NO))
        elif _echo_value(o["value"]) != want:
            errs.append((inv["index"], o["index"], want, _echo_value(o["value"])))
    errs += [(inv["index"], NO, _echo_value(inv["value"]), NO) for inv in open_.values()]
    return sorted(errs)


def echo_arrays(ops, rows, concurrency, cap):
    errs = echo(ops, rows, concurrency)
    hdr = np.zeros(1, dtype=E.ECHO_EXPLAIN_DT)
    slab = np.zeros(max(cap, 1), dtype=E.ECHO_ERROR_DT)
    n = min(len(errs), cap)
    for i, e in enumerate(errs[:n]):
        slab[i] = e
    hdr[0] = (n, int(n < len(errs)))
    return hdr[0], slab[:cap]
