"""Pure-Python restatement of the explained kafka verdict (include/maelsim.h, "kafka: the explanation of a verdict";
msim_kafka_finding / msim_kafka_explain) — written from that contract over (rows, payload), independently of csrc/kafka_check.cpp: the
observations are listed first, every finding is then a question asked of the list.  `explain(rows, payload)` gives (findings, count):
the findings as tuples (anomaly, key, offset, value, other, row_a, row_b) in the contract's order, and the ten true counts."""
from maelstrom_amd import _abi as A

KEYS, OFFS = 8, 2048
BIT = {name: bit for bit, name in A.KAFKA_ANOMALIES.items()}
NONE = A.NO_VALUE


def _rows(rows):
    for i, r in enumerate(rows):
        packed, value = int(r["packed"]), int(r["value"])
        yield i, packed & 3, (packed >> 2) & 31, packed >> 12, value, int(r["time_len"]) >> 48


def _blocks(payload, at, length):
    """the blocks of a poll's payload: (key, first offset, [messages]) — and whether all of it decoded"""
    w = [int(x) for x in payload[at:at + length]]
    out, q = [], 0
    while q < length:
        h = w[q]
        q += 1
        k, n, o0 = h & 7, (h >> 8) & 0xFF, h >> 16
        words = (n + 1) // 2
        if q + words > length:
            return out, False
        out.append((k, o0, [(w[q + e // 2] >> (16 * (e & 1))) & 0xFFFF for e in range(n)]))
        q += words
    return out, True


def explain(rows, payload):
    n_words = len(payload)
    obs = []                # (key, offset, message, row) in observation order
    sends, polls, fails = [], [], []   # (key, offset, message, row) of :ok sends, (key, offset, row) of polled pairs, (key, message, row) of :fail sends
    malformed = False
    for i, typ, f, proc, value, length in _rows(rows):
        if proc == A.PROCESS_NEMESIS:
            continue
        if f == A.F_SEND:
            k, m, o = value & 63, (value >> 6) & 0x7FF, value >> 17
            if typ == A.T_OK:
                if o == 0x7FF or k >= KEYS:
                    malformed = True
                    continue
                obs.append((k, o, m, i))
                sends.append((k, o, m, i))
            elif typ == A.T_FAIL and k < KEYS:
                fails.append((k, m, i))
        elif f == A.F_POLL and typ == A.T_OK and length:
            if value + length > n_words:
                malformed = True
                continue
            blocks, whole = _blocks(payload, value, length)
            malformed |= not whole
            for k, o0, ms in blocks:
                for e, m in enumerate(ms):
                    if o0 + e < OFFS:
                        polls.append((k, o0 + e, i))
                    if o0 + e < OFFS and m < OFFS:
                        obs.append((k, o0 + e, m, i))
                    else:
                        malformed = True

    found = []
    cells = {}              # (k, o) -> its observations in order
    homes = {}              # (k, m) -> (offset, row) of the first observation of m
    for k, o, m, row in obs:
        cells.setdefault((k, o), []).append((m, row))
        homes.setdefault((k, m), (o, row))
    polled = {(k, o) for k, o, _ in polls}
    top = {}
    for k, o, _ in polls:
        top[k] = max(top.get(k, -1), o)

    for (k, o) in sorted({(k, o) for k, o, _, _ in sends}):
        if (k, o) not in polled and o < top.get(k, -1):
            row_a = min(r for kk, oo, _, r in sends if (kk, oo) == (k, o))
            found.append((BIT["lost-write"], k, o, (int(rows[row_a]["value"]) >> 6) & 0x7FF, top[k], row_a,
                          min(r for kk, oo, r in polls if (kk, oo) == (k, top[k]))))
    for (k, o), seen in cells.items():
        last, last_row = seen[-1]
        if len({m for m, _ in seen}) >= 2:
            other, row_a = next((m, r) for m, r in seen if m != last)
            found.append((BIT["inconsistent-offsets"], k, o, last, other, row_a, last_row))
        elsewhere = [(m, r) for m, r in seen if homes[(k, m)][0] != o]
        if elsewhere:
            m, row_b = elsewhere[0]
            found.append((BIT["duplicate"], k, o, m, homes[(k, m)][0], homes[(k, m)][1], row_b))
        failed = [r for kk, mm, r in fails if (kk, mm) == (k, last)]
        if (k, o) in polled and failed:
            found.append((BIT["aborted-read"], k, o, last, 0, min(failed), min(r for kk, oo, r in polls if (kk, oo) == (k, o))))

    # the streams: what each process's client remembers per key
    lp, ls = {}, {}         # (process, key) -> (offset, row)
    for i, typ, f, proc, value, length in _rows(rows):
        if proc == A.PROCESS_NEMESIS:
            continue
        if (f == A.F_ASSIGN and typ == A.T_INVOKE) or (f == A.F_POLL and typ in (A.T_FAIL, A.T_INFO)):
            for k in range(KEYS):
                lp.pop((proc, k), None)
            continue
        if typ != A.T_OK:
            continue
        if f == A.F_SEND:
            k, m, o = value & 63, (value >> 6) & 0x7FF, value >> 17
            if k >= KEYS or o >= OFFS:
                continue
            if (proc, k) in ls and o <= ls[(proc, k)][0]:
                found.append((BIT["nonmonotonic-send"], k, o, m, ls[(proc, k)][0], ls[(proc, k)][1], i))
            ls[(proc, k)] = (o, i)
        elif f == A.F_POLL and length and value + length <= n_words:
            in_this_poll = set()
            for k, o0, ms in _blocks(payload, value, length)[0]:
                if not ms:
                    continue
                inner = "int-" if k in in_this_poll else ""
                if (proc, k) in lp:
                    was, row_a = lp[(proc, k)]
                    skipped = sum((k, o) in cells for o in range(was + 1, o0))
                    if o0 <= was:
                        found.append((BIT[inner + "nonmonotonic-poll"], k, o0, ms[0], was, row_a, i))
                    elif skipped:
                        found.append((BIT[inner + "poll-skip"], k, o0, skipped, was, row_a, i))
                lp[(proc, k)] = (o0 + len(ms) - 1, i)
                in_this_poll.add(k)

    found.sort()
    count = [0] * 10
    for f in found:
        count[f[0].bit_length() - 1] += 1
    count[9] = int(malformed)
    return found, count
