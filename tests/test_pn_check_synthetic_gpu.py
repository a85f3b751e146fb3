"""The pn-counter checker on the device (csrc/pn_check_dev.hip: the acceptable sums as a 4096-bit set, a word per lane, shifted across
lanes with ds_bpermute) at the edges of that set, against two judges: the host checker (msim_check_pn_rows, csrc/pn_check.cpp: sorted
ranges) and a plain Python reference that keeps the exact set of subset sums in Python integers (pn_counter.clj:84-123: every final :ok
read is the sum of the :ok adds plus any subset of the :info adds).  Device record = host record on every field the checker fills;
both = the Python reference on valid, attempt_count (final :ok reads), error_count (those outside the set) and stable_count (maximal
ranges of the set).

The edges: a window `pos - neg` of 4094..4097 values (4096 and wider is the host's), shifts by whole words (multiples of 64, where the
neighbour word must contribute nothing) and by 64 k +- 1 on a set that already has bits in several words, 1024 / 1025 indeterminate
adds, INT32_MIN / INT32_MAX deltas, a definite sum beyond 32 bits, final reads at the first and last bit and just outside, rows that
do not count (nemesis, :fail / :info / not final reads), 0 / 64 / 65 / 128 rows.  The checker has no developer trace: which level
answered is not observable here, only that the answer is the same.  tests/test_hipemu_parity.py runs this file on the host wavefront
emulator in the CPU suite."""
import ctypes as C
import random

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

pytestmark = pytest.mark.gpu
FIELDS = ("valid", "attempt_count", "error_count", "stable_count", "op_count", "ok_count", "fail_count", "info_count", "lost_count", "stale_count",
          "never_read_count", "duplicated_count")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def ok_add(d): return {"type": ":ok", "f": ":add", "value": d}
def info_add(d): return {"type": ":info", "f": ":add", "value": d}
def final(v, typ=":ok"): return {"type": typ, "f": ":read", "value": v, "final?": True}


def reference(ops):
    """(valid, final :ok reads, those outside the acceptable set, maximal ranges, the set) by the definition, in Python integers"""
    ops = [o for o in ops if o.get("process", 0) != A.PROCESS_NEMESIS]
    definite = sum(o["value"] for o in ops if o["f"] == ":add" and o["type"] == ":ok")
    acc = {definite}
    for o in ops:
        if o["f"] == ":add" and o["type"] == ":info":
            acc |= {v + o["value"] for v in acc}
    reads = [o["value"] for o in ops if o["f"] == ":read" and o["type"] == ":ok" and o.get("final?")]
    errors = sum(1 for v in reads if v not in acc)
    ranges = sum(1 for v in acc if v - 1 not in acc)
    return int(errors == 0), len(reads), errors, ranges, acc


def names_index(cases, name):
    return list(cases).index(name)


def _host(rows):
    res = A.CheckResult()
    rows = np.ascontiguousarray(rows)
    assert A.load().msim_check_pn_rows(rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(res), None, 0, None) == 0
    return res


def _check(cases):
    """cases: {name: ops}.  One batch through the device checker; every record against the host's and the reference's."""
    names = list(cases)
    hs = [E.encode_pn_history(cases[n]) for n in names]
    dev = E.check_pn_batch(hs)
    for i, name in enumerate(names):
        h = _host(hs[i])
        for f in FIELDS:
            assert int(dev[i][f]) == int(getattr(h, f)), (name, f, int(dev[i][f]), int(getattr(h, f)))
        valid, attempts, errors, ranges, _ = reference(cases[name])
        got = (int(dev[i]["valid"]), int(dev[i]["attempt_count"]), int(dev[i]["error_count"]), int(dev[i]["stable_count"]))
        assert got == (valid, attempts, errors, ranges), (name, got, (valid, attempts, errors, ranges))
    return dev


def _probe(ops, extra=()):
    """`ops` plus final reads at every edge of its acceptable set: the ends of each maximal range and the values just outside them,
    the window's first and last value and the values on either side of the 4096-bit map"""
    _, _, _, _, acc = reference(ops)
    lo, hi = min(acc), max(acc)
    vals = {lo - 1, lo, hi, hi + 1, lo + 4095, lo + 4096, lo + 4094, lo - 64, hi + 64}
    edges = sorted(v for v in acc if v - 1 not in acc or v + 1 not in acc)
    step = max(1, len(edges) // 40)
    for v in edges[::step] + edges[-2:]:
        vals |= {v - 1, v, v + 1}
    vals |= set(extra)
    return ops + [final(v) for v in sorted(vals) if I32_MIN <= v <= I32_MAX]


def _spread():
    """indeterminate adds that put bits into more than three words of the map before the shift under test: {0, 1, 70, 71, 130, 131, 200, 201}"""
    return [info_add(1), info_add(70), info_add(130)]


def test_window_widths(lib):
    """pos - neg of 4094, 4095 (the last the bitmap takes), 4096 and 4097 (the host's), from one large delta and from many small ones, upwards,
    downwards and both"""
    cases = {}
    for w in (4094, 4095, 4096, 4097):
        cases[f"one+{w}"] = _probe([ok_add(7), info_add(w)])
        cases[f"one-{w}"] = _probe([ok_add(-7), info_add(-w)])
        cases[f"split{w}"] = _probe([ok_add(3), info_add(w - 2000), info_add(-2000)])
        small = [info_add(37)] * (w // 37) + [info_add(w % 37)]            # every multiple of 37 and those plus the rest
        cases[f"many+{w}"] = _probe([ok_add(100)] + small)
        mixed = [info_add(-64)] * 20 + [info_add(63)] * ((w - 1280) // 63) + [info_add((w - 1280) % 63)]
        assert sum(abs(o["value"]) for o in mixed) == w
        cases[f"many+-{w}"] = _probe([ok_add(-100)] + mixed)
    _check(cases)


def test_shift_amounts(lib):
    """every shift the kernel takes apart into a lane distance and a bit distance: whole words (the bit distance 0: the neighbour word
    contributes nothing), one more and one less, the widest, none — on a set with bits in four words"""
    cases = {}
    for k in (1, 2, 31, 63):
        for d in (64 * k, 64 * k + 1, 64 * k - 1):
            # (beside a shift of 63 words only 62 values are left of the window: a set that straddles two words)
            spread = _spread() if k < 63 else [info_add(1), info_add(-30), info_add(31)]
            for sign in (1, -1):
                cases[f"{sign * d}"] = _probe(spread + [info_add(sign * d), info_add(0)])
                cases[f"{sign * d} first"] = _probe([info_add(sign * d), info_add(0)] + spread)
    for d in (4095, -4095):
        cases[f"{d}"] = _probe([info_add(d), info_add(0)])
    # two whole-word shifts in a row, in both directions, on a set whose words are full to the top bit
    cases["full words"] = _probe([ok_add(5)] + [info_add(1)] * 130 + [info_add(64), info_add(-128), info_add(1920), info_add(-1920)])
    cases["zero only"] = _probe([ok_add(9), info_add(0), info_add(0)])
    dev = _check(cases)
    assert (dev["valid"] == 0).all()   # (every probe has reads just outside the set)


def test_indeterminate_add_count(lib):
    """1024 indeterminate adds (the kernel's table) and 1025 (the host's), +1 and -1 mixed so that the window stays 1024 / 1025 wide; and
    1025 whose window is too wide as well"""
    cases = {}
    for n in (1023, 1024, 1025):
        adds = [info_add(1 if i % 2 else -1) for i in range(n)]
        cases[f"{n}"] = _probe([ok_add(50)] + adds)
        cases[f"{n} zeros"] = _probe([ok_add(50)] + [info_add(0)] * (n - 2) + [info_add(3), info_add(-64)])
    cases["1025 wide"] = _probe([info_add(4 if i % 2 else -4) for i in range(1025)])
    _check(cases)


def test_extreme_deltas_and_sums(lib):
    """INT32_MIN / INT32_MAX as indeterminate deltas (the window is far wider than the bitmap: the host's, and never `-d`), as definite
    ones, and a definite sum beyond 32 bits in either direction, which no 32-bit read can equal"""
    cases = {
        "info min": _probe([ok_add(1), info_add(I32_MIN), info_add(3)], extra=(I32_MIN, I32_MIN + 1, I32_MIN + 4, 1, 4)),
        "info max": _probe([ok_add(-1), info_add(I32_MAX), info_add(-3)], extra=(I32_MAX - 1, I32_MAX - 4, -1, -4)),
        "info min max": _probe([info_add(I32_MIN), info_add(I32_MAX), info_add(0)], extra=(-1, 0, I32_MIN, I32_MAX)),
        "ok min": _probe([ok_add(I32_MIN), info_add(5)], extra=(I32_MIN, I32_MIN + 5)),
        "ok max": _probe([ok_add(I32_MAX), info_add(-5)], extra=(I32_MAX, I32_MAX - 5)),
        "ok min twice": _probe([ok_add(I32_MIN), ok_add(I32_MIN), info_add(64)], extra=(0, 64, I32_MIN, I32_MAX)),
        "ok max x3": _probe([ok_add(I32_MAX)] * 3 + [info_add(-64), info_add(1)], extra=(I32_MAX, I32_MAX - 2, I32_MAX - 3, -3, -67)),
        "beyond and back": _probe([ok_add(I32_MAX)] * 2 + [ok_add(I32_MIN)] * 2 + [info_add(100), info_add(-100)], extra=(-2, -102, 98, 0)),
        "just beyond": _probe([ok_add(I32_MAX), ok_add(10), info_add(-20), info_add(64)], extra=(I32_MAX, I32_MAX - 10, I32_MAX - 9)),
    }
    dev = _check(cases)
    assert (dev["attempt_count"] > 0).all()


def test_beyond_and_back_by_hand(lib):
    """the previous test's one figure stated by hand, so that it does not rest on the reference alone: 2 (2^31 - 1) - 2 * 2^31 = -2,
    acceptable {-102, -2, 98}"""
    ops = [ok_add(I32_MAX)] * 2 + [ok_add(I32_MIN)] * 2 + [info_add(100), info_add(-100)]
    assert reference(ops)[4] == {-102, -2, 98}
    dev = _check({"in": ops + [final(-102), final(-2), final(98)], "out": ops + [final(-103), final(-101), final(0), final(99), final(-2)]})
    assert [int(d["valid"]) for d in dev] == [1, 0] and int(dev[1]["error_count"]) == 4 and int(dev[0]["stable_count"]) == 3


def test_final_reads(lib):
    """reads at lo - 1, lo, lo + 4095 and lo + 4096 of a set that fills its window, each alone and together; and what is not a final :ok
    read — :fail and :info final reads, :ok reads that are not final, a nemesis row — is not counted whatever it carries"""
    full = [ok_add(-2000)] + [info_add(1)] * 63 + [info_add(64)] * 63       # every value of [-2000, 2095]: 4096 of them, window 4095
    assert reference(full)[4] == set(range(-2000, 2096))
    cases = {}
    for name, v in (("lo-1", -2001), ("lo", -2000), ("lo+4095", 2095), ("lo+4096", 2096)):
        cases[name] = full + [final(v)]
    cases["all"] = full + [final(v) for v in (-2001, -2000, 2095, 2096, 0, 63, 64)]
    sparse = [ok_add(10), info_add(4095)]                                    # {10, 4105}: the first and the last bit alone
    for name, v in (("s lo-1", 9), ("s lo", 10), ("s lo+1", 11), ("s hi-1", 4104), ("s hi", 4105), ("s hi+1", 4106)):
        cases[name] = sparse + [final(v)]
    ignored = [final(77, ":fail"), final(78, ":info"), {"type": ":ok", "f": ":read", "value": 79}, {"type": ":invoke", "f": ":read", "value": None, "final?": True},
               {"type": ":ok", "f": ":read", "value": 80, "final?": True, "process": A.PROCESS_NEMESIS},
               {"type": ":info", "f": ":add", "value": 1000, "process": A.PROCESS_NEMESIS}, {"type": ":fail", "f": ":add", "value": 500}]
    cases["ignored only"] = sparse + ignored
    cases["ignored + good"] = sparse + ignored + [final(10), final(4105)]
    cases["ignored + bad"] = ignored + sparse + [final(1010)]
    cases["no reads"] = full
    dev = _check(cases)
    want = {"lo-1": 0, "lo": 1, "lo+4095": 1, "lo+4096": 0, "s lo-1": 0, "s lo": 1, "s lo+1": 0, "s hi-1": 0, "s hi": 1, "s hi+1": 0, "ignored only": 1, "ignored + good": 1,
            "ignored + bad": 0, "no reads": 1}
    for name, v in want.items():
        assert int(dev[names_index(cases, name)]["valid"]) == v, name
    assert int(dev[names_index(cases, "all")]["error_count"]) == 2 and int(dev[names_index(cases, "ignored only")]["attempt_count"]) == 0


def test_row_layout(lib):
    """0 rows; 64, 65 and 128 rows (the kernel reads 64 a time) with the deciding rows first, last and on either side of the boundary;
    nemesis rows in between"""
    nem = {"type": ":info", "f": ":add", "value": 999, "process": A.PROCESS_NEMESIS}
    cases = {"empty": []}
    for n in (63, 64, 65, 127, 128, 129):
        body = [info_add(64), ok_add(3), info_add(-129)]
        reads = [final(3), final(67), final(-126), final(-62), final(4)]
        pad = n - len(body) - len(reads)
        fill = [nem if i % 3 == 0 else {"type": ":invoke", "f": ":add", "value": 5} if i % 3 == 1 else {"type": ":fail", "f": ":add", "value": 5} for i in range(pad)]
        cases[f"{n} head"] = body + reads + fill
        cases[f"{n} tail"] = fill + body + reads
        cases[f"{n} split"] = body + fill + reads
        assert all(len(cases[f"{n} {w}"]) == n for w in ("head", "tail", "split"))
    dev = _check(cases)
    assert int(dev[0]["valid"]) == 1 and int(dev[0]["stable_count"]) == 1
    assert all(int(d["error_count"]) == 1 and int(d["attempt_count"]) == 5 and int(d["stable_count"]) == 4 for d in dev[1:])


def _random_case(seed):
    """a window drawn around 4096 (from a quarter of it to twice), made of 1..40 indeterminate deltas of both signs — some of them whole
    words —, definite adds, and final reads drawn from the set, from its edges and from outside"""
    rnd = random.Random(seed)
    target = rnd.choice([rnd.randrange(1, 1200), rnd.randrange(3000, 4096), rnd.randrange(4090, 4102), rnd.randrange(4096, 9000)])
    n = rnd.randrange(1, 14) if target > 4200 else rnd.randrange(1, 41)   # (the host's ranges double with every delta that joins nothing)
    cuts = sorted(rnd.randrange(target + 1) for _ in range(n - 1))
    mags = [b - a for a, b in zip([0] + cuts, cuts + [target])]
    mags = [m - m % 64 if rnd.random() < 0.25 else m for m in mags]
    ops = [ok_add(rnd.randrange(-5000, 5000)) for _ in range(rnd.randrange(4))]
    ops += [info_add(m if rnd.random() < 0.5 else -m) for m in mags]
    ops += [{"type": ":fail", "f": ":add", "value": rnd.randrange(-50, 50)} for _ in range(rnd.randrange(3))]
    rnd.shuffle(ops)
    acc = sorted(reference(ops)[4])
    reads = [rnd.choice(acc) for _ in range(rnd.randrange(6))]
    if rnd.random() < 0.5:
        reads += [rnd.choice(acc) + rnd.choice([-1, 1, 64, -64]) for _ in range(rnd.randrange(1, 4))]
    return _probe(ops + [final(v) for v in reads])


def test_random_histories(lib):
    """200 histories whose windows fall on both sides of 4096"""
    cases = {f"seed {s}": _random_case(s) for s in range(200)}
    widths = []
    for ops in cases.values():
        d = [o["value"] for o in ops if o["f"] == ":add" and o["type"] == ":info"]
        widths.append(sum(abs(x) for x in d))
    assert sum(w < 4096 for w in widths) >= 60 and sum(w >= 4096 for w in widths) >= 40 and any(4090 <= w < 4096 for w in widths), sorted(widths)
    dev = _check(cases)
    assert int((dev["stable_count"] > 8).sum()) >= 20
