"""The synthetic histories of the explained pn-counter, unique-ids and echo verdicts (tests/test_small_explain*.py): small — tens to a few
thousand rows, the two unique-ids histories that fill the tables apart — and shaped after the places where the kernels can go wrong.
Each set is a dict name -> (rows, n_host): n_host = 1 where the contract hands the history to the host walk."""
import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

NEMESIS = {"type": ":info", "f": ":add", "value": 77, "process": A.PROCESS_NEMESIS}   # a row no walk may look at (and every row index counts)


def _add(v, t=":ok", p=0):
    return {"type": t, "f": ":add", "value": v, "process": p}


def _read(v, final=True, t=":ok", p=1):
    return {"type": t, "f": ":read", "value": v, "final?": final, "process": p}


def _pn(*ops):
    return E.encode_pn_history(list(ops))


def pn_cases():
    c = {}
    c["empty"] = (_pn(), 0)
    c["no info"] = (_pn(_add(3), NEMESIS, _add(4), _read(7), _read(6, p=2)), 0)
    c["info 5"] = (_pn(_add(10), _add(5, ":info"), _read(10), _read(15, p=2), _read(12, p=3)), 0)
    c["reference indefinite"] = (_pn(_add(10), _add(5, ":info"), _add(-1, ":info"), _add(-1, ":info"), _read(11), _read(15)), 0)
    # 1024 one-value ranges in a window 2047 wide: every even number from 1 to 2047
    c["powers of two"] = (_pn(_add(1), *[_add(1 << k, ":info") for k in range(1, 11)], _read(1), _read(3, p=2), _read(2, p=3), _read(2047, p=4)), 0)
    ones = [_add(1, ":info")] * 63
    # [0, 63] ends on bit 63 of word 0; [128, 191] starts on bit 0 of word 2 and ends on its bit 63
    c["run ends on bit 63"] = (_pn(*ones, _add(128, ":info"), _read(63), _read(64, p=2), _read(128, p=3), _read(191, p=4), _read(192, p=5)), 0)
    c["run spans a word boundary"] = (_pn(*[_add(1, ":info")] * 10, _add(60, ":info"), _read(64), _read(11, p=2)), 0)
    # [0, 130] covers word 1 and more (start in lane 0, end in lane 2); [1000, 1130] the same from bit 40 of word 15 on
    c["run covers a word"] = (_pn(*[_add(1, ":info")] * 100, _add(30, ":info"), _add(1000, ":info"), _read(130), _read(131, p=2), _read(999, p=3), _read(1130, p=4)), 0)
    c["window 4095"] = (_pn(_add(7), _add(2000, ":info"), _add(-2095, ":info"), _read(7), _read(2007, p=2), _read(-2088, p=3), _read(-88, p=4), _read(-2089, p=5)), 0)
    c["window 4096"] = (_pn(_add(7), _add(2000, ":info"), _add(-2096, ":info"), _read(7), _read(2007, p=2), _read(-2089, p=3), _read(-89, p=4), _read(-2088, p=5)), 1)
    zeros = [_add(0, ":info")] * 1020
    c["1024 info adds"] = (_pn(*zeros, _add(1, ":info"), _add(-1, ":info"), _add(5, ":info"), _add(0, ":info"), _read(4), _read(3, p=2)), 0)
    c["1025 info adds"] = (_pn(*zeros, _add(1, ":info"), _add(-1, ":info"), _add(5, ":info"), _add(0, ":info"), _add(0, ":info"), _read(4), _read(3, p=2)), 1)
    filler = [_add(0)] * 62
    c["reads in rows 63 and 64"] = (_pn(_add(9), *filler, _read(9), _read(8, p=2), _read(9, p=3)), 0)
    c["reads that are not listed"] = (_pn(_add(2), _read(5, t=":fail"), _read(5, t=":info", p=2), _read(5, final=False, p=3), _read(2, p=4),
                                          {"type": ":invoke", "f": ":read", "value": None, "final?": True, "process": 5}), 0)
    c["below and above the window"] = (_pn(_add(100), _add(-3, ":info"), _add(4, ":info"), _read(96), _read(105, p=2), _read(101, p=3)), 0)
    many = [_read(1 if i % 3 else 3, p=i) for i in range(150)]   # more reads than a step of 64 rows, errors among them
    c["150 reads"] = (_pn(_add(1), _add(1, ":info"), _add(10, ":info"), *many, _add(-2, ":info")), 0)
    return c


def gen_rows(acks, invoked=()):
    """unique-ids rows: an :ok :generate per entry of `acks` (a packed id), in this order; the row numbers in `invoked` become :invoke rows
    (process i mod 7)"""
    n = len(acks)
    rows = np.zeros(n, dtype=E.OP_DT)
    rows["time_len"] = np.arange(n, dtype=np.uint64) * 1000
    rows["packed"] = A.T_OK | (A.F_GENERATE << 2) | ((np.arange(n, dtype=np.uint32) % 7) << 12)
    rows["value"] = np.asarray(acks, dtype=np.uint64).astype(np.uint32)
    for i in invoked:
        rows["packed"][i] = A.T_INVOKE | (A.F_GENERATE << 2) | ((i % 7) << 12)
    return rows


def _spread(n, seed):
    """n distinct ids below 2^31, none of them one of the small ids the cases duplicate"""
    rng = np.random.default_rng(seed)
    ids = np.unique(rng.integers(1 << 20, 1 << 31, size=n + n // 8, dtype=np.int64))
    rng.shuffle(ids)
    assert len(ids) >= n
    return ids[:n]


def unique_cases():
    """the small ones: every route takes them"""
    c = {}
    c["clean"] = (gen_rows(_spread(90, 1), invoked=(0, 5)), 0)
    c["empty"] = (gen_rows([]), 0)
    acks = list(_spread(200, 2)) + [11] * 2 + [12] * 3 + [13] * 70
    np.random.default_rng(3).shuffle(acks)
    c["2, 3 and 70 times"] = (gen_rows(acks, invoked=(1,)), 0)
    base = list(_spread(300, 4))
    adj = list(base); adj[10] = adj[11] = 500
    c["first rows adjacent"] = (gen_rows(adj), 0)
    far = list(base); far[5] = far[200] = far[299] = 501
    c["first rows in two chunks"] = (gen_rows(far), 0)
    wav = list(base); wav[3] = wav[70] = wav[64] = 502   # rows of the workgroup kernel's wavefronts 0 and 1: the first two are rows 3 and 64
    c["first rows in two wavefronts"] = (gen_rows(wav), 0)
    ties = list(_spread(40, 5)) + [9, 7, 8, 5, 6] * 2 + [4] * 3
    c["ties in count"] = (gen_rows(ties), 0)
    c["smallest and largest id"] = (gen_rows([0, 0xFFFFFFFF, 17, 0, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFE]), 0)
    c["one largest id"] = (gen_rows([0xFFFFFFFF, 3, 3]), 0)
    return c


def unique_bound_cases():
    """exactly the device bound of duplicated ids, and one more (the host's)"""
    d = A.UNIQUE_EXPLAIN_MAX_DUPS
    at = np.concatenate([np.arange(1, d + 1), _spread(50, 6), np.arange(d, 0, -1)])
    over = np.concatenate([np.arange(1, d + 2), _spread(50, 7), np.arange(d + 1, 0, -1), [5]])
    return {"at the bound": (gen_rows(at), 0), "beyond the bound": (gen_rows(over), 1)}


def unique_table_cases():
    """the LDS table filled to more than half (17000 of 32768 slots) with 40 duplicates; 19661 ids, so that the HBM-table route runs"""
    ids = _spread(17000, 8)
    fill = np.concatenate([ids, ids[100:4100:100]])
    np.random.default_rng(9).shuffle(fill)
    ids = _spread(19655, 10)
    hbm = np.concatenate([ids, ids[:6]])
    return {"table more than half full": (gen_rows(fill), 0)}, {"19661 ids": (gen_rows(hbm), 0)}


def echo_rows(ops):
    """echo rows: (type, process, value) per row"""
    tkw = {":invoke": A.T_INVOKE, ":ok": A.T_OK, ":fail": A.T_FAIL, ":info": A.T_INFO}
    rows = np.zeros(len(ops), dtype=E.OP_DT)
    for i, (t, p, v) in enumerate(ops):
        rows[i] = (i * 1000, tkw[t] | (A.F_ECHO << 2) | (p << 12), v)
    return rows


def _pair(p, v, t=":ok", got=None):
    return [(":invoke", p, v), (t, p, v if got is None else got)]


def echo_cases():
    """name -> (rows, concurrency)"""
    c = {}
    c["clean"] = (echo_rows(_pair(0, 1) + _pair(1, 2) + _pair(0, 3)), 2)
    c["empty"] = (echo_rows([]), 3)
    # 62 rows of pairs, an invocation in row 62 that completes in row 65, between them an invocation in row 63 whose :ok in row 64 carries another value
    ops = sum((_pair(i % 3, i) for i in range(31)), []) + [(":invoke", 0, 900), (":invoke", 1, 901), (":ok", 1, 902), (":ok", 0, 900)]
    c["invocation in row 63"] = (echo_rows(ops), 3)
    inter = [(":invoke", 0, 1), (":invoke", 1, 2), (":invoke", 2, 3), (":ok", 2, 3), (":ok", 1, 9), (":invoke", 2, 4), (":fail", 0, 1), (":info", 2, 4),
             (":invoke", 5, 5), (":ok", 5, 5), (":invoke", 8, 6), (":ok", 8, 7), (":invoke", 0, 8), (":invoke", 1, 10)]
    c["every kind of error"] = (echo_rows(inter), 3)   # (process 5 and 8 are the successors of 2: 2 + 3, 5 + 3)
    c["concurrency 1"] = (echo_rows(_pair(0, 1) + _pair(0, 2, got=3) + _pair(0, 4, ":info") + _pair(1, 5) + _pair(1, 6, ":fail") + [(":invoke", 1, 7)]), 1)
    wide = [(":invoke", p, 100 + p) for p in range(64)] + [(":ok" if p % 5 else ":fail", p, 100 + p + (p % 7 == 0)) for p in reversed(range(64))]
    wide += [(":invoke", p + 64, 300 + p) for p in range(0, 64, 5)] + [(":ok", p + 64, 300 + p) for p in range(0, 64, 10)]
    c["concurrency 64"] = (echo_rows(wide), 64)
    # the last thread's invocation, in row 0, never completes: the lane that notes it is not the lane that writes its record
    c["open invocation of thread 63 in row 0"] = (echo_rows([(":invoke", 63, 5)] + _pair(0, 1) + _pair(1, 2, got=3)), 64)
    nem = echo_rows(_pair(0, 1, got=2) + [(":info", 0, 0)] + _pair(1, 3, ":fail"))
    nem["packed"][2] = A.T_INFO | (A.F_START_PARTITION << 2) | (A.PROCESS_NEMESIS << 12)
    c["nemesis row"] = (nem, 2)
    many = sum((_pair(i % 4, i, got=i + (i % 2)) for i in range(200)), [])
    c["100 errors"] = (echo_rows(many), 4)
    return c
