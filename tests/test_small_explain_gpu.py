"""pn-counter / g-counter, unique-ids and echo: the explanation of a verdict on the device (pn_explain_kernel, unique_explain_kernel and
unique_explain_lds_kernel, echo_explain_kernel) through E.explain_{pn,unique,echo}_batch and Engine.explain_{pn,unique_ids,echo}, against
the host entries (msim_explain_*_rows; tests/test_small_explain.py holds those to the contract's Python restatement): record, header and
the whole slab byte for byte, and exactly the stated number of histories handed to the host walk."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import small_explain_cases as K
from test_small_explain import ECHO, PN, TABLES, host_echo, host_pn, host_unique

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, BOUND = K.unique_cases(), K.unique_bound_cases()


def _explained(batch, host, cases, cap, what, **kw):
    """one batch call over `cases` (name -> (rows, n_host)): every record, header and slab the host entry's, exactly the stated hand-overs"""
    names = list(cases)
    out, hdr, recs, handed = batch([cases[n][0] for n in names], with_n_host=True, **kw)
    for i, n in enumerate(names):
        w_out, w_hdr, w_slab = host(cases[n][0], cap)
        assert out[i].tobytes() == w_out.tobytes(), (what, n, cap, out[i], w_out)
        assert hdr[i].tobytes() == w_hdr.tobytes(), (what, n, cap, hdr[i], w_hdr)
        assert recs.slab[i].tobytes() == w_slab.tobytes(), (what, n, cap, recs.slab[i][:6], w_slab[:6])
    assert handed == sum(cases[n][1] for n in names), (what, cap, handed)
    return out, hdr, recs


def test_pn_batch_equals_the_host_entry(lib):
    """all the cases in one launch: roomy, no room, the four reads of "powers of two" only, and one record short of its 1028"""
    for cap in (1100, 0, 4, 1027):
        out, hdr, segs = _explained(lambda hs, **kw: E.explain_pn_batch(hs, max_records=cap, **kw), host_pn, PN, cap, "pn")
    i = list(PN).index("powers of two")
    assert (int(hdr[i]["n_reads"]), int(hdr[i]["n_ranges"]), int(hdr[i]["truncated"])) == (4, 1023, 1)
    one = {n: PN[n] for n in ("run covers a word",)}
    out, hdr, segs = _explained(lambda hs, **kw: E.explain_pn_batch(hs, max_records=16, **kw), host_pn, one, 16, "pn alone")
    assert E.pn_analysis(out[0], hdr[0], *segs[0])["acceptable"] == [[0, 130], [1000, 1130]]


def test_unique_small_cases(lib):
    """the route of the launch: the table in LDS; under MSIM_DEV_FLAGS bit 13 (the child of test_poisoned_allocations) in HBM workspace"""
    for cap in (80, 0, 1, 2):
        out, hdr, dups = _explained(lambda hs, **kw: E.explain_unique_batch(hs, max_dups=cap, **kw), host_unique, SMALL, cap, "unique")
    for n in ("first rows in two wavefronts", "smallest and largest id"):
        _explained(lambda hs, **kw: E.explain_unique_batch(hs, max_dups=8, **kw), host_unique, {n: SMALL[n]}, 8, "unique alone")


def test_unique_device_bound(lib):
    d = A.UNIQUE_EXPLAIN_MAX_DUPS
    for cap in (d + 8, d - 1):
        out, hdr, dups = _explained(lambda hs, **kw: E.explain_unique_batch(hs, max_dups=cap, **kw), host_unique, BOUND, cap, "unique bound")
    assert [int(h["n_dups"]) for h in hdr] == [d - 1, d - 1] and [int(h["truncated"]) for h in hdr] == [1, 1]


def test_unique_tables(lib):
    """the LDS table more than half full; 19661 ids: the HBM-table route"""
    for cases in TABLES:
        out, hdr, dups = _explained(lambda hs, **kw: E.explain_unique_batch(hs, max_dups=64, **kw), host_unique, cases, 64, "unique tables")
        assert int(hdr[0]["n_dups"]) == int(out[0]["duplicated_count"]) in (40, 6)


def test_echo_batch_equals_the_host_entry(lib):
    for name, (rows, conc) in ECHO.items():
        n = int(host_echo(rows, conc, 0)[0]["error_count"])
        for cap in sorted({n + 3, 0, 1, max(n - 1, 0)}):
            _explained(lambda hs, **kw: E.explain_echo_batch(hs, conc, max_errors=cap, **kw), lambda r, c: host_echo(r, conc, c), {name: (rows, 0)}, cap, "echo")
    three = {n: (ECHO[n][0], 0) for n in ECHO if ECHO[n][1] == 3}
    assert len(three) >= 3
    out, hdr, errs = _explained(lambda hs, **kw: E.explain_echo_batch(hs, 3, max_errors=8, **kw), lambda r, c: host_echo(r, 3, c), three, 8, "echo in one launch")
    assert E.echo_analysis(out[1], hdr[1], errs[1])["errors"] == [["Expected a message with :echo", "Please echo 901", "But received", {"type": "echo_ok", "echo": "Please echo 902"}]]


def test_engine_explain_echo_with_message_loss(lib):
    """lost messages time echoes out: every history's explanation counts what check() counts, and is the host entry's"""
    cfg = E.test_config("echo", node_count=2, rate=40, time_limit=3, p_loss=0.2, seed=5)
    with E.Engine(cfg) as eng:
        eng.run(0, 16)
        eng.check()
        plain = eng.check_results().copy()
        got = eng.explain_echo(max_errors=256)
        assert eng.check_results().tobytes() == plain.tobytes() and int(plain["error_count"].sum()) > 0
        eng.fetch()
        for i, (rec, hdr, errs) in enumerate(got):
            assert int(hdr["n_errors"]) == int(plain[i]["error_count"]) and int(hdr["truncated"]) == 0
            w_out, w_hdr, w_slab = host_echo(eng.raw_history(i)[0], cfg.concurrency, 256)
            assert errs.tobytes() == w_slab[:len(errs)].tobytes() and hdr.tobytes() == w_hdr.tobytes()
            assert int(w_out["error_count"]) == int(plain[i]["error_count"])
        bad = next(g for g in got if len(g[2]))
        assert E.echo_analysis(*bad)["valid?"] is False and E.echo_analysis(*bad)["errors"][0][3] is None


def test_engine_explain_pn_with_partitions(lib):
    cfg = E.test_config("pn-counter", node_count=5, rate=30, time_limit=12, latency=10, p_loss=0.15, nemesis=["partition"], nemesis_interval=3, seed=17)
    with E.Engine(cfg) as eng:
        eng.run(0, 16)
        eng.check()
        plain = eng.check_results().tobytes()
        got = eng.explain_pn(max_records=512)
        assert eng.check_results().tobytes() == plain
        eng.fetch()
        for i, (rec, hdr, reads, ranges) in enumerate(got):
            w_out, w_hdr, w_slab = host_pn(eng.raw_history(i)[0], 512)
            assert hdr.tobytes() == w_hdr.tobytes() and reads.tobytes() + ranges.tobytes() == w_slab[:len(reads) + len(ranges)].tobytes()
            assert len(reads) == int(rec["attempt_count"]) and len(ranges) == int(rec["stable_count"])
        assert max(len(g[3]) for g in got) >= 2   # timed-out adds: several ranges
        eng.set_dev_flags(0x800)   # the checks on the host cores: the walk explains
        again = eng.explain_pn(max_records=512)
        assert all(a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes() for a, b in zip(got, again))


def test_engine_explain_pn_of_flagged_instances(lib):
    """a pn-counter launch in which about half of the clusters stop at a lowered row capacity (tests/capacity_stop_cases.py): a flagged
    instance is not valid whatever its reads say, and its explanation is still written — on the device, and byte for byte the same by the
    host walk, which is handed the instance's flags (developer flag 0x800)"""
    import capacity_stop_cases as S
    cfg, ora, _ = S.capped("crdt8-pn", "rows")
    flagged = [i for i in range(S.N) if int(ora.meta["flags"][i])]
    assert 0 < len(flagged) < S.N
    with E.Engine(cfg) as eng:
        eng.run(0, S.N)
        got = eng.explain_pn(max_records=512)
        eng.fetch()
        assert [i for i in range(S.N) if eng.meta(i).flags] == flagged and eng.check_host_rechecks() == 0
        eng.check()
        assert b"".join(g[0].tobytes() for g in got) == eng.check_results().tobytes()
        eng.set_dev_flags(0x800)
        walked = eng.explain_pn(max_records=512)
        eng.fetch()
        for i, (dev, ref) in enumerate(zip(got, walked)):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, ref)), (i, dev[:2], ref[:2])
            rec, hdr, reads, ranges = dev
            assert int(rec["valid"]) == (0 if i in flagged else 1), (i, rec)
            assert len(ranges) == int(rec["stable_count"]) >= 1 and len(reads) == int(rec["attempt_count"]) and int(hdr["truncated"]) == 0
            w_out, w_hdr, w_slab = host_pn(eng.raw_history(i)[0], 512)   # (the entry of one history knows no flags: the verdict alone may differ)
            assert hdr.tobytes() == w_hdr.tobytes() and reads.tobytes() + ranges.tobytes() == w_slab[:len(reads) + len(ranges)].tobytes()
            assert int(w_out["error_count"]) == int(rec["error_count"]) and int(w_out["valid"]) == int(int(rec["error_count"]) == 0)
        assert E.pn_analysis(*got[flagged[0]])["valid?"] is False


def test_engine_explain_unique_ids_is_clean(lib):
    cfg = E.test_config("unique-ids", node_count=3, rate=50, time_limit=3, seed=2)
    with E.Engine(cfg) as eng:
        eng.run(0, 8)
        eng.check()
        plain = eng.check_results().tobytes()
        got = eng.explain_unique_ids()
        assert eng.check_results().tobytes() == plain and eng.check_host_rechecks() == 0
        assert all(int(rec["valid"]) == 1 and not hdr.tobytes().strip(b"\0") and len(dups) == 0 for rec, hdr, dups in got)
        assert E.unique_ids_analysis(*got[0])["duplicated"] == []
        eng.set_dev_flags(0x800)   # the checks on the host cores: the walk explains
        walked = eng.explain_unique_ids()
        assert eng.check_results().tobytes() == plain and all(a.tobytes() == b.tobytes() for g, w in zip(got, walked) for a, b in zip(g, w))


def test_refusals(lib):
    L = A.load()
    hdr = np.zeros(64, dtype=np.uint64)
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        assert L.msim_explain_echo(eng._ctx, hdr.ctypes.data, None, 0, 2) == A.E_RANGE   # before msim_run
        eng.run(0, 2)
        assert L.msim_explain_pn(eng._ctx, hdr.ctypes.data, None, 0, 2) == A.E_UNSUPPORTED
        assert L.msim_explain_unique(eng._ctx, hdr.ctypes.data, None, 0, 2) == A.E_UNSUPPORTED
        assert L.msim_explain_echo(eng._ctx, hdr.ctypes.data, None, 0, 1) == A.E_RANGE   # arrays shorter than the run
        assert L.msim_explain_echo(eng._ctx, hdr.ctypes.data, None, 1, 2) == A.E_INVALID
        assert L.msim_explain_echo(eng._ctx, hdr.ctypes.data, None, 0, 2) == 0
    with E.Engine(E.test_config("unique-ids", node_count=3, rate=10, time_limit=1, seed=1)) as eng:
        eng.run(0, 2)
        assert L.msim_explain_echo(eng._ctx, hdr.ctypes.data, None, 0, 2) == A.E_UNSUPPORTED


_TRACE = """
import sys
sys.path.insert(0, {tests!r})
from maelstrom_amd import engine as E
import small_explain_cases as K
u, e = K.unique_cases(), K.echo_cases()
E.explain_unique_batch([u["clean"][0], u["empty"][0]])
E.explain_echo_batch([e["clean"][0]], 2)
print("CLEAN DONE", file=sys.stderr, flush=True)
E.explain_unique_batch([u["clean"][0], u["ties in count"][0]])
E.explain_echo_batch([e["nemesis row"][0]], 2)
"""


def test_a_clean_batch_launches_no_explaining_kernel(lib):
    """the passes traced (MSIM_DEV_FLAGS bit 12, read once per process: a child): nothing of the explanation before the unclean batches"""
    env = dict(os.environ, MSIM_DEV_FLAGS="0x1000")
    r = subprocess.run([sys.executable, "-c", _TRACE.format(tests=os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    clean, unclean = r.stderr.split("CLEAN DONE")
    assert "explain_kernel" not in clean, clean
    assert "unique_explain_kernel (LDS table) over 1 of 2" in unclean and "echo_explain_kernel over 1 of 1" in unclean, unclean


def test_no_new_kernel_keeps_private_memory():
    from maelstrom_amd import _abi
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "private_memory_audit.py"), _abi.LIB_PATH], capture_output=True, text=True, timeout=300)
    if "libmaelsim_emu" in _abi.LIB_PATH:
        return   # (the host emulator's library has no code objects)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.split()[0]) > 150
    assert not [ln for ln in r.stdout.splitlines()[1:] if "explain_kernel" in ln and ("pn_" in ln or "unique_" in ln or "echo_" in ln)], r.stdout
    code = open(_abi.LIB_PATH, "rb").read()
    assert all(k in code for k in (b"pn_explain_kernel", b"unique_explain_kernel", b"unique_explain_lds_kernel", b"echo_explain_kernel"))


def test_poisoned_allocations(lib):
    """this module again in processes of their own with every device allocation filled with 0xA5 first (MSIM_POISON is read once per
    process): no table, list, slab or record is read before it is written.  The second child also has the HBM tables of unique-ids
    (developer flag 0x2000) in chunks of at most 7 histories (0x10000: the chunks reuse one workspace)."""
    if os.environ.get("MSIM_POISON"):
        return
    for flags, only in (("0", "not poisoned and not private"), ("0x12000", "unique and not clean and not private")):
        env = dict(os.environ, MSIM_POISON="165", MSIM_DEV_FLAGS=flags)
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", only],
                           env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
