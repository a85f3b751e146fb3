"""What the frames the device checkers share (csrc/check_run.h) must keep, and no other module pins: the checker on the host cores
(developer flag 0x800: host_check_run) for every workload that has one, against the device route's records; the refusals of the four
msim_explain_* entries of a run (explain_refusal) with their messages; msim_explain_set_full on an armed context, which takes the queued
check as msim_check does (msim_check_take_or_arm); and the edges of the explanation slabs (ExplainSlabs) through the batch entries: no
records wanted, a clean history, a history without rows — against the host *_rows entries.  8 histories per run, small configurations."""
import ctypes as C
import re

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import lin_explain_cases as LK
import setfull_explain_ref as SX
import test_rw_classify_gpu as RWT
import test_txn_classify_gpu as T
from test_lin_check_gpu import FIELDS as LIN_FIELDS
from test_kafka_explain import HAND as KAFKA_HAND, _GOOD as KAFKA_GOOD, host as kafka_host
from test_set_explain import host as set_host
from test_txn_explain import host as txn_host

pytestmark = pytest.mark.gpu

N = 8
HOST_ROUTE, TRACE = 0x800, 0x1000
CASES = {
    "lin-kv": dict(bin="raft", node_count=5, rate=30, time_limit=20, latency=10, nemesis=["partition"], nemesis_interval=5),
    "txn-list-append": dict(node_count=5, rate=100, time_limit=10, latency=5, nemesis=["partition"], nemesis_interval=3),
    "txn-rw-register": dict(node_count=5, rate=100, time_limit=10, latency=5, nemesis=["partition"], nemesis_interval=3),
    "kafka": dict(node_count=3, rate=60, time_limit=4, latency=5, nemesis=["partition"], nemesis_interval=2),
    "pn-counter": dict(node_count=5, rate=50, time_limit=8, latency=30, p_loss=0.1),
    "g-counter": dict(node_count=5, rate=50, time_limit=8, latency=30, p_loss=0.1),
    "unique-ids": dict(node_count=3, rate=300, time_limit=5, latency=5),
}
NO_ROWS = np.zeros(0, dtype=E.OP_DT)
EMPTY = (NO_ROWS, np.zeros(0, dtype=np.uint32))


@pytest.mark.parametrize("wl", list(CASES))
def test_host_route_gives_the_device_routes_records(lib, wl):
    """msim_check under 0x800: the device route's records byte for byte, a check time, lin_host_rechecks = n for lin-kv and untouched (0)
    for the others, and the same bytes from a second check() of the same run.  (txn-rw-register with msim_set_check_classify: without it
    the device leaves a history it proves valid the record of rw_check_kernel — the edges of the subgraph it built in lost_count —,
    which is not the host analysis's and never was; with it every record is.)"""
    cfg = E.test_config(wl, seed=31, **CASES[wl])
    classify = wl == "txn-rw-register"
    with E.Engine(cfg) as eng:
        eng.run(0, N)
        eng.check(classify)
        dev = eng.check_results().tobytes()
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(HOST_ROUTE)
        eng.run(0, N)
        eng.check(classify)
        host = eng.check_results().tobytes()
        assert host == dev
        assert eng.kernel_ms()[1] > 0
        assert eng.check_host_rechecks() == (N if wl == "lin-kv" else 0)
        eng.check(classify)
        assert eng.check_results().tobytes() == host
        assert eng.check_host_rechecks() == (N if wl == "lin-kv" else 0)


def _short_call(eng, name, n_out):
    """the C entry of Engine.explain_<name> with arrays that hold n_out histories -> (code, msim_last_error)"""
    lib, k = A.load(), 4
    if name == "lin_kv":
        a, b = np.zeros((max(n_out, 1), k), dtype=E.LIN_KEY_DT), np.zeros(max(n_out, 1), dtype=np.uint32)
        rc = lib.msim_explain_lin_kv(eng._ctx, a.ctypes.data, k, b.ctypes.data, n_out)
    else:
        hdr_dt, rec_dt = {"txn": (E.CYCLE_DT, E.CYCLE_STEP_DT), "set_full": (E.SET_EXPLAIN_DT, E.SET_ELEMENT_DT), "kafka": (E.KAFKA_EXPLAIN_DT, E.KAFKA_FINDING_DT)}[name]
        a, b = np.zeros(max(n_out, 1), dtype=hdr_dt), np.zeros((max(n_out, 1), k), dtype=rec_dt)
        rc = getattr(lib, "msim_explain_" + name)(eng._ctx, a.ctypes.data, b.ctypes.data, k, n_out)
    return rc, lib.msim_last_error(eng._ctx).decode()


@pytest.mark.parametrize("name,wl,kw,not_a", [
    ("lin_kv", "lin-kv", CASES["lin-kv"], "msim_explain_lin_kv: not a lin-kv context"),
    ("txn", "txn-list-append", CASES["txn-list-append"], "msim_explain_txn: not a txn-list-append or txn-rw-register context"),
    ("set_full", "g-set", dict(node_count=5, rate=10, time_limit=10), "msim_explain_set_full: not a broadcast or g-set context"),
    ("kafka", "kafka", CASES["kafka"], "msim_explain_kafka: not a kafka context"),
])
def test_explaining_entries_refuse_alike(lib, name, wl, kw, not_a):
    """another workload's context: MSIM_E_UNSUPPORTED; nothing run yet: MSIM_E_RANGE; arrays one history short: MSIM_E_RANGE — each with
    the entry's own message"""
    explain = "explain_" + name
    with E.Engine(E.test_config("echo", node_count=2, rate=10, time_limit=1, seed=1)) as eng:
        eng.run(0, 2)
        with pytest.raises(E.EngineError, match=re.escape(f"msim_explain_{name} failed (-6): {not_a}")):
            getattr(eng, explain)()
    with E.Engine(E.test_config(wl, seed=31, **kw)) as eng:
        with pytest.raises(E.EngineError, match=re.escape(f"msim_explain_{name} failed (-5): msim_explain_{name} before msim_run")):
            getattr(eng, explain)()
        eng.run(0, 2)
        assert _short_call(eng, name, 1) == (-5, f"msim_explain_{name}: output arrays shorter than the run")
        assert _short_call(eng, name, 2)[0] == 0


def _routes(err):
    return re.findall(r"^\[check\] (queued|taken|launched|explain) (\d+)$", err, re.M)


def test_set_full_explain_takes_a_queued_check_and_leaves_the_context_armed(lib, capfd):
    """run_async, check() (launched: the context arms), run_async (its check queued), explain_set_full: the queued check is taken, the
    records are a plain check()'s of that launch in another context, and the next launch still queues its check for check() to take"""
    cfg = E.test_config("g-set", node_count=5, rate=10, time_limit=10, seed=2)
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(TRACE)
        eng.run_async(0, N)
        eng.check()
        eng.run_async(1000, N)
        assert _routes(capfd.readouterr().err) == [("launched", str(N)), ("queued", str(N))]
        got = eng.explain_set_full(max_elements=16)
        assert _routes(capfd.readouterr().err) == [("taken", str(N)), ("explain", str(N))]
        recs = eng.check_results().tobytes()
        assert b"".join(r.tobytes() for r, _, _ in got) == recs
        eng.run_async(2000, N)
        eng.check()
        assert _routes(capfd.readouterr().err) == [("queued", str(N)), ("taken", str(N))]
    with E.Engine(cfg) as other:
        other.run_async(1000, N)
        other.check()
        assert other.check_results().tobytes() == recs


def _pick(hs, host_records, clean):
    """the first history with rows whose host record is clean (valid, no anomaly named) / is not"""
    for h, rec in zip(hs, host_records):
        rows = h[0] if isinstance(h, tuple) else h
        if len(rows) and (int(rec["valid"]) == 1 and int(rec["error_count"]) == 0) == clean:
            return h
    raise AssertionError("no such history")


def test_kafka_batch_without_findings_wanted_keeps_the_true_counts(lib):
    hs = [KAFKA_HAND[sorted(KAFKA_GOOD)[0]], KAFKA_HAND["poll_skip"], EMPTY]
    want = [kafka_host(h, 0) for h in hs]
    out, hdr, fs, handed = E.explain_kafka_batch(hs, 3, max_findings=0)
    for i, (w_out, w_hdr, _) in enumerate(want):
        assert out[i].tobytes() == w_out.tobytes() and hdr[i].tobytes() == w_hdr.tobytes(), (i, out[i], w_out, hdr[i], w_hdr)
    assert [int(t) for t in hdr["truncated"]] == [0, 1, 0] and [int(c.sum()) > 0 for c in hdr["count"]] == [False, True, False]
    assert not hdr["n_findings"].any() and handed == 0


def test_set_full_batch_without_elements_wanted_keeps_the_true_counts(lib):
    hs = [E.encode_set_history(SX.healthy()), E.encode_set_history(SX.tutorial()), EMPTY]
    want = [set_host(h, 0) for h in hs]
    out, hdr, els = E.explain_set_full_batch(hs, 120, A.WL_G_SET, max_elements=0)
    for i, (w_out, w_hdr, _) in enumerate(want):
        assert out[i].tobytes() == w_out.tobytes() and hdr[i].tobytes() == w_hdr.tobytes(), (i, out[i], w_out, hdr[i], w_hdr)
    assert [int(t) for t in hdr["truncated"]] == [0, 1, 0] and int(out[1]["lost_count"]) + int(out[1]["stale_count"]) + int(out[1]["never_read_count"]) > 0


@pytest.mark.parametrize("rw", [False, True])
def test_cycle_batches_leave_a_clean_historys_record_zero(lib, rw):
    mod = RWT if rw else T
    model = "strict-serializable"
    if rw:   # a write, then a read of it
        clean = E.encode_txn_history(RWT._ops((0, ":ok", [RWT._w(1, 1)], [RWT._w(1, 1)]), (1, ":ok", [[RWT.R, 1, None]], [[RWT.R, 1, 1]])), rw=True)
    else:
        clean = _pick(T.HAND_HS, [txn_host(h, model, 8)[0] for h in T.HAND_HS], True)
    hs = [clean, mod.HAND_HS[list(mod.HAND).index("G1c")], EMPTY]
    want = [txn_host(h, model, 8, rw) for h in hs]
    assert int(want[0][0]["valid"]) == 1 and int(want[0][0]["error_count"]) == 0 and len(hs[0][0])
    out, cycles, steps, _ = (E.explain_rw_batch if rw else E.explain_txn_batch)(hs, model, max_steps=8)
    for i, (w_out, w_cyc, w_steps) in enumerate(want):
        assert out[i].tobytes() == w_out.tobytes() and cycles[i].tobytes() == w_cyc.tobytes() and steps.slab[i].tobytes() == w_steps.tobytes(), (i, out[i], w_out, cycles[i], w_cyc)
    for i in (0, 2):
        assert not cycles[i].tobytes().strip(b"\0") and not steps.slab[i].tobytes().strip(b"\0")
    assert int(cycles[1]["length"]) == 2 == int(cycles[1]["n_steps"])


def test_lin_kv_batch_leaves_a_history_without_rows_no_key_and_a_zero_slab_row(lib):
    hand = [LK.encode(ops) for ops, _ in LK.HAND.values()]
    recs = [E.explain_lin_kv_history(h, 4)[0] for h in hand]
    hs = [_pick(hand, recs, True), _pick(hand, recs, False), NO_ROWS]
    want = [E.explain_lin_kv_history(h, 4) if len(h) else None for h in hs]
    rows, off = E._offsets_form(hs, payload=False)
    out = np.zeros(3, dtype=E.CHECK_DT)
    keys = np.full(3 * 4 * E.LIN_KEY_DT.itemsize // 4, 0xA5A5A5A5, dtype=np.uint32).view(E.LIN_KEY_DT).reshape(3, 4)   # (the entry clears what it does not write)
    nk = np.full(3, 0xA5A5A5A5, dtype=np.uint32)
    n_host = C.c_uint32()
    rc = A.load().msim_explain_lin_kv_batch(0, rows.ctypes.data, off.ctypes.data, 3, out.ctypes.data, keys.ctypes.data, 4, nk.ctypes.data, C.byref(n_host))
    assert rc == 0
    for i in (0, 1):
        w_out, w_keys = want[i]
        assert [int(out[i][f]) for f in LIN_FIELDS] == [int(w_out[f]) for f in LIN_FIELDS] and int(nk[i]) == int(w_out["attempt_count"]) > 0
        assert keys[i, :len(w_keys)].tobytes() == w_keys.tobytes() and not keys[i, len(w_keys):].tobytes().strip(b"\0")
    assert int(nk[2]) == 0 and not keys[2].tobytes().strip(b"\0") and int(out[2]["attempt_count"]) == 0
