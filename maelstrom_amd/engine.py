"""Host-side mirror of the reference's test-map -> history surface, above the C-ABI (include/maelsim.h).

`test_config(...)` plays the role of `maelstrom.core/maelstrom-test` (core.clj:53-102): it takes the CLI
option names of core.clj:136-229 and returns the finalized engine config.  `Engine.run` replaces
`jepsen.core/run!` for an ensemble of instances; `Engine.history(i)` yields the op maps that
`(checker/check (:checker test) test history opts)` consumes (core.clj:91-100), `Engine.net_stats(i)`
the map of net/checker.clj:28-41.  Everything here calls libmaelsim.so; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _abi as A

# The records as numpy dtypes, derived from _abi's Structures (A.RECORDS; tests/test_abi_tables.py holds both to the header).
(OP_DT, STATS_DT, EVENT_DT, CHECK_DT, LIN_KEY_DT, CYCLE_DT, CYCLE_STEP_DT, SET_ELEMENT_DT, SET_EXPLAIN_DT, LATENCY_DT, F_STATS_DT, PERF_DT) = (
    np.dtype(s) for s in (A.Op, A.NetStats, A.Event, A.CheckResult, A.LinKeyResult, A.CycleResult, A.CycleStep, A.SetElement, A.SetExplain,
                          A.LatencyDist, A.FStats, A.PerfResult))
# msim_inst_meta stays written out: its callers know the header's reserved[3] as three words r0, r1, r2 (the oracle's dtype has the same).
KAFKA_FINDING_DT, KAFKA_EXPLAIN_DT = np.dtype(A.KafkaFinding), np.dtype(A.KafkaExplain)   # (A.KAFKA_EXPLAIN_RECORDS)
(PN_READ_DT, PN_RANGE_DT, PN_EXPLAIN_DT, UNIQUE_DUP_DT, UNIQUE_EXPLAIN_DT, ECHO_ERROR_DT, ECHO_EXPLAIN_DT) = (
    np.dtype(s) for s in A.SMALL_EXPLAIN_RECORDS.values())
JOURNAL_MSG_DT, JOURNAL_SUMMARY_DT = (np.dtype(s) for s in A.JOURNAL_RECORDS.values())
TXN_FINDING_DT, TXN_EXPLAIN_DT = (np.dtype(s) for s in A.TXN_FINDINGS_RECORDS.values())
META_DT = np.dtype([(n, "<u4") for n in ("n_rows", "n_payload_words", "flags", "n_rounds", "n_events", "r0", "r1", "r2")])
PERF_QUANTILES = (0, 0.5, 0.95, 0.99, 1)

WORKLOADS = {"echo": A.WL_ECHO, "broadcast": A.WL_BROADCAST, "g-set": A.WL_G_SET, "lin-kv": A.WL_LIN_KV,
             "txn-list-append": A.WL_TXN_LIST_APPEND, "pn-counter": A.WL_PN_COUNTER, "g-counter": A.WL_G_COUNTER, "unique-ids": A.WL_UNIQUE_IDS,
             "txn-rw-register": A.WL_TXN_RW_REGISTER, "kafka": A.WL_KAFKA}
NODE_PROGRAMS = {"echo": A.NODE_ECHO, "broadcast-ff": A.NODE_BCAST_FF, "broadcast-ff-echoback": A.NODE_BCAST_FF_ECHOBACK,
                 "broadcast-ack-retry": A.NODE_BCAST_ACK_RETRY, "broadcast-rpc-all": A.NODE_BCAST_RPC_ALL,
                 "g-set": A.NODE_G_SET, "raft": A.NODE_RAFT, "single-key-txn": A.NODE_TXN_SINGLE_KEY,
                 "pn-counter": A.NODE_PN_COUNTER, "flake-ids": A.NODE_FLAKE_IDS, "lin-kv-proxy": A.NODE_LIN_KV_PROXY,
                 "txn-rw-register-hat": A.NODE_TXN_RW_HAT,
                 "multi-key-txn": A.NODE_TXN_MULTI_KEY, "datomic": A.NODE_TXN_DATOMIC, "tso-ids": A.NODE_TSO_IDS, "kafka": A.NODE_KAFKA,
                 "broadcast-batch": A.NODE_BCAST_BATCH}
SERVICES = {"lin-kv": A.SVC_LIN_KV, "seq-kv": A.SVC_SEQ_KV, "lww-kv": A.SVC_LWW_KV}
CONSISTENCY_MODELS = {"strict-serializable": A.CM_STRICT_SERIALIZABLE, "serializable": A.CM_SERIALIZABLE,
                      "snapshot-isolation": A.CM_SNAPSHOT_ISOLATION, "read-committed": A.CM_READ_COMMITTED,
                      "read-uncommitted": A.CM_READ_UNCOMMITTED}
TOPOLOGIES = {"grid": A.TOPO_GRID, "line": A.TOPO_LINE, "total": A.TOPO_TOTAL, "tree": A.TOPO_TREE2,
              "tree2": A.TOPO_TREE2, "tree3": A.TOPO_TREE3, "tree4": A.TOPO_TREE4}
LATENCY_DISTS = {"constant": A.LAT_CONSTANT, "uniform": A.LAT_UNIFORM, "exponential": A.LAT_EXPONENTIAL}
TYPE_KW = {A.T_INVOKE: ":invoke", A.T_OK: ":ok", A.T_FAIL: ":fail", A.T_INFO: ":info"}
F_KW = {A.F_ECHO: ":echo", A.F_BROADCAST: ":broadcast", A.F_READ: ":read", A.F_ADD: ":add",
        A.F_START_PARTITION: ":start-partition", A.F_STOP_PARTITION: ":stop-partition", A.F_WRITE: ":write", A.F_CAS: ":cas",
        A.F_TXN: ":txn", A.F_GENERATE: ":generate", A.F_SEND: ":send", A.F_POLL: ":poll", A.F_ASSIGN: ":assign", A.F_CRASH: ":crash"}
ERR_KW = {A.ERR_NET_TIMEOUT: ":net-timeout", A.ERR_TEMPORARILY_UNAVAILABLE: [":temporarily-unavailable", "not a leader"],
          A.ERR_KEY_DOES_NOT_EXIST: [":key-does-not-exist", "not found"], A.ERR_PRECONDITION_FAILED: [":precondition-failed", "cas mismatch"],
          A.ERR_TXN_CONFLICT: [":txn-conflict", "root altered"], A.ERR_TIMEOUT: [":timeout", "promise timed out"], A.ERR_ABORT: [":abort", "aborted"]}
SPEC_KW = {A.SPEC_ONE: ":one", A.SPEC_MAJORITY: ":majority", A.SPEC_MAJORITIES_RING: ":majorities-ring",
           A.SPEC_MINORITY_THIRD: ":minority-third"}


class EngineError(RuntimeError):
    pass


def _call(entry, *args):
    """One entry of the library without a context: a code other than MSIM_OK raises "<entry>: <code>" (Engine._chk is its twin with a
    context, whose message carries msim_last_error).  Arrays go in as their addresses (`.ctypes.data`): every entry has its prototype."""
    rc = getattr(A.load(), entry)(*args)
    if rc:
        raise EngineError(f"{entry}: {rc}")


def _concatenated(arrays, dtype):
    off = np.zeros(len(arrays) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return (np.concatenate(arrays) if arrays else np.zeros(0, dtype=dtype)), off


def _offsets_form(histories, payload=True):
    """The "offsets" form of a batch entry's input: the histories' rows concatenated and their n + 1 uint64 row offsets; with `payload`
    (the histories are (rows, payload words) pairs) the same for the payload, where no word at all becomes one zero word.
    -> (rows, row_offsets[, payload, payload_offsets]).  No rows at all stay no rows: explain_lin_kv_batch alone pads them."""
    if not payload:
        return _concatenated([np.ascontiguousarray(h) for h in histories], OP_DT)
    rows, ro = _concatenated([np.ascontiguousarray(h[0]) for h in histories], OP_DT)
    pay, po = _concatenated([np.ascontiguousarray(h[1], dtype=np.uint32) for h in histories], np.uint32)
    return rows, ro, (pay if len(pay) else np.zeros(1, dtype=np.uint32)), po


def _padded(arrays, dtype, width=None):
    width = int(width) if width else max(1, max(len(a) for a in arrays))
    slab = np.zeros((len(arrays), width), dtype=dtype)
    for i, a in enumerate(arrays):
        slab[i, :len(a)] = a
    return slab, np.asarray([len(a) for a in arrays], dtype=np.uint32)


def _slab_form(histories, payload=False, max_rows=None):
    """The "slab" form of a batch entry's input: history i zero-padded in row i of a (histories, max_rows) array, and n_rows; with
    `payload` (the histories are (rows, payload words) pairs) the payload slab likewise.  The widths are the longest history's, at least
    1, so an empty list of histories raises, as max() does (not with `max_rows` given).  -> (rows, n_rows[, payload])."""
    if not payload:
        return _padded([np.ascontiguousarray(h) for h in histories], OP_DT, max_rows)
    rows, nr = _padded([np.ascontiguousarray(r) for r, _ in histories], OP_DT, max_rows)
    return rows, nr, _padded([np.ascontiguousarray(p, dtype=np.uint32) for _, p in histories], np.uint32)[0]


def test_config(workload="broadcast", bin=None, node_count=5, concurrency=None, rate=5.0, time_limit=60.0,
                latency=0, latency_dist="constant", topology="grid", nemesis=(), nemesis_interval=10.0,
                p_loss=0.0, seed=0, **capacities):
    """Option map -> finalized msim_config.  Names follow core.clj:136-229; `bin` names a built-in node
    program (NODE_PROGRAMS) instead of an executable; `p_loss` is the net's :p-loss (net.clj:100,122)."""
    lib = A.load()
    cfg = A.Config()
    _call("msim_config_defaults", C.byref(cfg), WORKLOADS[workload], int(node_count))
    if bin is not None:
        cfg.node_program = NODE_PROGRAMS[bin]
    if concurrency is not None:
        cfg.concurrency = int(concurrency)
    cfg.rate_mhz = int(round(rate * 1000))
    cfg.time_limit_ms = int(round(time_limit * 1000))
    cfg.latency_mean_ms = int(latency)
    cfg.latency_dist = LATENCY_DISTS[latency_dist]
    cfg.topology = TOPOLOGIES[topology]
    cfg.nemesis_mask = A.NEMESIS_PARTITION if "partition" in set(nemesis) else 0
    cfg.nemesis_interval_ms = int(round(nemesis_interval * 1000))
    cfg.p_loss_q32 = min(int(p_loss * 2**32), 2**32 - 1)
    cfg.seed = int(seed)
    for k, v in capacities.items():
        if k == "proxy_service" and isinstance(v, str):
            v = SERVICES[v]
        if k == "consistency_model" and isinstance(v, str):
            v = CONSISTENCY_MODELS[v]
        if not hasattr(cfg, k):
            raise EngineError(f"unknown option {k}")
        setattr(cfg, k, int(v))
    err = C.create_string_buffer(256)
    rc = lib.msim_config_finalize(C.byref(cfg), err, 256)
    if rc:
        raise EngineError(f"invalid test options ({rc}): {err.value.decode()}")
    return cfg


class Engine:
    """One engine context on one HIP device (msim_create ... msim_destroy)."""

    def __init__(self, cfg, device=0):
        self.lib = A.load()
        self._ctx = C.c_void_p()
        err = C.create_string_buffer(256)
        rc = self.lib.msim_create(C.byref(cfg), device, C.byref(self._ctx), err, 256)
        if rc:
            raise EngineError(f"msim_create failed ({rc}): {err.value.decode()}")
        self.cfg = A.Config()
        self.lib.msim_get_config(self._ctx, C.byref(self.cfg))
        self.n = 0

    def _chk(self, rc, what):
        if rc:
            raise EngineError(f"{what} failed ({rc}): {self.lib.msim_last_error(self._ctx).decode()}")

    def close(self):
        if self._ctx:
            self.lib.msim_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, first_instance, n_instances):
        self._chk(self.lib.msim_run(self._ctx, first_instance, n_instances), "msim_run")
        self.n = n_instances

    def run_async(self, first_instance, n_instances, stream=None):
        """msim_run_async: queues the launch and returns.  stream=None is the context's own stream, on which check(), fetch(),
        fetch_begin() and kernel_ms() work: they wait for the launch and may be called at once.  They do not know a caller's stream
        (a hipStream_t as an integer): a caller that passes its own synchronises that stream before it calls any of them.  On a context
        whose launches the caller checks (see check()), a launch on the context's own stream queues the set-full / echo checker behind
        the simulation kernel at once; the slabs of device_buffers() are outputs, and what a caller writes into them is not checked."""
        self._chk(self.lib.msim_run_async(self._ctx, first_instance, n_instances, stream), "msim_run_async")
        self.n = n_instances

    def check(self, classify=False):
        """msim_check.  classify=True (msim_set_check_classify; the two transactional workloads and kafka only).  txn-rw-register: every
        history's record is the full analysis of check_rw_history, its allowed cycle classes named.  txn-list-append: a history that is not
        provably clean is analysed and its cycles classified on the device, not on the host cores (the records are the same).  kafka: a
        history that is not provably clean has its anomalies named on the device, not on the host cores (the records are the same;
        check_host_rechecks() then counts only classify_kafka_batch's hand-overs).  See anomaly_census, kafka_anomaly_census.
        Set-full (broadcast, g-set) and echo: the first check() of a launch on the context's own stream arms the context; its next
        launches queue the checker behind their simulation, and check() only waits for it (check_results() refuses until then).  A
        second check() of the same run launches the kernel again; a run nobody checked disarms the context; developer flag 0x40000
        keeps the checker where check() is called."""
        if classify or getattr(self, "_classify", False):
            self._chk(self.lib.msim_set_check_classify(self._ctx, 1 if classify else 0), "msim_set_check_classify")
            self._classify = bool(classify)
        self._chk(self.lib.msim_check(self._ctx), "msim_check")

    def explain_lin_kv(self, max_keys=256):
        """lin-kv: check() that also explains (msim_explain_lin_kv): per history of the last run (CHECK_DT record — check_results() holds
        the same afterwards —, LIN_KEY_DT records, one per key ascending: Knossos' :op / :previous-ok rows, the :configs' register values
        and the open calls; see lin_kv_analysis), written by the device search at every level it has."""
        keys = np.zeros((self.n, max_keys), dtype=LIN_KEY_DT)
        nk = np.zeros(self.n, dtype=np.uint32)
        self._chk(self.lib.msim_explain_lin_kv(self._ctx, keys.ctypes.data, max_keys, nk.ctypes.data, self.n), "msim_explain_lin_kv")
        res = self.check_results()
        return [(res[i], keys[i, :min(int(nk[i]), max_keys)].copy()) for i in range(self.n)]

    def explain_txn(self, max_steps=64):
        """txn-list-append / txn-rw-register: check(classify=True) that also explains (msim_explain_txn): per history of the last run
        (CHECK_DT record — check_results() holds the same afterwards —, CYCLE_DT record, CYCLE_STEP_DT steps: the witness cycle of the
        record's cycle class as include/maelsim.h defines it; see txn_cycle_analysis), found on the device."""
        cycles = np.zeros(self.n, dtype=CYCLE_DT)
        steps = np.zeros((self.n, max_steps), dtype=CYCLE_STEP_DT)
        self._chk(self.lib.msim_explain_txn(self._ctx, cycles.ctypes.data, steps.ctypes.data, max_steps, self.n), "msim_explain_txn")
        res = self.check_results()
        return [(res[i], cycles[i], steps[i, :int(cycles[i]["n_steps"])].copy()) for i in range(self.n)]

    def explain_txn_findings(self, max_findings=64):
        """txn-list-append / txn-rw-register: check(classify=True) that also explains the NON-CYCLE anomalies (msim_explain_txn_findings):
        per history of the last run (CHECK_DT record — check_results() holds the same afterwards —, TXN_EXPLAIN_DT header,
        TXN_FINDING_DT records: one witness per anomaly in the order include/maelsim_txn_findings.h defines; see txn_findings_analysis),
        found on the device.  A history with more findings than max_findings has header["truncated"] set; header["count"] is always
        the true number per anomaly."""
        hdr = np.zeros(max(self.n, 1), dtype=TXN_EXPLAIN_DT)
        fs = np.zeros((max(self.n, 1), max(max_findings, 1)), dtype=TXN_FINDING_DT)
        self._chk(self.lib.msim_explain_txn_findings(self._ctx, hdr.ctypes.data, fs.ctypes.data, max_findings, self.n), "msim_explain_txn_findings")
        res = self.check_results()
        return [(res[i], hdr[i], fs[i, :int(hdr[i]["n_findings"])].copy()) for i in range(self.n)]

    def explain_set_full(self, max_elements=256):
        """broadcast / g-set: check() that also explains (msim_explain_set_full): per history of the last run (CHECK_DT record —
        check_results() holds the same afterwards —, SET_EXPLAIN_DT header, SET_ELEMENT_DT records: the lost, the never-read and the
        stale elements, in this order, each kind ascending, with the rows of their :known / :last-present / :last-absent ops; see
        set_full_analysis), compacted on the device.  A history with more of them than max_elements has header["truncated"] set."""
        hdr = np.zeros(max(self.n, 1), dtype=SET_EXPLAIN_DT)
        els = np.zeros((max(self.n, 1), max(max_elements, 1)), dtype=SET_ELEMENT_DT)
        self._chk(self.lib.msim_explain_set_full(self._ctx, hdr.ctypes.data, els.ctypes.data, max_elements, self.n), "msim_explain_set_full")
        res = self.check_results()
        return [(res[i], hdr[i], els[i, :_n_set_records(hdr[i])].copy()) for i in range(self.n)]

    def explain_kafka(self, max_findings=64):
        """kafka: check(classify=True) that also explains (msim_explain_kafka): per history of the last run (CHECK_DT record —
        check_results() holds the same afterwards —, KAFKA_EXPLAIN_DT header, KAFKA_FINDING_DT records: one witness per anomaly in the
        order include/maelsim.h defines; see kafka_findings), found on the device.  A history with more findings than max_findings has
        header["truncated"] set; header["count"] is always the true number per anomaly."""
        hdr = np.zeros(max(self.n, 1), dtype=KAFKA_EXPLAIN_DT)
        fs = np.zeros((max(self.n, 1), max(max_findings, 1)), dtype=KAFKA_FINDING_DT)
        self._chk(self.lib.msim_explain_kafka(self._ctx, hdr.ctypes.data, fs.ctypes.data, max_findings, self.n), "msim_explain_kafka")
        res = self.check_results()
        return [(res[i], hdr[i], fs[i, :int(hdr[i]["n_findings"])].copy()) for i in range(self.n)]

    def _explain_small(self, entry, hdr_dt, rec_dt, cap):
        hdr = np.zeros(max(self.n, 1), dtype=hdr_dt)
        recs = np.zeros((max(self.n, 1), max(cap, 1)), dtype=rec_dt)
        self._chk(getattr(self.lib, entry)(self._ctx, hdr.ctypes.data, recs.ctypes.data, cap, self.n), entry)
        return self.check_results(), hdr, recs

    def explain_pn(self, max_records=256):
        """pn-counter / g-counter: check() that also explains (msim_explain_pn): per history of the last run (CHECK_DT record —
        check_results() holds the same afterwards —, PN_EXPLAIN_DT header, PN_READ_DT final reads, PN_RANGE_DT acceptable ranges; see
        pn_analysis), read off the device checker's bitmap.  The reads come first in a history's max_records records; a history with
        more reads and ranges than that has header["truncated"] set."""
        res, hdr, recs = self._explain_small("msim_explain_pn", PN_EXPLAIN_DT, PN_READ_DT, max_records)
        return [(res[i], hdr[i]) + _pn_segments(hdr[i], recs[i]) for i in range(self.n)]

    def explain_unique_ids(self, max_dups=48):
        """unique-ids: check() that also explains (msim_explain_unique): per history of the last run (CHECK_DT record, UNIQUE_EXPLAIN_DT
        header, UNIQUE_DUP_DT records: the duplicated ids by count descending, then id descending, with the rows of their first two
        acknowledgements; see unique_ids_analysis), found on the device."""
        res, hdr, recs = self._explain_small("msim_explain_unique", UNIQUE_EXPLAIN_DT, UNIQUE_DUP_DT, max_dups)
        return [(res[i], hdr[i], recs[i, :int(hdr[i]["n_dups"])].copy()) for i in range(self.n)]

    def explain_echo(self, max_errors=64):
        """echo: check() that also explains (msim_explain_echo): per history of the last run (CHECK_DT record, ECHO_EXPLAIN_DT header,
        ECHO_ERROR_DT records: the invocations the check counts as errors, in row order; see echo_analysis), found on the device."""
        res, hdr, recs = self._explain_small("msim_explain_echo", ECHO_EXPLAIN_DT, ECHO_ERROR_DT, max_errors)
        return [(res[i], hdr[i], recs[i, :int(hdr[i]["n_errors"])].copy()) for i in range(self.n)]

    def journal_messages(self, max_msgs):
        """The net journals of the last run analysed where they lie in HBM (msim_journal_messages; journal_capacity > 0; no fetch needed,
        and behind run_async no wait): per instance (JOURNAL_SUMMARY_DT summary, JOURNAL_MSG_DT records: one per :send in journal order,
        the first max_msgs of them, each with the :recv that delivered it or NO_VALUE; see journal_analysis).  The whole zero-padded
        (instances, max_msgs) slab is the list's `.slab`.  Not a check: check_results() is untouched."""
        summ = np.zeros(max(self.n, 1), dtype=JOURNAL_SUMMARY_DT)
        recs = np.zeros((max(self.n, 1), max(max_msgs, 1)), dtype=JOURNAL_MSG_DT)
        self._chk(self.lib.msim_journal_messages(self._ctx, summ.ctypes.data, recs.ctypes.data if max_msgs else None, max_msgs, self.n), "msim_journal_messages")
        out = _StepLists((summ[i], recs[i, :min(int(summ[i]["n_msgs"]), max_msgs)].copy()) for i in range(self.n))
        out.slab = recs[:, :max_msgs]
        return out

    def set_dev_flags(self, flags):
        """Developer switches of this context (msim_set_dev_flags): e.g. 0x200 one cluster per wavefront, 0x800 checkers on the host."""
        self._chk(self.lib.msim_set_dev_flags(self._ctx, int(flags)), "msim_set_dev_flags")

    def check_host_rechecks(self):
        """lin-kv: how many histories of the last check() the device handed to the host search."""
        return int(self.lib.msim_check_host_rechecks(self._ctx))

    def fetch(self):
        self._chk(self.lib.msim_fetch(self._ctx), "msim_fetch")

    def fetch_begin(self):
        """Compacts the histories on the device and queues their copies to the host; fetch() waits for them (msim_fetch_begin)."""
        self._chk(self.lib.msim_fetch_begin(self._ctx), "msim_fetch_begin")

    def kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        self._chk(self.lib.msim_last_kernel_ms(self._ctx, C.byref(a), C.byref(b)), "msim_last_kernel_ms")
        return a.value, b.value

    def check_availability(self, availability=None):
        """maelstrom.checker/availability-checker (checker.clj:6-39) over every history of the last run: `availability` is None,
        "total" or a number from 0 to 1 (--availability, core.clj:149).  Returns [{:valid? :ok-fraction}] (+ the two counts)."""
        mode, a = _availability_mode(availability)
        res = (A.Availability * self.n)()
        self._chk(self.lib.msim_check_availability(self._ctx, mode, a, res, self.n), "msim_check_availability")
        return [{"valid?": bool(r.valid), "ok-fraction": float(r.ok_fraction), "ok-count": r.ok_count, "invoke-count": r.invoke_count} for r in res]

    def check_perf(self, window_s=None, n_windows=0):
        """[upstream] jepsen.checker/stats with :by-f and the numbers behind jepsen.checker/perf's latency plots (core.clj:92-97) over
        every history of the last run, on the device (msim_check_perf): one record per history as check_perf_rows gives it.  With
        `window_s` and `n_windows` (at most 16) each record also has "windows": the latency records per time window of the invocation."""
        window_ms, n_windows = _perf_windows(window_s, n_windows)
        out = np.zeros(self.n, dtype=PERF_DT)
        win = np.zeros((self.n, n_windows, A.PERF_MAX_F, 3), dtype=LATENCY_DT)
        self._chk(self.lib.msim_check_perf(self._ctx, window_ms, n_windows, out.ctypes.data, self.n, win.ctypes.data if n_windows else None), "msim_check_perf")
        return [decode_perf(out[i], win[i] if n_windows else None) for i in range(self.n)]

    # ---- multi-GPU ensemble (include/maelsim.h "multi-GPU ensemble"; maelstrom_amd/ensemble.py) ----
    @staticmethod
    def comm_unique_id():
        """rank 0: the 128-byte RCCL id every rank passes to comm_init (the host moves it: torch.distributed, files, sockets)"""
        buf = C.create_string_buffer(A.COMM_ID_BYTES)
        rc = A.load().msim_comm_unique_id(buf)
        if rc:
            raise EngineError(f"msim_comm_unique_id failed ({rc}): RCCL not available")
        return buf.raw

    def comm_init(self, comm_id, rank, world):
        self._chk(self.lib.msim_comm_init(self._ctx, bytes(comm_id), rank, world), "msim_comm_init")

    def gather(self, root=0):
        """Variable-length history gather of the last run to `root` (device-side compaction + RCCL send/recv); returns the
        msim_gathered record (device pointers are valid on the root until the next gather)."""
        g = A.Gathered()
        self._chk(self.lib.msim_gather(self._ctx, root, C.byref(g)), "msim_gather")
        return g

    def device_buffers(self):
        db = A.DeviceBuffers()
        self._chk(self.lib.msim_device_buffers_get(self._ctx, C.byref(db)), "msim_device_buffers_get")
        return db

    def raw_history(self, i):
        """(rows, payload) numpy views of instance i (after fetch)."""
        ops, n_ops = C.POINTER(A.Op)(), C.c_uint32()
        pay, n_words = C.POINTER(C.c_uint32)(), C.c_uint32()
        self._chk(self.lib.msim_history(self._ctx, i, C.byref(ops), C.byref(n_ops), C.byref(pay), C.byref(n_words)), "msim_history")
        rows = np.ctypeslib.as_array(C.cast(ops, C.POINTER(C.c_uint8)), shape=(max(n_ops.value, 1) * 16,))[: n_ops.value * 16].view(OP_DT)
        payload = np.ctypeslib.as_array(pay, shape=(max(n_words.value, 1),))[: n_words.value]
        return rows, payload

    def raw_journal(self, i):
        """numpy view of instance i's net journal (journal_capacity > 0, after fetch)."""
        ev, n = C.POINTER(A.Event)(), C.c_uint32()
        self._chk(self.lib.msim_journal(self._ctx, i, C.byref(ev), C.byref(n)), "msim_journal")
        return np.ctypeslib.as_array(C.cast(ev, C.POINTER(C.c_uint8)), shape=(max(n.value, 1) * 16,))[: n.value * 16].view(EVENT_DT)

    def journal(self, i):
        return decode_journal(self.raw_journal(i), self.cfg.n_nodes)

    def net_stats_raw(self, i):
        st = A.NetStats()
        self._chk(self.lib.msim_net_stats_get(self._ctx, i, C.byref(st)), "msim_net_stats_get")
        return st

    def meta(self, i):
        m = A.InstMeta()
        self._chk(self.lib.msim_meta(self._ctx, i, C.byref(m)), "msim_meta")
        return m

    def check_results(self):
        res, n = C.POINTER(A.CheckResult)(), C.c_uint32()
        self._chk(self.lib.msim_check_results(self._ctx, C.byref(res), C.byref(n)), "msim_check_results")
        arr = np.ctypeslib.as_array(C.cast(res, C.POINTER(C.c_uint8)), shape=(n.value * C.sizeof(A.CheckResult),))
        return arr.view(CHECK_DT).copy()  # small; a copy outlives the ctx

    # ---- Jepsen-shaped views ---------------------------------------------------------------------
    def history(self, i):
        rows, payload = self.raw_history(i)
        return decode_history(rows, payload, self.cfg.n_nodes, self.cfg.workload)

    def net_stats(self, i):
        """The :net :stats map of net/checker.clj:28-41,55-67."""
        st = self.net_stats_raw(i)
        rows, _ = self.raw_history(i)
        return net_stats_map(st, rows)


def net_stats_map(st, rows):
    typ = rows["packed"] & 3
    proc = rows["packed"] >> 12
    op_count = int(((typ == A.T_INVOKE) & (proc != A.PROCESS_NEMESIS)).sum())
    get = (lambda k: int(st[k])) if isinstance(st, (np.void, dict)) else (lambda k: int(getattr(st, k)))
    m = {k: {"send-count": get(f"{k}_send"), "recv-count": get(f"{k}_recv"), "msg-count": get(f"{k}_send")}
         for k in ("all", "clients", "servers")}
    if op_count:
        m["all"]["msgs-per-op"] = m["all"]["msg-count"] / op_count
        m["servers"]["msgs-per-op"] = m["servers"]["msg-count"] / op_count
    m["valid?"] = True
    return m


def endpoint_name(ep, n_nodes):
    return f"n{ep}" if ep < n_nodes else f"c{ep - n_nodes}"


def decode_journal(events, n_nodes):
    """Binary events -> the Event maps of net/journal.clj:53 ({:id :time :type :message {:id :src :dest :body}})."""
    out = []
    for i in range(len(events)):
        msg, route = int(events["msg"][i]), int(events["route"][i])
        body = {"type": A.MSG_TYPES[msg & 0x7F], "a": int(events["a"][i])}
        if route >> 16:
            body["msg_id/in_reply_to"] = route >> 16
        out.append({"id": i, "time": int(events["time_us"][i]) * 1000, "type": ":recv" if msg & 0x80 else ":send",
                    "message": {"id": msg >> 8, "src": endpoint_name(route & 0xFF, n_nodes),
                                "dest": endpoint_name((route >> 8) & 0xFF, n_nodes), "body": body}})
    return out


def journal_stats(events, n_nodes):
    """maelstrom.net.checker's fold over the journal (net/checker.clj:28-41): send/recv/msg counts for all,
    clients (a client endpoint involved, util.clj:12-16) and servers.  Every endpoint >= n_nodes counts as a client here, the service
    endpoints behind the client slots (lin-kv, lww-kv, lin-tso) too, which the reference counts as servers: journal_messages_history /
    journal_analysis draw the classes by the client slots and do not."""
    msg, route = events["msg"], events["route"]
    recv = (msg & 0x80) != 0
    cl = ((route & 0xFF) >= n_nodes) | (((route >> 8) & 0xFF) >= n_nodes)
    ids = msg >> 8
    res = {}
    for name, sel in (("all", np.ones(len(events), bool)), ("clients", cl), ("servers", ~cl)):
        res[name] = {"send-count": int((sel & ~recv).sum()), "recv-count": int((sel & recv).sum()),
                     "msg-count": int(len(np.unique(ids[sel])))}
    return res


def journal_messages_history(events, n_nodes, client_slots, max_msgs=None):
    """One journal's messages on the host (msim_journal_messages_rows; needs no device; exact for every journal): every :send joined
    to its :recv -> (JOURNAL_SUMMARY_DT summary, JOURNAL_MSG_DT records, one per :send in journal order: the first max_msgs; None: all).
    include/maelsim_journal.h is the contract.  client_slots: max(concurrency, n_nodes) for an engine's journal."""
    events = np.ascontiguousarray(events)
    cap = len(events) if max_msgs is None else int(max_msgs)
    summ = np.zeros(1, dtype=JOURNAL_SUMMARY_DT)
    recs = np.zeros(max(cap, 1), dtype=JOURNAL_MSG_DT)
    _call("msim_journal_messages_rows", events.ctypes.data, len(events), n_nodes, client_slots, summ.ctypes.data, recs.ctypes.data if cap else None, cap)
    return summ[0], recs[:min(int(summ[0]["n_msgs"]), cap)]


def journal_messages_batch(journals, n_nodes, client_slots, max_msgs, device=0, with_n_host=False):
    """journal_messages_history over many journals in one device batch (msim_journal_messages_batch).  Returns (JOURNAL_SUMMARY_DT
    summaries, a list of JOURNAL_MSG_DT arrays); the whole zero-padded (journals, max_msgs) slab is the list's `.slab`.  with_n_host:
    also how many journals the host walk did instead — exactly those that are not well-formed."""
    ev, off = _concatenated([np.ascontiguousarray(j) for j in journals], EVENT_DT)
    n = len(journals)
    summ = np.zeros(n, dtype=JOURNAL_SUMMARY_DT)
    recs = np.zeros((n, max(max_msgs, 1)), dtype=JOURNAL_MSG_DT)
    n_host = C.c_uint32()
    _call("msim_journal_messages_batch", device, ev.ctypes.data if len(ev) else None, off.ctypes.data, n, n_nodes, client_slots, summ.ctypes.data,
          recs.ctypes.data if max_msgs else None, max_msgs, C.addressof(n_host))
    msgs = _StepLists(recs[i, :min(int(summ[i]["n_msgs"]), max_msgs)].copy() for i in range(n))
    msgs.slab = recs[:, :max_msgs]
    return (summ, msgs, n_host.value) if with_n_host else (summ, msgs)


def journal_analysis(summary, msgs=None, service_names=None):
    """The :net :stats map of net/checker.clj:28-41 from one journal's summary ({"all" / "clients" / "servers": {"send-count",
    "recv-count", "msg-count"}}; pure formatting), plus "delivery": the undelivered messages and the latency quantiles per class, the
    counts that make a journal malformed, the endpoints that occur in sort-clients order (util.clj:18-28: c0 c1 .. n0 n1 .. and the
    services last, by name — `service_names` names the endpoints behind the client slots in order, else "service<k>").  With `msgs`,
    "undelivered-ids" lists the ids of the records without a :recv."""
    res = {name: {"send-count": int(summary["send_count"][k]), "recv-count": int(summary["recv_count"][k]), "msg-count": int(summary["msg_count"][k])}
           for k, name in enumerate(("all", "clients", "servers"))}
    n_nodes, slots = int(summary["n_nodes"]), int(summary["client_slots"])
    eps = [e for e in range(256) if int(summary["endpoints"][e >> 5]) >> (e & 31) & 1]
    svc = lambda e: service_names[e - n_nodes - slots] if service_names and e - n_nodes - slots < len(service_names) else f"service{e - n_nodes - slots}"
    names = ([f"c{e - n_nodes}" for e in eps if n_nodes <= e < n_nodes + slots] + [f"n{e}" for e in eps if e < n_nodes]
             + sorted(svc(e) for e in eps if e >= n_nodes + slots))
    lat = {name: {"count": int(d["count"]), "sum-us": int(d["sum_us"]), "quantiles-us": {q: int(v) for q, v in zip(PERF_QUANTILES, d["q_us"])}}
           for name, d in zip(("clients", "servers"), summary["latency"])}
    res["delivery"] = {"undelivered": {name: int(summary["undelivered"][k]) for k, name in enumerate(("all", "clients", "servers"))},
                       "latency": lat, "dup-sends": int(summary["dup_sends"]), "orphan-recvs": int(summary["orphan_recvs"]),
                       "extra-recvs": int(summary["extra_recvs"]), "endpoints": names,
                       "truncated": bool(int(summary["flags"]) & A.JOURNAL_TRUNCATED), "table-truncated": bool(int(summary["flags"]) & A.JOURNAL_TABLE_TRUNCATED)}
    if msgs is not None:
        res["delivery"]["undelivered-ids"] = [int(m["id"]) for m in msgs if int(m["recv_event"]) == A.NO_VALUE]
    res["valid?"] = bool(int(summary["valid"]) == 1)
    return res


def bitmap_to_list(words):
    out = []
    for wi, w in enumerate(np.asarray(words, dtype=np.uint32)):
        w = int(w)
        while w:
            b = w & -w
            out.append(wi * 32 + b.bit_length() - 1)
            w ^= b
    return out


def _nil(x):
    return None if x == 0xFF else x


def decode_rw_txn(words):
    """Payload words of one rw-register transaction -> [[f k v] ...] (txn_rw_register.clj:82-84): one word per micro-op."""
    return [[":w" if w & 1 else ":r", (w >> 1) & 0x7FFF, None if (w >> 16) & 0xFF == 0xFF else (w >> 16) & 0xFF] for w in (int(x) for x in words)]


def encode_rw_txn(txn):
    """[[f k v] ...] -> payload words (inverse of decode_rw_txn)."""
    return [(1 if f == ":w" else 0) | (k << 1) | ((0xFF if v is None else v) << 16) for f, k, v in txn]


def decode_poll(words):
    """The poll_ok block of a kafka :poll -> {key [[offset msg] ...]} (include/maelsim.h msim_op)."""
    out, i, words = {}, 0, [int(w) for w in words]
    while i < len(words):
        h = words[i]; i += 1
        key, n, o = h & 7, (h >> 8) & 0xFF, h >> 16
        msgs = []
        for e in range(n):
            msgs.append([o + e, (words[i + e // 2] >> (16 * (e % 2))) & 0xFFFF])
        i += (n + 1) // 2
        out.setdefault(str(key), []).extend(msgs)   # (a key's pairs that do not continue a run are a block of their own)
    return out


def _kafka_range(i, key, msg, offset):
    """The binary layout's fields (include/maelsim.h: keys 0..7, message values and offsets below 2047): out-of-range values are an
    error, never masked — a masked key or a count that spills into the offset bits would be CHECKED as a different history."""
    if not (0 <= int(key) < 8 and 0 <= int(msg) < 2047 and 0 <= int(offset) < 2047):
        raise EngineError(f"kafka op {i}: key {key} / message {msg} / offset {offset} outside the binary layout (keys 0..7, messages and offsets below 2047)")


def encode_kafka_history(ops):
    """Jepsen-shaped kafka ops ({type, process, f, value[, time]}; values as decode_history gives them) -> (rows, payload) in the engine's
    binary layout, so that externally produced histories can be fed to msim_check_kafka_rows."""
    tkw = {v: k for k, v in TYPE_KW.items()}
    fkw = {":send": A.F_SEND, ":poll": A.F_POLL, ":assign": A.F_ASSIGN, ":crash": A.F_CRASH}
    rows = np.zeros(len(ops), dtype=OP_DT)
    pay = []
    for i, op in enumerate(ops):
        typ, f, process = tkw[op["type"]], fkw[op["f"]], A.PROCESS_NEMESIS if op["process"] == ":nemesis" else int(op["process"])
        value, ln = A.NO_VALUE, 0
        if f == A.F_SEND:
            _, k, v = op["value"][0]
            msg, off = (v[1], v[0]) if isinstance(v, (list, tuple)) else (v, 0x7FF)
            _kafka_range(i, k, msg, off if isinstance(v, (list, tuple)) else 0)
            value = int(k) | (msg << 6) | (off << 17)
        elif f == A.F_POLL and typ == A.T_OK and len(op["value"][0]) > 1:
            value = len(pay)
            for k, pairs in op["value"][0][1].items():
                runs = []
                for o, m in pairs:   # runs of consecutive offsets, at most 255 messages each (the header's count has 8 bits)
                    _kafka_range(i, k, m, o)
                    if runs and runs[-1][0] + len(runs[-1][1]) == o and len(runs[-1][1]) < 255:
                        runs[-1][1].append(m)
                    else:
                        runs.append((o, [m]))
                if not pairs:
                    _kafka_range(i, k, 0, 0)
                for o, ms in runs or [(0, [])]:
                    pay.append(int(k) | (len(ms) << 8) | (o << 16))
                    for e in range(0, len(ms), 2):
                        pay.append(ms[e] | ((ms[e + 1] << 16) if e + 1 < len(ms) else 0))
            ln = len(pay) - value
            if ln == 0:
                value = A.NO_VALUE
        elif f == A.F_ASSIGN:
            value, ln = len(pay), len(op["value"])
            for k in op["value"]:
                _kafka_range(i, k, 0, 0)
            pay.extend(int(k) | (0x80000000 if op.get("seek-to-beginning?") else 0) for k in op["value"])
        rows[i] = (int(op.get("time", i * 1000)) | (ln << 48), typ | (f << 2) | (process << 12), value)
    return rows, np.asarray(pay if pay else [0], dtype=np.uint32)


def check_kafka_history(rows, payload):
    """The kafka checker (msim_check_kafka_rows) on one history -> dict."""
    res = A.CheckResult()
    rows = np.ascontiguousarray(rows); payload = np.ascontiguousarray(payload, dtype=np.uint32)
    _call("msim_check_kafka_rows", rows.ctypes.data, len(rows), payload.ctypes.data, len(payload), C.byref(res))
    return {"valid?": {1: True, 0: False, 2: "unknown"}[res.valid], "anomalies": sorted(n for b, n in A.KAFKA_ANOMALIES.items() if res.error_count & b),
            "send-count": res.attempt_count, "acked-count": res.stable_count, "lost-count": res.lost_count, "unobserved-count": res.never_read_count,
            "duplicate-count": res.duplicated_count, "ok-count": res.ok_count, "fail-count": res.fail_count, "info-count": res.info_count}


def decode_txn(words):
    """Payload words of one transaction -> [[f k v] ...] (txn_list_append.clj:27-39; encoding: include/maelsim.h msim_op)."""
    out, i, words = [], 0, [int(w) for w in words]
    while i < len(words):
        w = words[i]; i += 1
        key, x = (w >> 1) & 0x7FFF, (w >> 16) & 0xFF
        if w & 1:
            out.append([":append", key, x])
        elif x == 0xFF:
            out.append([":r", key, None])
        else:
            nw = (x + 3) // 4
            out.append([":r", key, [(words[i + e // 4] >> (8 * (e % 4))) & 0xFF for e in range(x)]])
            i += nw
    return out


def encode_txn(txn):
    """[[f k v] ...] -> payload words (inverse of decode_txn)."""
    words = []
    for f, k, v in txn:
        if f == ":append":
            words.append(1 | (k << 1) | (v << 16))
        elif v is None:
            words.append((k << 1) | (0xFF << 16))
        else:
            words.append((k << 1) | (len(v) << 16))
            for i in range(0, len(v), 4):
                words.append(sum(x << (8 * j) for j, x in enumerate(v[i:i + 4])))
    return words


def encode_txn_history(ops, rw=False):
    """Jepsen-shaped txn ops ({type, process, value[, time]}) -> (rows, payload) in the engine's binary layout, so that
    externally produced list-append (rw=True: rw-register) histories can be fed to msim_check_txn_rows / msim_check_rw_rows."""
    tkw = {v: k for k, v in TYPE_KW.items()}
    rows = np.zeros(len(ops), dtype=OP_DT)
    payload = []
    for i, op in enumerate(ops):
        w = encode_rw_txn(op["value"]) if rw else encode_txn(op["value"])
        rows["time_len"][i] = int(op.get("time", i * 1000)) | (len(w) << 48)
        rows["packed"][i] = tkw[op["type"]] | (A.F_TXN << 2) | (int(op["process"]) << 12)
        rows["value"][i] = len(payload)
        payload.extend(w)
    return rows, np.asarray(payload, dtype=np.uint32)


def _check_txn_rows(entry, rows, payload, *model):
    res = A.CheckResult()
    rows = np.ascontiguousarray(rows); payload = np.ascontiguousarray(payload, dtype=np.uint32)
    _call(entry, rows.ctypes.data, len(rows), payload.ctypes.data, len(payload), *model, C.byref(res))
    return {"valid?": {1: True, 0: False, 2: "unknown"}[res.valid], "anomalies": sorted(n for b, n in A.ANOMALIES.items() if res.error_count & b),
            "txn-count": res.attempt_count, "ok-count": res.ok_count, "fail-count": res.fail_count, "info-count": res.info_count,
            "edge-count": res.lost_count, "cycle-txns": res.stale_count, "anomaly-bits": res.error_count}


def check_txn_history(rows, payload):
    """The host list-append checker (msim_check_txn_rows) on one history -> dict with :valid? and the anomaly names."""
    return _check_txn_rows("msim_check_txn_rows", rows, payload)


def check_rw_history(rows, payload, consistency_model="strict-serializable"):
    """The host rw-register checker (msim_check_rw_rows) on one history -> dict like check_txn_history."""
    return _check_txn_rows("msim_check_rw_rows", rows, payload, CONSISTENCY_MODELS[consistency_model])


def check_pn_history(rows):
    """The host pn-counter checker (msim_check_pn_rows) on one history -> the reference's result map (pn_counter.clj:120-123
    minus the op maps of :errors)."""
    res = A.CheckResult()
    rows = np.ascontiguousarray(rows)
    ranges = (C.c_int64 * 512)()
    n = C.c_uint32()
    _call("msim_check_pn_rows", rows.ctypes.data, len(rows), C.byref(res), ranges, 256, C.byref(n))
    finals = [int(np.int32(np.uint32(v))) for v, p in zip(rows["value"], rows["packed"]) if (p >> 11) & 1 and (p & 3) == A.T_OK and (p >> 12) != A.PROCESS_NEMESIS]
    return {"valid?": bool(res.valid), "error-count": res.error_count, "final-reads": finals,
            "acceptable": [[ranges[2 * i], ranges[2 * i + 1]] for i in range(min(n.value, 256))]}


def encode_pn_history(ops):
    """Jepsen-shaped pn-counter ops ({type, f, value[, final?, process]}) -> rows, for msim_check_pn_rows."""
    tkw = {v: k for k, v in TYPE_KW.items()}
    rows = np.zeros(len(ops), dtype=OP_DT)
    for i, op in enumerate(ops):
        rows["time_len"][i] = i * 1000
        v = op.get("value")
        rows["value"][i] = 0xFFFFFFFF if v is None else (int(v) & 0xFFFFFFFF)
        f = A.F_ADD if op["f"] == ":add" else A.F_READ
        rows["packed"][i] = tkw[op["type"]] | (f << 2) | ((1 if op.get("final?") else 0) << 11) | (int(op.get("process", 0)) << 12)
    return rows


def encode_set_history(ops):
    """Jepsen-shaped broadcast / g-set ops ({type, process, f, value[, time, final?]}: :broadcast / :add carry the element, a read's :ok
    the list of elements) -> (rows, payload) in the engine's binary layout (include/maelsim.h msim_op: a read result is a bitmap in the
    payload area), so that externally produced histories can be fed to msim_check_set_full_batch.  Inverse of decode_history."""
    tkw = {v: k for k, v in TYPE_KW.items()}
    fkw = {":broadcast": A.F_BROADCAST, ":add": A.F_ADD, ":read": A.F_READ}
    rows = np.zeros(len(ops), dtype=OP_DT)
    pay = []
    for i, op in enumerate(ops):
        typ, f, process = tkw[op["type"]], fkw[op["f"]], int(op["process"])
        value, ln = A.NO_VALUE, 0
        if f != A.F_READ:
            value = int(op["value"])
            if not 0 <= value < 65536:
                raise EngineError(f"op {i}: element {value} outside the binary layout (0..65535)")
        elif typ == A.T_OK:
            els = [int(x) for x in op["value"]]
            if len(set(els)) != len(els):
                raise EngineError(f"op {i}: a read holding an element twice has no bitmap form")
            ln = (max(els) // 32 + 1) if els else 0
            value = len(pay)
            words = [0] * ln
            for x in els:
                words[x // 32] |= 1 << (x % 32)
            pay.extend(words)
        rows[i] = (int(op.get("time", i * 1000)) | (ln << 48), typ | (f << 2) | ((1 if op.get("final?") else 0) << 11) | (process << 12), value)
    return rows, np.asarray(pay if pay else [0], dtype=np.uint32)


def encode_lin_kv_history(ops):
    """Jepsen-shaped lin-kv ops ({type, process, f, value = [k v] / [k [v v']][, time]}; lin_kv.clj:53-67) -> rows for
    msim_check_lin_kv_rows / msim_check_lin_kv_batch.  Keys and values below 255 (nil = 255 in the binary layout)."""
    tkw = {v: k for k, v in TYPE_KW.items()}
    fkw = {":read": A.F_READ, ":write": A.F_WRITE, ":cas": A.F_CAS}
    rows = np.zeros(len(ops), dtype=OP_DT)
    for i, op in enumerate(ops):
        k, v = op["value"]
        v1, v2 = (v if op["f"] == ":cas" else (v, None))
        for x in (k, v1, v2):
            if x is not None and not 0 <= int(x) < 255:
                raise EngineError(f"op {i}: key / value {x} outside the binary layout (0..254)")
        value = int(k) | ((0xFF if v1 is None else int(v1)) << 8) | ((0xFF if v2 is None else int(v2)) << 16)
        rows[i] = (int(op.get("time", i * 1000)), tkw[op["type"]] | (fkw[op["f"]] << 2) | (int(op["process"]) << 12), value)
    return rows


def check_lin_kv_history(rows):
    """The per-key linearizability check (msim_check_lin_kv_rows, host search) on one history -> dict."""
    res = A.CheckResult()
    rows = np.ascontiguousarray(rows)
    _call("msim_check_lin_kv_rows", rows.ctypes.data, len(rows), C.byref(res))
    return {"valid?": {1: True, 0: False, 2: "unknown"}[res.valid], "key-count": res.attempt_count, "invalid-keys": res.error_count}


def decode_history(rows, payload, n_nodes, workload=A.WL_BROADCAST, node_program=None):
    """Binary rows -> list of Jepsen op maps (SURVEY.md §8b 'History surface').  `node_program` matters for unique-ids only (what an id is)."""
    ops = []
    for idx in range(len(rows)):
        tl, packed, value = int(rows["time_len"][idx]), int(rows["packed"][idx]), int(rows["value"][idx])
        typ, f, err = packed & 3, (packed >> 2) & 31, (packed >> 7) & 15
        final, process, ln = (packed >> 11) & 1, packed >> 12, tl >> 48
        op = {"index": idx, "time": tl & 0xFFFFFFFFFFFF, "type": TYPE_KW[typ], "f": F_KW.get(f, f),
              "process": ":nemesis" if process == A.PROCESS_NEMESIS else process}
        if workload == A.WL_LIN_KV and f in (A.F_READ, A.F_WRITE, A.F_CAS):  # independent tuples, lin_kv.clj:53-67
            k, v1, v2 = value & 0xFF, _nil((value >> 8) & 0xFF), _nil((value >> 16) & 0xFF)
            op["value"] = [k, [v1, v2]] if f == A.F_CAS else [k, v1]
        elif f == A.F_GENERATE and node_program == A.NODE_TSO_IDS:   # a lin-tso timestamp (service.clj:121-123)
            op["value"] = value if typ == A.T_OK else None
        elif f == A.F_GENERATE:   # flake id [time count node-id], flake_ids.clj:30-31
            op["value"] = [value >> 20, (value >> 5) & 0x7FFF, f"n{value & 31}"] if typ == A.T_OK else None
        elif f == A.F_SEND:   # [[:send k msg]] / [[:send k [offset msg]]], workload/kafka.clj:188-190
            k, msg, off = value & 63, (value >> 6) & 0x7FF, value >> 17
            op["value"] = [[":send", str(k), msg if off == 0x7FF else [off, msg]]]
        elif f == A.F_POLL:   # [[:poll]] / [[:poll {k [[offset msg] ...]}]], :171-186 (keys are strings, :247-283)
            op["value"] = [[":poll", decode_poll(payload[value:value + ln])]] if typ == A.T_OK else [[":poll"]]
            if typ != A.T_OK and ln:
                op["offsets"] = {str(int(w) & 7): int(w) >> 8 for w in payload[value:value + ln]}   # engine abstraction: what the client asked with
        elif f == A.F_ASSIGN:
            ws = [int(w) for w in payload[value:value + ln]]
            op["value"] = [str(w & 7) for w in ws]
            if ws and ws[0] >> 31:
                op["seek-to-beginning?"] = True
        elif f == A.F_CRASH:
            op["value"] = None
        elif f == A.F_TXN:
            op["value"] = (decode_rw_txn if workload == A.WL_TXN_RW_REGISTER else decode_txn)(payload[value:value + ln])
        elif workload in (A.WL_PN_COUNTER, A.WL_G_COUNTER) and f in (A.F_ADD, A.F_READ):  # pn_counter.clj:22-58: signed delta / counter value
            signed = value - (1 << 32) if value & 0x80000000 else value
            op["value"] = signed if (f == A.F_ADD or typ == A.T_OK) else None
        elif f == A.F_READ:
            op["value"] = bitmap_to_list(payload[value:value + ln]) if typ == A.T_OK else None
        elif f == A.F_ECHO:
            v = f"Please echo {value}"
            op["value"] = {"type": "echo_ok", "echo": v} if typ == A.T_OK else v
        elif f == A.F_START_PARTITION:
            if ln:
                g = payload[value:value + ln].reshape(n_nodes, A.MASK_WORDS)
                op["value"] = [":isolated", {f"n{d}": [f"n{s}" for s in bitmap_to_list(g[d])] for d in range(n_nodes) if g[d].any()}]
            else:
                op["value"] = SPEC_KW[value]
        elif f == A.F_STOP_PARTITION:
            op["value"] = None if idx == 0 or int(rows["packed"][idx - 1]) != packed or False else ":network-healed"
        else:
            op["value"] = None if value == A.NO_VALUE else value
        if err in ERR_KW:
            op["error"] = ERR_KW[err]
        if final:
            op["final?"] = True
        ops.append(op)
    return ops


def _availability_mode(availability):
    if availability is None:
        return A.AVAIL_NIL, 0.0
    if availability in ("total", ":total"):
        return A.AVAIL_TOTAL, 0.0
    if isinstance(availability, (int, float)) and not isinstance(availability, bool):
        return A.AVAIL_FRACTION, float(availability)
    raise EngineError(f"Don't know how to handle :availability {availability!r}")   # checker.clj:36-39


def check_availability_rows(rows, availability=None):
    """The availability checker for one history on the host (msim_check_availability_rows)."""
    mode, a = _availability_mode(availability)
    r = A.Availability()
    rows = np.ascontiguousarray(rows)
    _call("msim_check_availability_rows", rows.ctypes.data, len(rows), mode, a, C.byref(r))
    return {"valid?": bool(r.valid), "ok-fraction": float(r.ok_fraction), "ok-count": r.ok_count, "invoke-count": r.invoke_count}


def _perf_windows(window_s, n_windows):
    n_windows = int(n_windows)
    if n_windows < 0 or n_windows > A.PERF_MAX_WINDOWS:
        raise EngineError(f"n_windows must be 0..{A.PERF_MAX_WINDOWS}")
    if not n_windows:
        return 0, 0
    window_ms = int(round((window_s or 0) * 1000))
    if window_ms <= 0 or window_ms >= 2**32:
        raise EngineError("windows need a window_s of at least one millisecond")
    return window_ms, n_windows


def _decode_latency(d):
    return {"count": int(d["count"]), "sum-us": int(d["sum_us"]), "quantiles-us": {q: int(v) for q, v in zip(PERF_QUANTILES, d["q_us"])}}


def decode_perf(rec, windows=None):
    """One msim_perf_result (a PERF_DT record; `windows` its [n_windows][slot][type] latency records) as maps: the :stats fields,
    "open-count", "complete?" (False: more than four distinct :f, "by-f" holds the four lowest), per :f the counts, "unpaired" and
    "latency" by completion type; "windows" = per window {:f {type latency}}."""
    names = [F_KW.get(int(rec["by_f"][k]["f"]), int(rec["by_f"][k]["f"])) for k in range(int(rec["n_f"]))]
    out = {"valid?": bool(rec["valid"]), "count": int(rec["count"]), "ok-count": int(rec["ok_count"]), "fail-count": int(rec["fail_count"]),
           "info-count": int(rec["info_count"]), "open-count": int(rec["open_count"]), "complete?": not (int(rec["flags"]) & 1), "by-f": {}}
    for k, name in enumerate(names):
        fs = rec["by_f"][k]
        out["by-f"][name] = {"valid?": bool(fs["valid"]), "count": int(fs["count"]), "ok-count": int(fs["ok_count"]), "fail-count": int(fs["fail_count"]),
                             "info-count": int(fs["info_count"]), "unpaired": int(fs["unpaired"]),
                             "latency": {TYPE_KW[t + 1]: _decode_latency(fs["latency"][t]) for t in range(3)}}
    if windows is not None:
        out["windows"] = [{name: {TYPE_KW[t + 1]: _decode_latency(w[k][t]) for t in range(3)} for k, name in enumerate(names)} for w in windows]
    return out


def stats_map(record):
    """The reference's :stats map (doc/02-echo/index.md:369-378) of a check_perf / check_perf_rows record."""
    keys = ("valid?", "count", "ok-count", "fail-count", "info-count")
    m = {k: record[k] for k in keys}
    m["by-f"] = {f: {k: fs[k] for k in keys} for f, fs in record["by-f"].items()}
    return m


def perf_census(records):
    """An ensemble's per-history records (Engine.check_perf) pooled on the host, next to anomaly_census: per (:f, completion type) that
    occurs, how many histories have it, the total count, the mean latency in us (sum of sum-us / total count) and the min, median and
    max over those histories of each quantile."""
    pools = {}
    for rec in records:
        for f, fs in rec["by-f"].items():
            for typ, d in fs["latency"].items():
                if d["count"]:
                    pools.setdefault((f, typ), []).append(d)
    census = {}
    for key, ds in sorted(pools.items()):
        count = sum(d["count"] for d in ds)
        census[key] = {"histories": len(ds), "count": count, "mean-us": sum(d["sum-us"] for d in ds) / count,
                       "quantiles-us": {q: {"min": int(min(v)), "median": float(np.median(v)), "max": int(max(v))}
                                        for q in PERF_QUANTILES for v in [[d["quantiles-us"][q] for d in ds]]}}
    return census


def check_perf_rows(rows, concurrency, window_s=None, n_windows=0):
    """:stats / :perf of one history on the host (msim_check_perf_rows): the record Engine.check_perf gives per history."""
    window_ms, n_windows = _perf_windows(window_s, n_windows)
    rows = np.ascontiguousarray(rows)
    out = np.zeros(1, dtype=PERF_DT)
    win = np.zeros((n_windows, A.PERF_MAX_F, 3), dtype=LATENCY_DT)
    _call("msim_check_perf_rows", rows.ctypes.data if len(rows) else None, len(rows), int(concurrency), window_ms, n_windows, out.ctypes.data, win.ctypes.data if n_windows else None)
    return decode_perf(out[0], win if n_windows else None)


def check_perf_batch(histories, concurrency, window_s=None, n_windows=0, max_rows=None, device=0):
    """:stats / :perf of several histories (arrays of rows) through the device kernel behind Engine.check_perf (msim_check_perf_batch);
    `max_rows` = the slab size (default: the longest history)."""
    window_ms, n_windows = _perf_windows(window_s, n_windows)
    slab, nr = _slab_form(histories, max_rows=max_rows)
    n = len(nr)
    out = np.zeros(n, dtype=PERF_DT)
    win = np.zeros((n, n_windows, A.PERF_MAX_F, 3), dtype=LATENCY_DT)
    _call("msim_check_perf_batch", device, slab.ctypes.data, nr.ctypes.data, slab.shape[1], n, int(concurrency), window_ms, n_windows, out.ctypes.data, win.ctypes.data if n_windows else None)
    return [decode_perf(out[i], win[i] if n_windows else None) for i in range(n)]


def check_lin_kv_batch(histories, device=0):
    """lin-kv: per-key linearizability of several histories (each an array of rows) with the device search behind Engine.check()
    (msim_check_lin_kv_batch).  Returns the CHECK_DT records, one per history."""
    rows, off = _offsets_form(histories, payload=False)   # histories without a single row go in as no rows; explain_lin_kv_batch pads them
    out = np.zeros(len(off) - 1, dtype=CHECK_DT)
    _call("msim_check_lin_kv_batch", device, rows.ctypes.data, off.ctypes.data, len(out), out.ctypes.data)
    return out


def explain_lin_kv_history(rows, max_keys=256):
    """The explaining lin-kv check of one history on the host (msim_explain_lin_kv_rows) -> (CHECK_DT record, LIN_KEY_DT records, one per
    key ascending: Knossos' :op / :previous-ok rows and the :configs' register values; include/maelsim.h msim_lin_key_result)."""
    rows = np.ascontiguousarray(rows)
    out = np.zeros(1, dtype=CHECK_DT)
    keys = np.zeros(max_keys, dtype=LIN_KEY_DT)
    n = C.c_uint32()
    _call("msim_explain_lin_kv_rows", rows.ctypes.data, len(rows), out.ctypes.data_as(C.POINTER(A.CheckResult)), keys.ctypes.data, max_keys, C.byref(n))
    return out[0], keys[:min(n.value, max_keys)].copy()


def explain_lin_kv_batch(histories, device=0, max_keys=256, with_n_host=False):
    """The explaining lin-kv check of several histories (arrays of rows) with the device search (msim_explain_lin_kv_batch): per history
    (CHECK_DT record — what check_lin_kv_batch gives —, LIN_KEY_DT records as explain_lin_kv_history gives them).  with_n_host: also how
    many histories the host search finished."""
    rows, off = _offsets_form(histories, payload=False)
    if len(rows) == 0:   # unlike check_lin_kv_batch, which hands no rows in as they are: one zero row
        rows = np.zeros(1, dtype=OP_DT)
    n = len(off) - 1
    out = np.zeros(n, dtype=CHECK_DT)
    keys = np.zeros((n, max_keys), dtype=LIN_KEY_DT)
    nk = np.zeros(n, dtype=np.uint32)
    n_host = C.c_uint32()
    _call("msim_explain_lin_kv_batch", device, rows.ctypes.data, off.ctypes.data, n, out.ctypes.data, keys.ctypes.data, max_keys, nk.ctypes.data, C.byref(n_host))
    res = [(out[i], keys[i, :min(int(nk[i]), max_keys)].copy()) for i in range(n)]
    return (res, n_host.value) if with_n_host else res


def lin_kv_analysis(rows, key_records, payload=None, n_nodes=0):
    """The Jepsen-shaped result map of `independent/checker` over Knossos' `checker/linearizable` from the key records of one history
    (pure formatting): {"valid?", "results": {k: {"linearizable": {"valid?", "op", "previous-ok", "configs": [{"model": v}, ...],
    "pending-count"}}}, "failures": [k ...]}; op / previous-ok are the history's ops as decode_history gives them (None where the record
    has MSIM_NO_VALUE), a model value None is nil.  Not reported: :final-paths, :last-op, the number of configurations."""
    verdict = {1: True, 0: False, 2: "unknown"}
    ops = []

    def op_at(row):
        if int(row) == A.NO_VALUE:
            return None
        if not ops:
            ops.extend(decode_history(rows, payload if payload is not None else np.zeros(1, dtype=np.uint32), n_nodes, A.WL_LIN_KV))
        return ops[int(row)]

    results, failures = {}, []
    for rec in key_records:
        k, valid = int(rec["key"]), verdict[int(rec["valid"])]
        n_shown = min(int(rec["n_values"]), 8)
        results[k] = {"linearizable": {"valid?": valid, "op": op_at(rec["op_row"]), "previous-ok": op_at(rec["previous_ok_row"]),
                                       "configs": [{"model": _nil(int(v))} for v in rec["values"][:n_shown]], "value-count": int(rec["n_values"]),
                                       "pending-count": int(rec["n_pending"])}}
        if valid is False:
            failures.append(k)
    valid = False if failures else ("unknown" if any(r["linearizable"]["valid?"] == "unknown" for r in results.values()) else True)
    return {"valid?": valid, "results": results, "failures": failures}


def check_unique_batch(histories, device=0, fn="msim_check_unique_batch"):
    """unique-ids (or, with fn="msim_check_pn_batch", pn-counter / g-counter): several histories (arrays of rows) through the device
    checker behind Engine.check()."""
    slab, nr = _slab_form(histories)
    out = np.zeros(len(nr), dtype=CHECK_DT)
    _call(fn, device, slab.ctypes.data, nr.ctypes.data, slab.shape[1], len(nr), out.ctypes.data)
    return out


def check_set_full_batch(histories, concurrency, workload=A.WL_BROADCAST, max_values=None, device=0):
    """broadcast / g-set (set-full) or echo: several histories — (rows, payload words) pairs — through the device checker behind
    Engine.check() (msim_check_set_full_batch)."""
    rows, nr, pay, max_values = _set_full_slabs(histories, max_values)
    out = np.zeros(len(nr), dtype=CHECK_DT)
    _call("msim_check_set_full_batch", device, workload, concurrency, rows.ctypes.data, nr.ctypes.data, rows.shape[1], pay.ctypes.data, pay.shape[1],
          max_values, len(nr), out.ctypes.data)
    return out


def _n_set_records(hdr):
    return int(hdr["n_lost"]) + int(hdr["n_never_read"]) + int(hdr["n_stale"])


def _set_full_slabs(histories, max_values):
    """(rows, n_rows, payload, max_values) of check_set_full_batch's call"""
    rows, nr, pay = _slab_form(histories, payload=True)
    if max_values is None:   # every add / broadcast invocation creates one element
        f = (rows["packed"] >> 2) & 31
        adds = (((f == A.F_ADD) | (f == A.F_BROADCAST)) & ((rows["packed"] & 3) == 0)).sum(axis=1).max()
        max_values = max(32, (int(adds) + 31) // 32 * 32)
    return rows, nr, pay, max_values


def explain_set_full_history(rows, payload, workload=A.WL_BROADCAST, max_elements=256):
    """The explaining set-full check of one broadcast / g-set history on the host (msim_explain_set_full_rows; needs no device) ->
    (CHECK_DT record, SET_EXPLAIN_DT header, SET_ELEMENT_DT records: the lost, never-read and stale elements as include/maelsim.h
    msim_set_explain lays them out).  The whole zero-padded slab of max_elements records is the returned array's `.base`."""
    rows = np.ascontiguousarray(rows); payload = np.ascontiguousarray(payload, dtype=np.uint32)
    out = np.zeros(1, dtype=CHECK_DT)
    hdr = np.zeros(1, dtype=SET_EXPLAIN_DT)
    slab = np.zeros(max(max_elements, 1), dtype=SET_ELEMENT_DT)
    _call("msim_explain_set_full_rows", workload, rows.ctypes.data, len(rows), payload.ctypes.data, len(payload),
          out.ctypes.data_as(C.POINTER(A.CheckResult)), hdr.ctypes.data, slab.ctypes.data, max_elements)
    return out[0], hdr[0], slab[:_n_set_records(hdr[0])]


def explain_set_full_batch(histories, concurrency, workload=A.WL_BROADCAST, max_values=None, device=0, max_elements=256):
    """broadcast / g-set: check_set_full_batch with the explanation written on the device (msim_explain_set_full_batch).  Returns
    (CHECK_DT records, SET_EXPLAIN_DT headers, a list of SET_ELEMENT_DT arrays — the records written per history); the whole zero-padded
    slab is the returned list's `.slab` ((histories, max_elements))."""
    rows, nr, pay, max_values = _set_full_slabs(histories, max_values)
    n = len(nr)
    out = np.zeros(n, dtype=CHECK_DT)
    hdr = np.zeros(n, dtype=SET_EXPLAIN_DT)
    slab = np.zeros((n, max(max_elements, 1)), dtype=SET_ELEMENT_DT)
    _call("msim_explain_set_full_batch", device, workload, concurrency, rows.ctypes.data, nr.ctypes.data, rows.shape[1], pay.ctypes.data, pay.shape[1],
          max_values, n, out.ctypes.data, hdr.ctypes.data, slab.ctypes.data, max_elements)
    els = _StepLists(slab[i, :_n_set_records(hdr[i])].copy() for i in range(n))
    els.slab = slab[:, :max_elements]
    return out, hdr, els


def set_full_analysis(record, header, elements, rows=None, payload=None, n_nodes=0, workload=A.WL_BROADCAST):
    """The Jepsen-shaped result map of `checker/set-full` (doc/03-broadcast/01-broadcast.md:564-577) from one history's record, header
    and element records (pure formatting): valid?, the five counts, lost / never-read / stale (element lists), worst-stale (a list of
    {element, outcome, stable-latency, known, last-absent}), stable-latencies / lost-latencies ({0 .5 .95 .99 1}; only where the class
    has members), duplicated-count, duplicated.  With `rows`, known / last-absent are the ops as decode_history gives them, else row
    indices (None = nil).  A truncated header gives the lists as far as they were written, and "truncated": True."""
    ops = []

    def op_at(row):
        if int(row) == A.NO_VALUE:
            return None
        if rows is None:
            return int(row)
        if not ops:
            ops.extend(decode_history(rows, payload if payload is not None else np.zeros(1, dtype=np.uint32), n_nodes, workload))
        return ops[int(row)]

    nl, nn = int(header["n_lost"]), int(header["n_never_read"])
    pts = PERF_QUANTILES
    res = {"valid?": {1: True, 0: False, 2: "unknown"}[int(record["valid"])],
           "attempt-count": int(record["attempt_count"]), "stable-count": int(record["stable_count"]), "lost-count": int(record["lost_count"]),
           "lost": [int(e["element"]) for e in elements[:nl]],
           "never-read-count": int(record["never_read_count"]), "never-read": [int(e["element"]) for e in elements[nl:nl + nn]],
           "stale-count": int(record["stale_count"]), "stale": [int(e["element"]) for e in elements[nl + nn:]],
           "worst-stale": [{"element": int(e["element"]), "outcome": A.SET_OUTCOMES[int(e["outcome"])], "stable-latency": int(e["latency_ms"]),
                            "known": op_at(e["known_row"]), "last-absent": op_at(e["last_absent_row"])}
                           for e in header["worst_stale"][:int(header["n_worst_stale"])]],
           "duplicated-count": int(record["duplicated_count"]), "duplicated": {}}
    if int(record["stable_count"]):
        res["stable-latencies"] = {q: int(v) for q, v in zip(pts, record["stable_latency_ms"])}
    if int(record["lost_count"]):
        res["lost-latencies"] = {q: int(v) for q, v in zip(pts, header["lost_latency_ms"])}
    if int(header["truncated"]):
        res["truncated"] = True
    return res


def _pn_segments(hdr, slab):
    """(PN_READ_DT final reads, PN_RANGE_DT ranges) of one history's slab of 16-byte records"""
    nr, ng = int(hdr["n_reads"]), int(hdr["n_ranges"])
    return slab[:nr].copy(), slab[nr:nr + ng].copy().view(PN_RANGE_DT)


def _explain_small_history(entry, rows, hdr_dt, rec_dt, cap, *extra):
    rows = np.ascontiguousarray(rows)
    out = np.zeros(1, dtype=CHECK_DT)
    hdr = np.zeros(1, dtype=hdr_dt)
    slab = np.zeros(max(cap, 1), dtype=rec_dt)
    _call(entry, rows.ctypes.data, len(rows), *extra, out.ctypes.data_as(C.POINTER(A.CheckResult)), hdr.ctypes.data, slab.ctypes.data, cap)
    return out[0], hdr[0], slab[:cap]


def _explain_small_batch(entry, histories, device, hdr_dt, rec_dt, cap, *extra):
    """-> (CHECK_DT records, headers, the (histories, cap) slab, n_host)"""
    slab, nr = _slab_form(histories)
    n = len(nr)
    out = np.zeros(n, dtype=CHECK_DT)
    hdr = np.zeros(n, dtype=hdr_dt)
    recs = np.zeros((n, max(cap, 1)), dtype=rec_dt)
    n_host = C.c_uint32()
    _call(entry, device, *extra, slab.ctypes.data, nr.ctypes.data, slab.shape[1], n, out.ctypes.data, hdr.ctypes.data, recs.ctypes.data, cap, C.addressof(n_host))
    return out, hdr, recs[:, :cap], n_host.value


def explain_pn_history(rows, max_records=256):
    """The explaining pn-counter / g-counter check of one history on the host (msim_explain_pn_rows; needs no device) -> (CHECK_DT
    record, PN_EXPLAIN_DT header, PN_READ_DT final reads, PN_RANGE_DT acceptable ranges; include/maelsim_small_explain.h)."""
    out, hdr, slab = _explain_small_history("msim_explain_pn_rows", rows, PN_EXPLAIN_DT, PN_READ_DT, max_records)
    return (out, hdr) + _pn_segments(hdr, slab)


def explain_pn_batch(histories, device=0, max_records=256, with_n_host=False):
    """pn-counter / g-counter: check_pn_batch with the explanation written on the device (msim_explain_pn_batch).  Returns (CHECK_DT
    records, PN_EXPLAIN_DT headers, a list of (final reads, ranges) per history); the whole zero-padded slab of 16-byte records is the
    list's `.slab`.  with_n_host: also how many histories the host walk explained."""
    out, hdr, slab, n_host = _explain_small_batch("msim_explain_pn_batch", histories, device, PN_EXPLAIN_DT, PN_READ_DT, max_records)
    segs = _StepLists(_pn_segments(hdr[i], slab[i]) for i in range(len(out)))
    segs.slab = slab
    return (out, hdr, segs, n_host) if with_n_host else (out, hdr, segs)


def pn_analysis(record, header, reads, ranges, rows=None, n_nodes=0, workload=A.WL_PN_COUNTER):
    """The reference's result map (workload/pn_counter.clj:122-125) from one history's record, header, final reads and ranges (pure
    formatting): {"valid?", "errors" (None where there is none: (seq errors)), "final-reads", "acceptable"}; the errors are the ops
    as decode_history gives them with `rows`, else row indices.  A truncated header gives what was written, and "truncated": True."""
    bad = [int(r["row"]) for r in reads if not int(r["in_set"])]
    if rows is not None and bad:
        ops = decode_history(rows, np.zeros(1, dtype=np.uint32), n_nodes, workload)
        bad = [ops[i] for i in bad]
    res = {"valid?": bool(int(record["valid"])), "errors": bad or None, "final-reads": [int(r["value"]) for r in reads],
           "acceptable": [[int(g["lower"]), int(g["upper"])] for g in ranges]}
    if int(header["truncated"]):
        res["truncated"] = True
    return res


def explain_unique_history(rows, max_dups=48):
    """The explaining unique-ids check of one history on the host (msim_explain_unique_rows) -> (CHECK_DT record, UNIQUE_EXPLAIN_DT
    header, UNIQUE_DUP_DT records: the duplicated ids by count descending, then packed id descending)."""
    out, hdr, slab = _explain_small_history("msim_explain_unique_rows", rows, UNIQUE_EXPLAIN_DT, UNIQUE_DUP_DT, max_dups)
    return out, hdr, slab[:int(hdr["n_dups"])]


def explain_unique_batch(histories, device=0, max_dups=48, with_n_host=False):
    """unique-ids: check_unique_batch with the explanation written on the device (msim_explain_unique_batch).  Returns (CHECK_DT
    records, UNIQUE_EXPLAIN_DT headers, a list of UNIQUE_DUP_DT arrays); the whole slab is the list's `.slab`."""
    out, hdr, slab, n_host = _explain_small_batch("msim_explain_unique_batch", histories, device, UNIQUE_EXPLAIN_DT, UNIQUE_DUP_DT, max_dups)
    dups = _StepLists(slab[i, :int(hdr[i]["n_dups"])].copy() for i in range(len(out)))
    dups.slab = slab
    return (out, hdr, dups, n_host) if with_n_host else (out, hdr, dups)


def decode_id(value, node_program=None):
    """a packed :generate :value as decode_history presents it: a lin-tso timestamp, else a flake id [time count node-id]"""
    value = int(value)
    return value if node_program == A.NODE_TSO_IDS else [value >> 20, (value >> 5) & 0x7FFF, f"n{value & 31}"]


def unique_ids_analysis(record, header, dups, node_program=None):
    """[upstream] jepsen.checker/unique-ids' result map from one history's record, header and duplicate records (pure formatting):
    {"valid?", "attempted-count", "acknowledged-count", "duplicated-count", "duplicated", "range"}.  "duplicated" takes the first 48
    records — the most often acknowledged ids — and presents them sorted by id, as [id, count] pairs (a flake id is a vector, no key
    of a Python dict); ids are decoded per node program, as decode_history decodes them."""
    shown = sorted(((int(d["id"]), int(d["count"])) for d in dups[:48]))
    lo, hi = (int(v) for v in record["stable_latency_ms"][:2])
    res = {"valid?": bool(int(record["valid"])), "attempted-count": int(record["attempt_count"]), "acknowledged-count": int(record["ok_count"]),
           "duplicated-count": int(record["duplicated_count"]), "duplicated": [[decode_id(i, node_program), c] for i, c in shown],
           "range": [decode_id(lo, node_program), decode_id(hi, node_program)] if int(record["ok_count"]) else [None, None]}
    if int(header["truncated"]):
        res["truncated"] = True
    return res


def explain_echo_history(rows, concurrency, max_errors=64):
    """The explaining echo check of one history on the host (msim_explain_echo_rows) -> (CHECK_DT record, ECHO_EXPLAIN_DT header,
    ECHO_ERROR_DT records: the invocations that count as errors, ascending by row)."""
    out, hdr, slab = _explain_small_history("msim_explain_echo_rows", rows, ECHO_EXPLAIN_DT, ECHO_ERROR_DT, max_errors, int(concurrency))
    return out, hdr, slab[:int(hdr["n_errors"])]


def explain_echo_batch(histories, concurrency, device=0, max_errors=64, with_n_host=False):
    """echo: check_set_full_batch(workload=WL_ECHO) with the explanation written on the device (msim_explain_echo_batch).  Returns
    (CHECK_DT records, ECHO_EXPLAIN_DT headers, a list of ECHO_ERROR_DT arrays); the whole slab is the list's `.slab`."""
    out, hdr, slab, n_host = _explain_small_batch("msim_explain_echo_batch", histories, device, ECHO_EXPLAIN_DT, ECHO_ERROR_DT, max_errors, int(concurrency))
    errs = _StepLists(slab[i, :int(hdr[i]["n_errors"])].copy() for i in range(len(out)))
    errs.slab = slab
    return (out, hdr, errs, n_host) if with_n_host else (out, hdr, errs)


def echo_analysis(record, header, errors):
    """workload/echo.clj:62-63's result map from one history's record, header and error records (pure formatting): {"valid?", "errors":
    [["Expected a message with :echo", v, "But received", v'], ...]} — v the invocation's :value, v' the completion's (an echo_ok body
    where it was an :ok, else None: a :fail / :info carries no body, a missing completion is nil)."""
    def body(v):
        return None if int(v) == A.NO_VALUE else {"type": "echo_ok", "echo": f"Please echo {int(v)}"}
    res = {"valid?": bool(int(record["valid"])),
           "errors": [["Expected a message with :echo", f"Please echo {int(e['expected'])}", "But received", body(e["received"])] for e in errors]}
    if int(header["truncated"]):
        res["truncated"] = True
    return res


def check_pn_batch(histories, device=0):
    """pn-counter / g-counter: several histories through the device checker behind Engine.check() (msim_check_pn_batch)."""
    return check_unique_batch(histories, device, fn="msim_check_pn_batch")


def check_txn_batch(histories, device=0):
    """txn-list-append: several histories, each (rows, payload), through the device pass behind Engine.check() with the host analysis
    for what it cannot prove clean (msim_check_txn_batch).  Returns the CHECK_DT records, one per history."""
    rows, ro, pay, po = _offsets_form(histories)
    out = np.zeros(len(ro) - 1, dtype=CHECK_DT)
    _call("msim_check_txn_batch", device, rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, len(out), out.ctypes.data)
    return out


def _check_offsets_batch(entry, histories, device, word):
    """The entries (device, offsets form, n_histories, one word — a consistency model or the concurrency —, out, n_host)"""
    rows, ro, pay, po = _offsets_form(histories)
    out = np.zeros(len(ro) - 1, dtype=CHECK_DT)
    n_host = C.c_uint32()
    _call(entry, device, rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, len(out), word, out.ctypes.data, C.byref(n_host))
    return out, n_host.value


def check_rw_batch(histories, consistency_model="read-committed", device=0, _entry="msim_check_rw_batch"):
    """txn-rw-register: several histories, each (rows, payload), through the device passes behind Engine.check(): one proves a history
    free of what the model proscribes, the other analyses and classifies the rest (msim_check_rw_batch); the host analysis only takes
    what exceeds the device capacities.  Returns (CHECK_DT records, how many histories went to the host)."""
    return _check_offsets_batch(_entry, histories, device, CONSISTENCY_MODELS[consistency_model])


def classify_rw_batch(histories, consistency_model="read-committed", device=0):
    """txn-rw-register: the full analysis of every history on the device (msim_classify_rw_batch): each record is what
    check_rw_history's msim_check_rw_rows writes, the allowed cycle classes of valid histories included.  Returns (records, n_host)."""
    return check_rw_batch(histories, consistency_model, device, _entry="msim_classify_rw_batch")


def classify_txn_batch(histories, consistency_model="strict-serializable", device=0):
    """txn-list-append: several histories, each (rows, payload), analysed on the device whatever they hold (msim_classify_txn_batch): the
    clean passes of check_txn_batch first, then the full analysis (every anomaly, the cycle classes) of what they cannot prove clean.
    Each record is what check_txn_batch gives, judged under `consistency_model`; the host analysis only takes what exceeds the device
    capacities.  Returns (CHECK_DT records, how many histories went to the host)."""
    return check_rw_batch(histories, consistency_model, device, _entry="msim_classify_txn_batch")


def explain_txn_history(rows, payload, consistency_model="strict-serializable", max_steps=64, _entry="msim_explain_txn_rows"):
    """The host list-append analysis of one history with the witness cycle of its cycle class (msim_explain_txn_rows; include/maelsim.h
    msim_cycle_result) -> (CHECK_DT record, CYCLE_DT record, CYCLE_STEP_DT steps, the first min(length, max_steps) of the cycle)."""
    rows = np.ascontiguousarray(rows); payload = np.ascontiguousarray(payload, dtype=np.uint32)
    out = np.zeros(1, dtype=CHECK_DT)
    cycle = np.zeros(1, dtype=CYCLE_DT)
    steps = np.zeros(max_steps, dtype=CYCLE_STEP_DT)
    _call(_entry, rows.ctypes.data, len(rows), payload.ctypes.data, len(payload), CONSISTENCY_MODELS[consistency_model],
          out.ctypes.data_as(C.POINTER(A.CheckResult)), cycle.ctypes.data, steps.ctypes.data, max_steps)
    return out[0], cycle[0], steps[:int(cycle[0]["n_steps"])].copy()


def explain_rw_history(rows, payload, consistency_model="strict-serializable", max_steps=64):
    """The same for one rw-register history (msim_explain_rw_rows)."""
    return explain_txn_history(rows, payload, consistency_model, max_steps, _entry="msim_explain_rw_rows")


def explain_txn_batch(histories, consistency_model="strict-serializable", device=0, max_steps=64, _entry="msim_explain_txn_batch"):
    """txn-list-append: classify_txn_batch with the witness cycles found on the device (msim_explain_txn_batch).  Returns (CHECK_DT
    records, CYCLE_DT records, a list of CYCLE_STEP_DT arrays — the steps written per history —, how many histories went to the host).
    The whole zero-padded slab of steps is the returned list's `.slab` ((histories, max_steps))."""
    rows, ro, pay, po = _offsets_form(histories)
    n = len(ro) - 1
    out = np.zeros(n, dtype=CHECK_DT)
    cycles = np.zeros(n, dtype=CYCLE_DT)
    slab = np.zeros((n, max_steps), dtype=CYCLE_STEP_DT)
    n_host = C.c_uint32()
    _call(_entry, device, rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, n,
          CONSISTENCY_MODELS[consistency_model], out.ctypes.data, C.byref(n_host), cycles.ctypes.data, slab.ctypes.data, max_steps)
    steps = _StepLists(slab[i, :int(cycles[i]["n_steps"])].copy() for i in range(n))
    steps.slab = slab
    return out, cycles, steps, n_host.value


class _StepLists(list):
    """explain_txn_batch's list of step arrays; `.slab` is the whole zero-padded array the entry wrote"""


def explain_rw_batch(histories, consistency_model="read-committed", device=0, max_steps=64):
    """txn-rw-register: classify_rw_batch with the witness cycles found on the device (msim_explain_rw_batch); as explain_txn_batch."""
    return explain_txn_batch(histories, consistency_model, device, max_steps, _entry="msim_explain_rw_batch")


def txn_cycle_analysis(rows, payload, cycle, steps, n_nodes=0, rw=False):
    """elle's :anomalies map for the witness cycle of one history (pure formatting): {"anomalies": {"G-single-realtime": [{"cycle":
    [ops ...], "steps": [{"type": "rw"}, ...]}]}} — the cycle's ops are the transactions' completions as decode_history gives them (the
    invocation where one never completed), a step's type the strongest-first name of its kinds ("ww", "wr", "rw", "realtime"; "types"
    lists all of them where parallel edges were merged).  No cycle: {"anomalies": {}}.  A witness longer than the steps given is
    marked "truncated": its true length.  Not reported: the :key / :value of a step, witnesses of the non-cycle anomalies."""
    bits = int(cycle["anomalies"])
    if not bits:
        return {"anomalies": {}}
    name = next(n for b, n in A.ANOMALIES.items() if bits & b & 0x39) + ("-realtime" if bits & 512 else "")
    ops = decode_history(rows, payload, n_nodes, A.WL_TXN_RW_REGISTER if rw else A.WL_TXN_LIST_APPEND)
    entry = {"cycle": [ops[int(s["inv_row"] if int(s["cmp_row"]) == A.NO_VALUE else s["cmp_row"])] for s in steps],
             "steps": [dict({"type": next(n for b, n in A.EDGE_KINDS.items() if int(s["kinds"]) & b)},
                            **({"types": [n for b, n in A.EDGE_KINDS.items() if int(s["kinds"]) & b]} if bin(int(s["kinds"])).count("1") > 1 else {}))
                       for s in steps]}
    if int(cycle["length"]) > len(steps):
        entry["truncated"] = int(cycle["length"])
    return {"anomalies": {name: [entry]}}


def explain_txn_findings_history(rows, payload, workload="txn-list-append", consistency_model="strict-serializable", max_findings=64):
    """The host analysis of one list-append / rw-register history with a witness for every non-cycle anomaly
    (msim_explain_txn_findings_rows; needs no device) -> (CHECK_DT record — what msim_check_txn_rows / msim_check_rw_rows write —,
    TXN_EXPLAIN_DT header, TXN_FINDING_DT records as include/maelsim_txn_findings.h defines them, in its order).  The whole zero-padded
    slab of max_findings records is the returned array's `.base`."""
    rows = np.ascontiguousarray(rows); payload = np.ascontiguousarray(payload, dtype=np.uint32)
    out = np.zeros(1, dtype=CHECK_DT)
    hdr = np.zeros(1, dtype=TXN_EXPLAIN_DT)
    slab = np.zeros(max(max_findings, 1), dtype=TXN_FINDING_DT)
    _call("msim_explain_txn_findings_rows", WORKLOADS[workload], rows.ctypes.data, len(rows), payload.ctypes.data, len(payload),
          CONSISTENCY_MODELS[consistency_model], out.ctypes.data_as(C.POINTER(A.CheckResult)), hdr.ctypes.data, slab.ctypes.data, max_findings)
    return out[0], hdr[0], slab[:int(hdr[0]["n_findings"])]


def explain_txn_findings_batch(histories, workload="txn-list-append", consistency_model="strict-serializable", device=0, max_findings=64,
                               with_n_host=False):
    """classify_txn_batch / classify_rw_batch with the non-cycle findings written on the device (msim_explain_txn_findings_batch;
    txn_findings_kernel / rw_findings_kernel).  Returns (CHECK_DT records, TXN_EXPLAIN_DT headers, a list of TXN_FINDING_DT arrays — the
    records written per history, whose `.slab` is the whole zero-padded (histories, max_findings) array)[, how many histories went to
    the host walk: the hand-overs of the classify entries, and more than A.TXN_FINDINGS_CAPACITY findings]."""
    rows, ro, pay, po = _offsets_form(histories)
    n = len(ro) - 1
    out = np.zeros(n, dtype=CHECK_DT)
    hdr = np.zeros(n, dtype=TXN_EXPLAIN_DT)
    slab = np.zeros((n, max(max_findings, 1)), dtype=TXN_FINDING_DT)
    n_host = C.c_uint32()
    _call("msim_explain_txn_findings_batch", device, WORKLOADS[workload], rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, n,
          CONSISTENCY_MODELS[consistency_model], out.ctypes.data, C.byref(n_host), hdr.ctypes.data, slab.ctypes.data, max_findings)
    fs = _StepLists(slab[i, :int(hdr[i]["n_findings"])].copy() for i in range(n))
    fs.slab = slab[:, :max_findings]
    return (out, hdr, fs, n_host.value) if with_n_host else (out, hdr, fs)


def txn_findings_analysis(rows, payload, header, findings, rw=False, n_nodes=0):
    """elle's :anomalies map for the non-cycle findings of one history (pure formatting): {"anomalies": {"internal": [{"op", "mop",
    "expected"}], "incompatible-order": [{"key", "values": [list(m), ord(k)]}], "G1a": [{"op", "mop", "element", "writer"}], "G1b":
    [... "writer", "writer-final"], "duplicate-elements": [...], "dirty-update": [...], "cyclic-versions": [{"key", "element",
    "count"}]}}.  Ops are decode_history's (a transaction's completion; its invocation where it never completed); `expected` of a
    list-append internal finding is the earlier read's list followed by the transaction's own appends since, or ["...", *appends]
    without an earlier read; a list marked "truncated" names the true number of findings where the slab held fewer."""
    ops = decode_history(rows, payload, n_nodes, A.WL_TXN_RW_REGISTER if rw else A.WL_TXN_LIST_APPEND)
    NV = A.NO_VALUE

    def party(inv, cmp_):
        """(the op shown, the transaction's form)"""
        if inv == NV:
            return (ops[cmp_] if cmp_ != NV else None), None
        done = cmp_ != NV
        form = ops[cmp_] if done and (int(rows["packed"][cmp_]) & 3) == A.T_OK else ops[inv]
        return (ops[cmp_] if done else ops[inv]), form["value"]

    def val(x):
        return None if x == NV else x

    out = {}
    for f in findings:
        f = {k: int(f[k]) for k in f.dtype.names}
        name = A.ANOMALIES[f["anomaly"]]
        op, form = party(f["inv_row"], f["cmp_row"])
        w_op, w_form = party(f["other_inv_row"], f["other_cmp_row"])
        mop = form[f["mop"]] if form is not None and f["mop"] != NV else None
        if name == "internal":
            e = {"op": op, "mop": mop}
            if mop is not None and not rw:
                since = 0 if f["other_mop"] == NV else f["other_mop"] + 1
                own = [m[2] for m in form[since:f["mop"]] if m[0] == ":append" and m[1] == f["key"]]
                e["expected"] = (["..."] if f["other_mop"] == NV else list(form[f["other_mop"]][2] or [])) + own
            elif mop is not None:
                e["expected"] = val(f["other_element"])
        elif name == "incompatible-order":
            e = {"key": f["key"], "values": [mop[2], w_form[f["other_mop"]][2]]}
        elif name == "cyclic-versions":
            e = {"key": f["key"], "element": f["element"] or None, "count": f["count"]}
        elif name == "dirty-update":
            e = {"key": f["key"], "op": op, "element": f["element"], "writer": w_op, "aborted-element": f["other_element"]}
        elif name == "duplicate-elements":
            e = {"op": op, "mop": mop, "key": f["key"], "element": f["element"]}
            if w_op is not None:
                e.update({"other-op": w_op, "other-mop": w_form[f["other_mop"]], "count": f["count"]})
            else:
                e["positions"] = [f["count"], f["other_element"]]
        else:   # G1a, G1b
            e = {"op": op, "mop": mop, "key": f["key"], "element": f["element"], "writer": w_op}
            if name == "G1b":
                e["writer-final"] = f["other_element"]
        out.setdefault(name, []).append(e)
    bits = {b: n for b, n in A.ANOMALIES.items()}
    for b, name in bits.items():
        true_n = int(header["count"][b.bit_length() - 1])
        if true_n > len(out.get(name, [])):
            out.setdefault(name, []).append({"truncated": true_n})
    return {"anomalies": out}


def anomaly_census(results):
    """How many records of a txn check (CHECK_DT) carry each anomaly of A.ANOMALIES (by name), and how many none ("clean")."""
    bits = np.asarray(results["error_count"], dtype=np.uint32)
    census = {name: int(((bits & np.uint32(b)) != 0).sum()) for b, name in A.ANOMALIES.items()}
    census["clean"] = int((bits == 0).sum())
    return census



def check_kafka_batch(histories, concurrency, device=0, _entry="msim_check_kafka_batch"):
    """kafka: several histories, each (rows, payload), through the device pass behind Engine.check() (csrc/kafka_check_dev.hip) with the
    host checker for what it cannot prove clean (msim_check_kafka_batch); `concurrency` = the worker threads of the test.  Returns
    (CHECK_DT records, how many histories went to the host)."""
    return _check_offsets_batch(_entry, histories, device, concurrency)


def classify_kafka_batch(histories, concurrency, device=0):
    """kafka: as check_kafka_batch, but a history the device cannot prove clean has its anomalies named on the device too
    (msim_classify_kafka_batch, kafka_classify_kernel): every record is what check_kafka_history's msim_check_kafka_rows writes, all
    anomaly bits and counts.  Only what does not decode, a process that returns after a later one of its worker, and offsets or messages
    from 1152 on go to the host checker.  Returns (CHECK_DT records, how many histories went to the host).  See kafka_anomaly_census."""
    return check_kafka_batch(histories, concurrency, device, _entry="msim_classify_kafka_batch")


def explain_kafka_history(rows, payload, max_findings=64):
    """The explaining kafka check of one history on the host (msim_explain_kafka_rows; needs no device) -> (CHECK_DT record — what
    msim_check_kafka_rows writes —, KAFKA_EXPLAIN_DT header, KAFKA_FINDING_DT records: one witness per anomaly as include/maelsim.h
    defines them, in its order).  The whole zero-padded slab of max_findings records is the returned array's `.base`."""
    rows = np.ascontiguousarray(rows); payload = np.ascontiguousarray(payload, dtype=np.uint32)
    out = np.zeros(1, dtype=CHECK_DT)
    hdr = np.zeros(1, dtype=KAFKA_EXPLAIN_DT)
    slab = np.zeros(max(max_findings, 1), dtype=KAFKA_FINDING_DT)
    _call("msim_explain_kafka_rows", rows.ctypes.data, len(rows), payload.ctypes.data, len(payload), out.ctypes.data_as(C.POINTER(A.CheckResult)),
          hdr.ctypes.data, slab.ctypes.data, max_findings)
    return out[0], hdr[0], slab[:int(hdr[0]["n_findings"])]


def explain_kafka_batch(histories, concurrency, device=0, max_findings=64):
    """kafka: classify_kafka_batch with the explanation written on the device (msim_explain_kafka_batch, kafka_explain_kernel).  Returns
    (CHECK_DT records, KAFKA_EXPLAIN_DT headers, a list of KAFKA_FINDING_DT arrays — the records written per history, whose `.slab` is
    the whole zero-padded (histories, max_findings) array —, how many histories went to the host walk: the three cases of
    classify_kafka_batch, offsets or messages from A.KAFKA_EXPLAIN_TABLE_BOUND on, more than A.KAFKA_EXPLAIN_MAX_FINDINGS findings)."""
    rows, ro, pay, po = _offsets_form(histories)
    n = len(ro) - 1
    out = np.zeros(n, dtype=CHECK_DT)
    hdr = np.zeros(n, dtype=KAFKA_EXPLAIN_DT)
    slab = np.zeros((n, max(max_findings, 1)), dtype=KAFKA_FINDING_DT)
    n_host = C.c_uint32()
    _call("msim_explain_kafka_batch", device, rows.ctypes.data, ro.ctypes.data, pay.ctypes.data, po.ctypes.data, n, concurrency, out.ctypes.data,
          hdr.ctypes.data, slab.ctypes.data, max_findings, C.byref(n_host))
    fs = _StepLists(slab[i, :int(hdr[i]["n_findings"])].copy() for i in range(n))
    fs.slab = slab[:, :max_findings]
    return out, hdr, fs, n_host.value


def kafka_findings(hdr, findings):
    """One history's findings named (pure formatting): a list of {"anomaly": its name in A.KAFKA_ANOMALIES, "key", "offset", "value",
    "other", "row-a", "row-b" (None = none)}; the polls' skips and nonmonotonic steps also carry jepsen's "delta" = offset - other, a
    skip its "skipped-count" = value (workload/kafka.clj:42-60).  A truncated header ends the list with {"truncated": the true counts by name}."""
    out = []
    for f in findings:
        bit = int(f["anomaly"])
        d = {"anomaly": A.KAFKA_ANOMALIES[bit], "key": int(f["key"]), "offset": int(f["offset"]), "value": int(f["value"]), "other": int(f["other"]),
             "row-a": None if int(f["row_a"]) == A.NO_VALUE else int(f["row_a"]), "row-b": None if int(f["row_b"]) == A.NO_VALUE else int(f["row_b"])}
        if bit & (2 | 8 | 16 | 32):
            d["delta"] = d["offset"] - d["other"]
        if bit & (8 | 32):
            d["skipped-count"] = d["value"]
        out.append(d)
    if int(hdr["truncated"]):
        out.append({"truncated": {name: int(hdr["count"][b.bit_length() - 1]) for b, name in A.KAFKA_ANOMALIES.items() if int(hdr["count"][b.bit_length() - 1])}})
    return out


def kafka_anomaly_census(results):
    """How many records of a kafka check (CHECK_DT) carry each anomaly of A.KAFKA_ANOMALIES (by name), and how many none ("clean")."""
    bits = np.asarray(results["error_count"], dtype=np.uint32)
    census = {name: int(((bits & np.uint32(b)) != 0).sum()) for b, name in A.KAFKA_ANOMALIES.items()}
    census["clean"] = int((bits == 0).sum())
    return census


def journal_fressian(cfg, events, payload):
    """One instance's net journal as the bytes of a net-journal/<stripe>.fressian file (msim_journal_fressian_rows, csrc/fressian.cpp):
    what maelstrom.net.journal writes (journal.clj:55-141) and maelstrom.net.checker / net.viz read."""
    ev = np.ascontiguousarray(events)
    pay = np.ascontiguousarray(payload, dtype=np.uint32)
    args = (C.byref(cfg), ev.ctypes.data, len(ev), pay.ctypes.data, len(pay))
    need = C.c_size_t()
    _call("msim_journal_fressian_rows", *args, None, 0, C.byref(need))
    buf = (C.c_ubyte * max(need.value, 1))()
    _call("msim_journal_fressian_rows", *args, buf, need.value, None)
    return bytes(buf[: need.value])


def journal_svg(cfg, events):
    """One journal as the reference's Lamport diagram (net/viz.clj:281-325), SVG text: a column per endpoint, a row per event, an arrow
    per delivered message (msim_journal_svg_rows, csrc/journal_svg.cpp; the first 10000 events behind the init traffic)."""
    events = np.ascontiguousarray(events)
    need = C.c_size_t()
    _call("msim_journal_svg_rows", C.byref(cfg), events.ctypes.data, len(events), None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value + 1)
    _call("msim_journal_svg_rows", C.byref(cfg), events.ctypes.data, len(events), buf, need.value, None)
    return buf.raw[:need.value].decode()


def history_edn_native(cfg, rows, payload):
    """history.edn text of one history straight from the binary rows (msim_history_edn_rows, csrc/edn.cpp)."""
    rows = np.ascontiguousarray(rows); payload = np.ascontiguousarray(payload, dtype=np.uint32)
    need = C.c_size_t()
    args = (C.byref(cfg), rows.ctypes.data, len(rows), payload.ctypes.data, len(payload))
    _call("msim_history_edn_rows", *args, None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    _call("msim_history_edn_rows", *args, buf, need.value, None)
    return buf.value.decode()


def history_edn(ops):
    """Jepsen history.edn text (one op map per line)."""
    def edn(v):
        if v is None:
            return "nil"
        if v is True:
            return "true"
        if isinstance(v, str):
            return v if v.startswith(":") else '"' + v + '"'
        if isinstance(v, dict):
            return "{" + ", ".join(f"{edn(k if str(k).startswith(':') else ':' + str(k)) if not (str(k).startswith('n') or str(k).isdigit()) else edn(str(k))} {edn(x)}" for k, x in v.items()) + "}"
        if isinstance(v, (list, tuple)):
            return "[" + " ".join(edn(x) for x in v) + "]"
        return str(v)
    lines = []
    for op in ops:
        keys = ["type", "f", "value", "time", "process", "index"] + [k for k in ("error", "final?", "seek-to-beginning?") if k in op]
        lines.append("{" + ", ".join(f":{k} {edn(op[k])}" for k in keys) + "}")
    return "\n".join(lines) + "\n"
