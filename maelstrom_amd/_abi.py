"""ctypes mirror of include/maelsim.h — the C-ABI boundary of libmaelsim.so.

This is the binding a reference maintainer would write on the JVM side as JNI (INTEGRATION.md shows that
stub); here it is ctypes because the host language available in this image is Python.  Nothing in this
module touches the oracle: if libmaelsim.so is missing or there is no HIP device the engine raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSIM_LIB") or os.path.join(HERE, "libmaelsim.so")   # MSIM_LIB: developer knob for A/B builds

ABI_VERSION = 1

# enums (include/maelsim.h)
OK, E_INVALID, E_NO_DEVICE, E_HIP, E_NOMEM, E_RANGE, E_UNSUPPORTED, E_OVERFLOW = 0, -1, -2, -3, -4, -5, -6, -7
WL_ECHO, WL_BROADCAST, WL_G_SET, WL_LIN_KV, WL_TXN_LIST_APPEND, WL_PN_COUNTER, WL_G_COUNTER, WL_UNIQUE_IDS, WL_TXN_RW_REGISTER, WL_KAFKA = range(10)
NODE_ECHO, NODE_BCAST_FF, NODE_BCAST_FF_ECHOBACK, NODE_BCAST_ACK_RETRY, NODE_BCAST_RPC_ALL, NODE_G_SET, NODE_RAFT, NODE_TXN_SINGLE_KEY, NODE_PN_COUNTER, NODE_FLAKE_IDS, NODE_LIN_KV_PROXY, NODE_TXN_RW_HAT, NODE_TXN_MULTI_KEY, NODE_TSO_IDS, NODE_KAFKA, NODE_TXN_DATOMIC, NODE_BCAST_BATCH = range(17)
SVC_LIN_KV, SVC_SEQ_KV, SVC_LWW_KV = range(3)
CM_STRICT_SERIALIZABLE, CM_SERIALIZABLE, CM_SNAPSHOT_ISOLATION, CM_READ_COMMITTED, CM_READ_UNCOMMITTED = range(5)
LAT_CONSTANT, LAT_UNIFORM, LAT_EXPONENTIAL = range(3)
TOPO_GRID, TOPO_LINE, TOPO_TOTAL, TOPO_TREE2, TOPO_TREE3, TOPO_TREE4 = range(6)
NEMESIS_PARTITION = 1
T_INVOKE, T_OK, T_FAIL, T_INFO = range(4)
F_ECHO, F_BROADCAST, F_READ, F_ADD, F_START_PARTITION, F_STOP_PARTITION, F_WRITE, F_CAS, F_TXN, F_GENERATE, F_SEND, F_POLL, F_ASSIGN, F_CRASH = range(14)
ERR_NONE, ERR_NET_TIMEOUT, ERR_RPC, ERR_TEMPORARILY_UNAVAILABLE, ERR_KEY_DOES_NOT_EXIST, ERR_PRECONDITION_FAILED, ERR_TXN_CONFLICT, ERR_TIMEOUT, ERR_ABORT = range(9)
SPEC_ONE, SPEC_MAJORITY, SPEC_MAJORITIES_RING, SPEC_MINORITY_THIRD = range(4)
PROCESS_NEMESIS = 0xFFFFF
NO_VALUE = 0xFFFFFFFF
FLAG_ROWS_OVERFLOW, FLAG_PAYLOAD_OVERFLOW, FLAG_INBOX_OVERFLOW, FLAG_VALUES_OVERFLOW, FLAG_ROUND_LIMIT, FLAG_JOURNAL_OVERFLOW, FLAG_ARENA_OVERRUN = 1, 2, 4, 8, 16, 32, 64
MSG_TYPES = ["", "init", "init_ok", "topology", "topology_ok", "echo", "echo_ok", "broadcast", "broadcast_ok", "read", "read_ok",
             "add", "add_ok", "replicate", "write", "write_ok", "cas", "cas_ok", "error", "request_vote", "request_vote_res",
             "append_entries", "append_entries_res", "txn", "txn_ok", "generate", "generate_ok", "replicate_ack", "ts", "ts_ok",
             "send", "send_ok", "poll", "poll_ok", "list_committed_offsets", "list_committed_offsets_ok", "commit_offsets", "commit_offsets_ok",
             "broadcast_many", "broadcast_many_ok"]
KAFKA_ANOMALIES = {1: "lost-write", 2: "nonmonotonic-poll", 4: "nonmonotonic-send", 8: "poll-skip", 16: "int-nonmonotonic-poll", 32: "int-poll-skip",
                   64: "inconsistent-offsets", 128: "duplicate", 256: "aborted-read", 512: "malformed"}
ANOMALIES = {1: "G0", 2: "G1a", 4: "G1b", 8: "G1c", 16: "G-single", 32: "G2", 64: "internal", 128: "duplicate-elements",
             256: "incompatible-order", 512: "realtime", 1024: "dirty-update", 2048: "cyclic-versions"}
MASK_WORDS = 4

SET_STABLE, SET_LOST, SET_NEVER_READ = range(3)   # MSIM_SET_*
SET_OUTCOMES = {SET_STABLE: "stable", SET_LOST: "lost", SET_NEVER_READ: "never-read"}
EDGE_KINDS = {1: "ww", 2: "wr", 4: "rw", 8: "realtime"}   # MSIM_EDGE_*
AVAIL_NIL, AVAIL_TOTAL, AVAIL_FRACTION = range(3)
PERF_MAX_F, PERF_MAX_WINDOWS = 4, 16
COMM_ID_BYTES = 128
# kafka_explain_kernel's capacities (csrc/kafka_check_dev.hip): an observation that names an offset or message from KAFKA_EXPLAIN_TABLE_BOUND
# on, and a history of more than KAFKA_EXPLAIN_MAX_FINDINGS findings, are explained by the host walk
KAFKA_EXPLAIN_TABLE_BOUND, KAFKA_EXPLAIN_MAX_FINDINGS = 384, 1024
# unique_explain_kernel's capacity (MSIM_UNIQUE_EXPLAIN_MAX_DUPS: a history of more duplicated ids is explained by the host walk) and
# pn_explain_kernel's (csrc/pn_check_dev.hip: a window of acceptable values this wide, or wider, is the host walk's)
UNIQUE_EXPLAIN_MAX_DUPS, PN_EXPLAIN_WINDOW = 1024, 4096


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("workload", C.c_uint32),
        ("node_program", C.c_uint32), ("n_nodes", C.c_uint32), ("concurrency", C.c_uint32),
        ("rate_mhz", C.c_uint32), ("time_limit_ms", C.c_uint32), ("latency_mean_ms", C.c_uint32),
        ("latency_dist", C.c_uint32), ("p_loss_q32", C.c_uint32), ("topology", C.c_uint32),
        ("nemesis_mask", C.c_uint32), ("nemesis_interval_ms", C.c_uint32), ("client_timeout_ms", C.c_uint32),
        ("quiesce_ms", C.c_uint32), ("seed", C.c_uint64), ("max_values", C.c_uint32), ("max_rows", C.c_uint32),
        ("max_payload_words", C.c_uint32), ("inbox_capacity", C.c_uint32), ("spill_capacity", C.c_uint32),
        ("journal_capacity", C.c_uint32), ("key_count", C.c_uint32), ("max_txn_length", C.c_uint32),
        ("max_writes_per_key", C.c_uint32), ("proxy_service", C.c_uint32), ("consistency_model", C.c_uint32), ("replication_words", C.c_uint32),
    ]


class Op(C.Structure):
    _fields_ = [("time_len", C.c_uint64), ("packed", C.c_uint32), ("value", C.c_uint32)]


class NetStats(C.Structure):
    _fields_ = [("all_send", C.c_uint64), ("all_recv", C.c_uint64), ("clients_send", C.c_uint64),
                ("clients_recv", C.c_uint64), ("servers_send", C.c_uint64), ("servers_recv", C.c_uint64)]


class InstMeta(C.Structure):
    _fields_ = [("n_rows", C.c_uint32), ("n_payload_words", C.c_uint32), ("flags", C.c_uint32), ("n_rounds", C.c_uint32),
                ("n_events", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class Event(C.Structure):
    _fields_ = [("time_us", C.c_uint32), ("msg", C.c_uint32), ("a", C.c_uint32), ("route", C.c_uint32)]


class CheckResult(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("attempt_count", C.c_uint32), ("stable_count", C.c_uint32),
                ("lost_count", C.c_uint32), ("never_read_count", C.c_uint32), ("stale_count", C.c_uint32),
                ("duplicated_count", C.c_uint32), ("error_count", C.c_uint32), ("stable_latency_ms", C.c_uint32 * 5),
                ("op_count", C.c_uint32), ("ok_count", C.c_uint32), ("fail_count", C.c_uint32), ("info_count", C.c_uint32)]


class DeviceBuffers(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("payload", C.c_void_p), ("stats", C.c_void_p), ("meta", C.c_void_p),
                ("check", C.c_void_p), ("journal", C.c_void_p),
                ("rows_bytes", C.c_uint64), ("payload_bytes", C.c_uint64), ("stats_bytes", C.c_uint64),
                ("meta_bytes", C.c_uint64), ("check_bytes", C.c_uint64), ("journal_bytes", C.c_uint64),
                ("n_instances", C.c_uint32), ("max_rows", C.c_uint32),
                ("max_payload_words", C.c_uint32), ("journal_capacity", C.c_uint32)]


class Availability(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("ok_fraction", C.c_float), ("ok_count", C.c_uint32), ("invoke_count", C.c_uint32)]


class LatencyDist(C.Structure):
    _fields_ = [("count", C.c_uint32), ("q_us", C.c_uint32 * 5), ("sum_us", C.c_uint64)]


class FStats(C.Structure):
    _fields_ = [("f", C.c_uint32), ("valid", C.c_uint32), ("count", C.c_uint32), ("ok_count", C.c_uint32), ("fail_count", C.c_uint32),
                ("info_count", C.c_uint32), ("unpaired", C.c_uint32), ("reserved", C.c_uint32), ("latency", LatencyDist * 3)]


class PerfResult(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("n_f", C.c_uint32), ("count", C.c_uint32), ("ok_count", C.c_uint32), ("fail_count", C.c_uint32),
                ("info_count", C.c_uint32), ("open_count", C.c_uint32), ("flags", C.c_uint32), ("by_f", FStats * PERF_MAX_F)]


class LinKeyResult(C.Structure):
    _fields_ = [("key", C.c_uint32), ("valid", C.c_uint32), ("op_row", C.c_uint32), ("previous_ok_row", C.c_uint32),
                ("n_pending", C.c_uint32), ("n_values", C.c_uint32), ("values", C.c_uint8 * 8)]


class Gathered(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("payload", C.c_void_p), ("meta", C.c_void_p), ("stats", C.c_void_p),
                ("rows_bytes", C.c_uint64), ("payload_bytes", C.c_uint64), ("meta_bytes", C.c_uint64), ("stats_bytes", C.c_uint64),
                ("bytes_received", C.c_uint64), ("n_instances", C.c_uint32), ("world", C.c_uint32), ("rank", C.c_uint32), ("ms", C.c_float)]

class CycleResult(C.Structure):
    _fields_ = [("anomalies", C.c_uint32), ("length", C.c_uint32), ("n_steps", C.c_uint32), ("reserved", C.c_uint32)]


class CycleStep(C.Structure):
    _fields_ = [("txn", C.c_uint32), ("inv_row", C.c_uint32), ("cmp_row", C.c_uint32), ("kinds", C.c_uint32)]


class SetElement(C.Structure):
    _fields_ = [("element", C.c_uint32), ("outcome", C.c_uint32), ("latency_ms", C.c_uint32), ("known_row", C.c_uint32),
                ("last_present_row", C.c_uint32), ("last_absent_row", C.c_uint32)]


class SetExplain(C.Structure):
    _fields_ = [("n_lost", C.c_uint32), ("n_never_read", C.c_uint32), ("n_stale", C.c_uint32), ("truncated", C.c_uint32),
                ("n_worst_stale", C.c_uint32), ("lost_latency_ms", C.c_uint32 * 5), ("worst_stale", SetElement * 8)]


class KafkaFinding(C.Structure):
    _fields_ = [("anomaly", C.c_uint32), ("key", C.c_uint32), ("offset", C.c_uint32), ("value", C.c_uint32), ("other", C.c_uint32),
                ("row_a", C.c_uint32), ("row_b", C.c_uint32), ("reserved", C.c_uint32)]


class KafkaExplain(C.Structure):
    _fields_ = [("n_findings", C.c_uint32), ("truncated", C.c_uint32), ("count", C.c_uint32 * 10)]


class PnRead(C.Structure):
    _fields_ = [("row", C.c_uint32), ("value", C.c_int32), ("process", C.c_uint32), ("in_set", C.c_uint32)]


class PnRange(C.Structure):
    _fields_ = [("lower", C.c_int64), ("upper", C.c_int64)]


class PnExplain(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("n_ranges", C.c_uint32), ("truncated", C.c_uint32), ("reserved", C.c_uint32), ("definite_sum", C.c_int64)]


class UniqueDup(C.Structure):
    _fields_ = [("id", C.c_uint32), ("count", C.c_uint32), ("first_row", C.c_uint32), ("second_row", C.c_uint32)]


class UniqueExplain(C.Structure):
    _fields_ = [("n_dups", C.c_uint32), ("truncated", C.c_uint32)]


class EchoError(C.Structure):
    _fields_ = [("invoke_row", C.c_uint32), ("complete_row", C.c_uint32), ("expected", C.c_uint32), ("received", C.c_uint32)]


class EchoExplain(C.Structure):
    _fields_ = [("n_errors", C.c_uint32), ("truncated", C.c_uint32)]


class TxnFinding(C.Structure):
    _fields_ = [("anomaly", C.c_uint32), ("key", C.c_uint32), ("inv_row", C.c_uint32), ("cmp_row", C.c_uint32), ("mop", C.c_uint32),
                ("other_inv_row", C.c_uint32), ("other_cmp_row", C.c_uint32), ("other_mop", C.c_uint32),
                ("element", C.c_uint32), ("other_element", C.c_uint32), ("count", C.c_uint32), ("reserved", C.c_uint32)]


class TxnExplain(C.Structure):
    _fields_ = [("n_findings", C.c_uint32), ("truncated", C.c_uint32), ("count", C.c_uint32 * 12), ("reserved", C.c_uint32 * 2)]


class JournalMsg(C.Structure):
    _fields_ = [("id", C.c_uint32), ("send_event", C.c_uint32), ("recv_event", C.c_uint32), ("send_time_us", C.c_uint32),
                ("latency_us", C.c_uint32), ("kind", C.c_uint32), ("route", C.c_uint32), ("a", C.c_uint32)]


class JournalSummary(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("n_events", C.c_uint32), ("flags", C.c_uint32), ("n_msgs", C.c_uint32),
                ("send_count", C.c_uint32 * 3), ("recv_count", C.c_uint32 * 3), ("msg_count", C.c_uint32 * 3), ("undelivered", C.c_uint32 * 3),
                ("dup_sends", C.c_uint32), ("orphan_recvs", C.c_uint32), ("extra_recvs", C.c_uint32), ("n_nodes", C.c_uint32),
                ("client_slots", C.c_uint32), ("reserved", C.c_uint32 * 3), ("endpoints", C.c_uint32 * 8), ("latency", LatencyDist * 2)]


# The one table of records: the header's struct name -> its Structure, field names and order as in include/maelsim.h.  engine.py derives
# the numpy dtypes from these (np.dtype(Structure)); tests/test_abi_tables.py compiles a probe against the header and compares every
# size and offset with both.
RECORDS = {
    "msim_config": Config, "msim_op": Op, "msim_net_stats": NetStats, "msim_event": Event, "msim_inst_meta": InstMeta,
    "msim_check_result": CheckResult, "msim_lin_key_result": LinKeyResult, "msim_cycle_result": CycleResult, "msim_cycle_step": CycleStep,
    "msim_set_element": SetElement, "msim_set_explain": SetExplain, "msim_availability": Availability, "msim_latency_dist": LatencyDist,
    "msim_f_stats": FStats, "msim_perf_result": PerfResult, "msim_device_buffers": DeviceBuffers, "msim_gathered": Gathered,
}

# The one table of prototypes: entry -> (restype, argtypes), every entry include/maelsim.h declares, in its order.  A pointer the callers
# fill from a numpy array is a void pointer, so that an array's address (`.ctypes.data`, a plain int) is what every call site passes;
# tests/test_abi_tables.py holds arity, parameter classes and return classes to the header's declarations.
_P, _i, _u32, _u64, _sz, _f64, _f32, _vp, _s = C.POINTER, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_double, C.c_float, C.c_void_p, C.c_char_p
_res = _P(CheckResult)
_offsets_args = (_i, _vp, _vp, _vp, _vp, _u32)   # device, rows, row_offsets, payload, payload_offsets, n_histories
_classify = (_i, _offsets_args + (_u32, _vp, _vp))   # ... consistency_model / concurrency, out, n_host
_slab = (_i, (_i, _vp, _vp, _u32, _u32, _vp))   # device, rows, n_rows, max_rows, n_histories, out
_explain_rows = (_i, (_vp, _u32, _vp, _u32, _u32, _res, _vp, _vp, _u32))
_explain_batch = (_i, _offsets_args + (_u32, _vp, _vp, _vp, _vp, _u32))
_set_full_args = (_i, _u32, _u32, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp)
PROTOTYPES = {
    "msim_abi_version": (_u32, ()),
    "msim_device_count": (_i, ()),
    "msim_config_defaults": (_i, (_P(Config), _u32, _u32)),
    "msim_config_finalize": (_i, (_P(Config), _s, _sz)),
    "msim_create": (_i, (_P(Config), _i, _P(_vp), _s, _sz)),
    "msim_run": (_i, (_vp, _u64, _u32)),
    "msim_run_async": (_i, (_vp, _u64, _u32, _vp)),
    "msim_check": (_i, (_vp,)),
    "msim_set_check_classify": (_i, (_vp, _u32)),
    "msim_set_dev_flags": (_i, (_vp, _u32)),
    "msim_check_host_rechecks": (_u32, (_vp,)),
    "msim_check_txn_batch": (_i, _offsets_args + (_vp,)),
    "msim_classify_txn_batch": _classify,
    "msim_check_rw_batch": _classify,
    "msim_classify_rw_batch": _classify,
    "msim_check_pn_batch": _slab,
    "msim_check_set_full_batch": (_i, _set_full_args),
    "msim_check_kafka_rows": (_i, (_vp, _u32, _vp, _u32, _res)),
    "msim_check_kafka_batch": _classify,
    "msim_classify_kafka_batch": _classify,
    "msim_check_unique_batch": _slab,
    "msim_check_lin_kv_batch": (_i, (_i, _vp, _vp, _u32, _vp)),
    "msim_check_lin_kv_rows": (_i, (_vp, _u32, _res)),
    "msim_explain_lin_kv_rows": (_i, (_vp, _u32, _res, _vp, _u32, _P(_u32))),
    "msim_explain_lin_kv_batch": (_i, (_i, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _P(_u32))),
    "msim_explain_lin_kv": (_i, (_vp, _vp, _u32, _vp, _u32)),
    "msim_check_txn_rows": (_i, (_vp, _u32, _vp, _u32, _vp)),
    "msim_proscribed_anomalies": (_u32, (_u32,)),
    "msim_violated_anomalies": (_u32, (_u32, _u32)),
    "msim_check_rw_rows": (_i, (_vp, _u32, _vp, _u32, _u32, _vp)),
    "msim_explain_txn_rows": _explain_rows,
    "msim_explain_rw_rows": _explain_rows,
    "msim_explain_txn_batch": _explain_batch,
    "msim_explain_rw_batch": _explain_batch,
    "msim_explain_txn": (_i, (_vp, _vp, _vp, _u32, _u32)),
    "msim_explain_set_full_rows": (_i, (_u32, _vp, _u32, _vp, _u32, _res, _vp, _vp, _u32)),
    "msim_explain_set_full_batch": (_i, _set_full_args + (_vp, _vp, _u32)),
    "msim_explain_set_full": (_i, (_vp, _vp, _vp, _u32, _u32)),
    "msim_check_unique_rows": (_i, (_vp, _u32, _vp)),
    "msim_check_pn_rows": (_i, (_vp, _u32, _vp, _vp, _u32, _vp)),
    "msim_history_edn_rows": (_i, (_P(Config), _vp, _u32, _vp, _u32, _s, _sz, _P(_sz))),
    "msim_check_availability": (_i, (_vp, _u32, _f64, _P(Availability), _u32)),
    "msim_check_availability_rows": (_i, (_vp, _u32, _u32, _f64, _P(Availability))),
    "msim_check_perf": (_i, (_vp, _u32, _u32, _vp, _u32, _vp)),
    "msim_check_perf_rows": (_i, (_vp, _u32, _u32, _u32, _u32, _vp, _vp)),
    "msim_check_perf_batch": (_i, (_i, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp)),
    "msim_journal_fressian_rows": (_i, (_P(Config), _vp, _u32, _vp, _u32, _vp, _sz, _P(_sz))),
    "msim_fetch": (_i, (_vp,)),
    "msim_fetch_begin": (_i, (_vp,)),
    "msim_history": (_i, (_vp, _u32, _P(_P(Op)), _P(_u32), _P(_P(_u32)), _P(_u32))),
    "msim_net_stats_get": (_i, (_vp, _u32, _P(NetStats))),
    "msim_journal": (_i, (_vp, _u32, _P(_P(Event)), _P(_u32))),
    "msim_meta": (_i, (_vp, _u32, _P(InstMeta))),
    "msim_check_results": (_i, (_vp, _P(_P(CheckResult)), _P(_u32))),
    "msim_device_buffers_get": (_i, (_vp, _P(DeviceBuffers))),
    "msim_comm_unique_id": (_i, (_s,)),
    "msim_comm_init": (_i, (_vp, _s, _i, _i)),
    "msim_gather": (_i, (_vp, _i, _P(Gathered))),
    "msim_last_kernel_ms": (_i, (_vp, _P(_f32), _P(_f32))),
    "msim_get_config": (_i, (_vp, _P(Config))),
    "msim_selftest_wave": (_i, (_i,)),
    "msim_last_error": (_s, (_vp,)),
    "msim_destroy": (None, (_vp,)),
}
EXPORTS = list(PROTOTYPES)

# The same two tables for include/maelsim_kafka_explain.h (maelsim.h includes it): the explained kafka verdicts.  They stand beside
# RECORDS / PROTOTYPES, not in them, because those are held to maelsim.h's own text, declaration for declaration
# (tests/test_abi_tables.py); tests/test_kafka_explain.py holds these to their header the same way.
KAFKA_EXPLAIN_RECORDS = {"msim_kafka_finding": KafkaFinding, "msim_kafka_explain": KafkaExplain}
KAFKA_EXPLAIN_PROTOTYPES = {
    "msim_explain_kafka_rows": (_i, (_vp, _u32, _vp, _u32, _res, _vp, _vp, _u32)),
    "msim_explain_kafka_batch": (_i, _offsets_args + (_u32, _vp, _vp, _vp, _u32, _vp)),
    "msim_explain_kafka": (_i, (_vp, _vp, _vp, _u32, _u32)),
}

# ... and for include/maelsim_small_explain.h: the explained pn-counter / g-counter, unique-ids and echo verdicts
# (tests/test_small_explain.py holds these to their header).
SMALL_EXPLAIN_RECORDS = {"msim_pn_read": PnRead, "msim_pn_range": PnRange, "msim_pn_explain": PnExplain, "msim_unique_dup": UniqueDup,
                         "msim_unique_explain": UniqueExplain, "msim_echo_error": EchoError, "msim_echo_explain": EchoExplain}
_small_rows = (_i, (_vp, _u32, _res, _vp, _vp, _u32))
_small_batch = (_i, (_i, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp))
_small_ctx = (_i, (_vp, _vp, _vp, _u32, _u32))
SMALL_EXPLAIN_PROTOTYPES = {
    "msim_explain_pn_rows": _small_rows,
    "msim_explain_unique_rows": _small_rows,
    "msim_explain_echo_rows": (_i, (_vp, _u32, _u32, _res, _vp, _vp, _u32)),
    "msim_explain_pn_batch": _small_batch,
    "msim_explain_unique_batch": _small_batch,
    "msim_explain_echo_batch": (_i, (_i, _u32, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp)),
    "msim_explain_pn": _small_ctx,
    "msim_explain_unique": _small_ctx,
    "msim_explain_echo": _small_ctx,
}

# ... and for include/maelsim_journal.h: the net journal's messages (tests/test_journal_messages.py holds these to their header).
JOURNAL_TRUNCATED, JOURNAL_TABLE_TRUNCATED = 1, 2   # MSIM_JOURNAL_*
JOURNAL_WG = 256   # journal_messages_kernel's workgroup (csrc/journal_dev.hip): the events are swept in blocks of this many
JOURNAL_RECORDS = {"msim_journal_msg": JournalMsg, "msim_journal_summary": JournalSummary}
JOURNAL_PROTOTYPES = {
    "msim_journal_messages_rows": (_i, (_vp, _u32, _u32, _u32, _vp, _vp, _u32)),
    "msim_journal_messages_batch": (_i, (_i, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp)),
    "msim_journal_messages": (_i, (_vp, _vp, _vp, _u32, _u32)),
    "msim_journal_svg_rows": (_i, (_P(Config), _vp, _u32, _s, _sz, _P(_sz))),
}

# ... and for include/maelsim_txn_findings.h: a witness for every non-cycle anomaly of the transactional checkers
# (tests/test_txn_findings.py holds these to their header).
TXN_FINDINGS_CAPACITY = 1024   # MSIM_TXN_FINDINGS_CAPACITY: a history of more findings is explained by the host walk
TXN_FINDINGS_RECORDS = {"msim_txn_finding": TxnFinding, "msim_txn_explain": TxnExplain}
TXN_FINDINGS_PROTOTYPES = {
    "msim_explain_txn_findings_rows": (_i, (_u32, _vp, _u32, _vp, _u32, _u32, _res, _vp, _vp, _u32)),
    "msim_explain_txn_findings_batch": (_i, (_i, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u32)),
    "msim_explain_txn_findings": (_i, (_vp, _vp, _vp, _u32, _u32)),
}

_lib = None


def load():
    """Loads libmaelsim.so (built in-tree by maelstrom_amd.build / __graft_entry__.build) and gives every entry its prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -m maelstrom_amd.build` (hipcc, gfx950). "
                           "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**PROTOTYPES, **KAFKA_EXPLAIN_PROTOTYPES, **SMALL_EXPLAIN_PROTOTYPES, **JOURNAL_PROTOTYPES,
                                      **TXN_FINDINGS_PROTOTYPES}.items():
        fn = getattr(lib, name, None)   # MSIM_LIB may name an older build (the A/B tools under tools/ time the parent's): an entry it lacks is skipped, and calling it still raises
        if fn is not None:
            fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = lib
    return lib
