// launch_plan.h — how msim_run launches a configuration: two tables and one pure function (host only, included by engine.hip alone).
// MSIM_PACKED_LAYOUTS has a row per layout with several clusters per wavefront, in order of preference; MSIM_NODE_PROGRAMS a row per
// MSIM_NODE_* value: what a cluster of that program needs in HBM scratch and in LDS, and its one-cluster-per-wavefront kernels.
// msim_plan_launch() turns a configuration into the numbers of a launch.  A new node program is one row of the second table, a new
// packed layout one row of the first.  tools/launch_plan_dump.py prints both over a grid (tests/test_launch_plan.py pins the output).
#ifndef MSIM_LAUNCH_PLAN_H
#define MSIM_LAUNCH_PLAN_H
#include "sim_kernels.h"   // the layout constants of the one-cluster kernels
#include "layout_thresholds.h"

// engine.hip (internal like the launchers; they have external linkage so that tools/launch_plan_dump.cpp links against engine.hip's object)
uint32_t msim_mk_tcap(const msim_config &c), msim_mk_ccap(const msim_config &c), msim_raft_log_cap(const msim_config &c);

// ---- 1. The packed layouts (wave_common.h, where they are declared, says what each is)------------------------------------------------------------------------
// A launch takes the FIRST row that is eligible for the configuration, whose launch-size floor the batch meets (min_clusters,
// layout_thresholds.h; 0: none) and whose launcher does not answer MSIM_LAYOUT_DOES_NOT_FIT (the cluster state does not fit the
// layout's LDS); with no such row, one cluster per wavefront.  MSIM_DEV_FLAGS bit 9 skips the table, bit 10 ignores the floors.
// INVARIANT: apart from the pair duo / bcast8 (both simulate the fire-and-forget broadcast programs; duo goes first, under bit 15
// bcast8), at most ONE row is eligible for any configuration msim_config_finalize accepts: "first" is a preference within that pair
// only, and an instance's scratch holds the extra words of one row beside duo's.  tools/launch_plan_dump.cpp asserts it over its grid.
struct PackedLayout {
  const char *name;   // as `[layout] <name> <n>` prints it
  bool (*eligible)(const msim_config &);
  uint32_t (*min_clusters)(const msim_config &);
  uint64_t (*extra_scratch_words)(const msim_config &);   // behind the spill area: the layout keeps fewer envelopes in LDS
  hipError_t (*launch)(const KParams &, uint32_t, hipStream_t);
};
template <uint32_t FLOOR> static uint32_t msim_floor(const msim_config &) { return FLOOR; }
#define MSIM_PACKED_ROW(name_, floor_) {#name_, msim_##name_##_eligible, floor_, msim_##name_##_extra_scratch_words, msim_launch_##name_}
static const PackedLayout MSIM_PACKED_LAYOUTS[] = {
  MSIM_PACKED_ROW(duo, msim_floor<0>), MSIM_PACKED_ROW(bcast8, msim_floor<MSIM_BCAST8_MIN_CLUSTERS>),
  MSIM_PACKED_ROW(raft4, msim_floor<0>), MSIM_PACKED_ROW(svc4, msim_floor<MSIM_SVC4_MIN_CLUSTERS>),
  MSIM_PACKED_ROW(txng4, msim_floor<MSIM_TXNG4_MIN_CLUSTERS>), MSIM_PACKED_ROW(dtg4, msim_dtg4_min_clusters),
  MSIM_PACKED_ROW(txn8, msim_floor<0>), MSIM_PACKED_ROW(mk8, msim_floor<0>), MSIM_PACKED_ROW(dt8, msim_floor<MSIM_DT8_MIN_CLUSTERS>),
  MSIM_PACKED_ROW(hat8, msim_hat8_min_clusters), MSIM_PACKED_ROW(kafka8, msim_floor<MSIM_KAFKA8_MIN_CLUSTERS>),
  MSIM_PACKED_ROW(uid8, msim_floor<MSIM_UID8_MIN_CLUSTERS>), MSIM_PACKED_ROW(crdt8, msim_floor<MSIM_CRDT8_MIN_CLUSTERS>),
};
#undef MSIM_PACKED_ROW
static const PackedLayout &MSIM_DUO = MSIM_PACKED_LAYOUTS[0], &MSIM_BCAST8 = MSIM_PACKED_LAYOUTS[1];

// Queues the packed kernel for a launch of n clusters by the rule above and names it in *kname; MSIM_LAYOUT_DOES_NOT_FIT when no row
// took the launch (*duo_required_failed: duo was tried under bit 10 and the cluster state did not fit).
static inline hipError_t msim_launch_packed(const KParams &kp, uint32_t n, hipStream_t st, const char **kname, bool *duo_required_failed) {
  const msim_config &c = kp.cfg;
  *duo_required_failed = false;
  if (kp.dev_flags & 0x200u) return MSIM_LAYOUT_DOES_NOT_FIT;
  for (const PackedLayout &l : MSIM_PACKED_LAYOUTS) {
    if (!l.eligible(c) || (n < l.min_clusters(c) && !(kp.dev_flags & 0x400u))) continue;
    if (&l == &MSIM_DUO && (kp.dev_flags & 0x8000u) && MSIM_BCAST8.eligible(c)) continue;   // (bit 15: small clusters eight per wavefront instead)
    const hipError_t e = l.launch(kp, n, st);
    if (e != MSIM_LAYOUT_DOES_NOT_FIT) { *kname = l.launch == msim_launch_svc4 && c.node_program == MSIM_NODE_TSO_IDS ? "svc4<TSO>" : l.name; return e; }
    if (&l == &MSIM_DUO && (kp.dev_flags & 0x400u)) { *duo_required_failed = true; return e; }
  }
  return MSIM_LAYOUT_DOES_NOT_FIT;
}

// ---- 2. The node programs -----------------------------------------------------------------------------------------------------------
typedef hipError_t (*msim_launch1_fn)(const KParams &, uint32_t, size_t, hipStream_t);
struct Launcher1 { msim_launch1_fn fn; const char *name; };
struct NodeProgram {
  uint32_t id;         // MSIM_NODE_*: the row's index
  uint32_t services;   // service queues (and lanes) beside the nodes'
  uint64_t (*scratch_words)(const msim_config &);        // protocol scratch in front of the spill area
  uint64_t (*client_spill_words)(const msim_config &);   // scratch behind the spill area (null: none)
  size_t (*inbox_bytes)(const msim_config &, uint32_t services);    // LDS: the nodes', services' and clients' inboxes
  size_t (*state_bytes)(const msim_config &, uint32_t dev_flags);   // LDS: the protocol's state
  Launcher1 one, many, wide;   // one worker per node, several (concurrency > n_nodes), 33..127 nodes; {}: no such kernel
};
static inline uint32_t msim_slots(const msim_config &c) { return c.concurrency > c.n_nodes ? c.concurrency : c.n_nodes; }   // client worker slots (KParams::CS)
static inline bool msim_many(const msim_config &c) { return c.concurrency > c.n_nodes; }   // a lane per endpoint, a client inbox per worker slot
static inline uint64_t msim_set_words4(const msim_config &c) { return ((uint64_t)c.n_nodes * (c.max_values / 32) + 3) & ~3ull; }   // wide clusters: the nodes' sets

// protocol scratch words
static uint64_t ps_none(const msim_config &) { return 4; }
static uint64_t ps_bcast_ff(const msim_config &c) { return c.n_nodes > 32 ? 4 + msim_set_words4(c) : 4; }
// (wide clusters: 128-bit unacked masks per (node, value), the retry FIFO, the nodes' sets)
static uint64_t ps_bcast_ack(const msim_config &c) { return c.n_nodes > 32 ? (uint64_t)c.n_nodes * c.max_values * 6 + msim_set_words4(c) : c.node_program == MSIM_NODE_BCAST_ACK_RETRY ? (uint64_t)c.n_nodes * c.max_values * 3 : 4; }
// batched gossip: the nodes' u16 arrival logs, then 16 bytes per (node, peer) link (sim_kernel_general.inc g_log / g_link)
static uint64_t ps_bcast_batch(const msim_config &c) { return (uint64_t)c.n_nodes * (c.max_values / 2) + (uint64_t)c.n_nodes * c.n_nodes * 4; }
static uint64_t ps_crdt(const msim_config &c) {
  const uint64_t ticks = wide_crdt_ticks(c), w = ticks * c.n_nodes * (c.max_values / 32);
  // wide clusters: + the union of every tick's snapshots (wide_union_off: what a node that received all of a tick merges in one go), the
  // ticks' frequent elements and rare holders (sim_kernel_wide.inc SPARSE), the nodes' sets
  return c.n_nodes <= 32 ? w : ((w + ticks * (c.max_values / 32) + 3) & ~3ull) + (c.node_program == MSIM_NODE_G_SET ? wide_sparse_words(ticks, c.max_values / 32) : 0) + msim_set_words4(c);
}
static uint64_t ps_raft(const msim_config &c) { return (uint64_t)c.n_nodes * msim_raft_log_cap(c) * 2 + (uint64_t)c.n_nodes * R_ARENA_WORDS; }
static uint64_t ps_txn(const msim_config &c) { return (uint64_t)c.max_values * (c.max_writes_per_key + 1); }   // elements + counts per key
static uint64_t ps_mk(const msim_config &c) {   // elements, counts, map position, entry version, thunk counts, thunk versions + ids, the nodes' caches, the replica bytes
  return (uint64_t)c.max_values * (c.max_writes_per_key + 4 + 2 * (c.max_writes_per_key + 1)) + (uint64_t)c.n_nodes * msim_mk_ccap(c) + (uint64_t)c.n_nodes * msim_mk_tcap(c) / 4 + 4 +
         (uint64_t)c.n_nodes * ((msim_many(c) ? MKG_SLOTS : MK_SLOTS) - MK_SL) * mk_slot_words(8);   // + the transaction slots that are not in LDS (several workers per node: mkg_kernel<> has MKG_SLOTS)
}
static uint64_t ps_kafka(const msim_config &c) { return (uint64_t)KF_KEYS * (2 * (c.max_writes_per_key + 1) + 1); }   // the logs + the committed-offset lists of the keys
// registers per node + txn table + pending masks (bytes) + replicate lists
static uint64_t ps_hat(const msim_config &c) { const uint64_t G = c.max_rows / 2; return (uint64_t)c.n_nodes * c.max_values + 2 * G + ((uint64_t)c.n_nodes * G + 3) / 4 + c.replication_words; }
static uint64_t cs_svc(const msim_config &c) { return (uint64_t)msim_slots(c) * (R_CLIENT_CAP - PX_CL) * 4; }   // svc_kernel<>: the clients' inboxes beyond PX_CL envelopes
// LDS: inboxes of inbox_capacity envelopes per node and service, CLIENT_CAP per worker slot
template <uint32_t CLIENT_CAP> static size_t ib_queues(const msim_config &c, uint32_t services) { return ((size_t)(c.n_nodes + services) * c.inbox_capacity + (size_t)msim_slots(c) * CLIENT_CAP) * 16; }
template <uint32_t CLIENT_CAP> static size_t ib_wide(const msim_config &c, uint32_t services) { return ib_queues<CLIENT_CAP>(c, services) + wide_client_bytes(c); }   // (wide: + the pairs' client state)
// LDS: protocol state
static size_t st_sets(const msim_config &c, uint32_t dev_flags) {
  const size_t sets = (size_t)c.n_nodes * (c.max_values / 32) * 4;
  // the sets of a wide cluster live in HBM scratch unless they fit LDS (wide_sets_in_lds); + the CRDTs' delivered-but-unmerged replicates
  return c.n_nodes > 32 ? (wide_sets_in_lds(c, dev_flags) ? sets : 0) + wide_pending_bytes(c) : sets;
}
static size_t st_raft(const msim_config &c, uint32_t) { return (size_t)c.n_nodes * 256 + (size_t)c.n_nodes * c.n_nodes * 3 * 4; }   // KV state + next/match index + append_entries refs
// callbacks per node + service states (seq-kv: + its ring of 32) + seq-kv indices
static size_t st_svc(const msim_config &c, uint32_t) { return (size_t)c.n_nodes * PX_SLOTS * 8 + ((c.node_program == MSIM_NODE_LIN_KV_PROXY && c.proxy_service == MSIM_SVC_SEQ_KV) ? 34 : 2) * 256 + 64 * 4; }
static size_t st_txn(const msim_config &c, uint32_t) { return (size_t)c.n_nodes * (msim_many(c) ? TG_SLOTS : TXN_SLOTS) * 16 + 36 * 4; }   // transactions in flight per node + the generator's key pool
// transactions in flight (the first MK_SL per node), a round's messages per node, the generator's key pool
static size_t st_mk(const msim_config &c, uint32_t) { return ((size_t)c.n_nodes * MK_SL * mk_slot_words(mk_keys_for(c)) + (size_t)c.n_nodes * mk_keys_for(c) * 3 + 36) * 4; }
static size_t st_dt(const msim_config &c, uint32_t) { return ((size_t)c.n_nodes * (msim_many(c) ? DG_WORDS : DC_WORDS) + 36) * 4; }   // the nodes' transactions (lock holder, waiting queue, save stack), the generator's key pool
// request handlers, offset caches, client offsets (per worker slot), key pool, lin-kv lengths
static size_t st_kafka(const msim_config &c, uint32_t) { return ((size_t)c.n_nodes * (msim_many(c) ? KFG_SLOTS : KF_SLOTS) * KSW + (size_t)c.n_nodes * KF_KEYS + (size_t)msim_slots(c) * KF_KEYS + 36 + 2 * KF_KEYS) * 4; }
static size_t st_hat(const msim_config &, uint32_t) { return 36 * 4; }   // the generator's key pool

#define L1(name_) {msim_launch_##name_, #name_}
static const NodeProgram MSIM_NODE_PROGRAMS[] = {
  {MSIM_NODE_ECHO, 0, ps_none, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_a), {}, {}},
  {MSIM_NODE_BCAST_FF, 0, ps_bcast_ff, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_b), {}, L1(wide_bcast)},
  {MSIM_NODE_BCAST_FF_ECHOBACK, 0, ps_bcast_ff, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_b), {}, L1(wide_bcast)},
  {MSIM_NODE_BCAST_ACK_RETRY, 0, ps_bcast_ack, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_c), {}, L1(wide_ack)},
  {MSIM_NODE_BCAST_RPC_ALL, 0, ps_bcast_ack, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_c), {}, L1(wide_ack)},
  {MSIM_NODE_G_SET, 0, ps_crdt, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_a), {}, L1(wide_gset)},
  {MSIM_NODE_RAFT, 0, ps_raft, nullptr, ib_wide<R_CLIENT_CAP>, st_raft, L1(raft1), {}, {}},
  {MSIM_NODE_TXN_SINGLE_KEY, 1, ps_txn, nullptr, ib_queues<T_CLIENT_CAP>, st_txn, L1(txn1), L1(txng), {}},   // + the lin-kv lane
  {MSIM_NODE_PN_COUNTER, 0, ps_crdt, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_a), {}, L1(wide_pn)},
  {MSIM_NODE_FLAKE_IDS, 0, ps_none, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_a), {}, {}},
  {MSIM_NODE_LIN_KV_PROXY, 1, ps_none, cs_svc, ib_queues<PX_CL>, st_svc, L1(svc1), {}, {}},
  {MSIM_NODE_TXN_RW_HAT, 0, ps_hat, nullptr, ib_queues<T_CLIENT_CAP>, st_hat, L1(hat1), L1(hatg), {}},
  {MSIM_NODE_TXN_MULTI_KEY, 2, ps_mk, nullptr, ib_queues<T_CLIENT_CAP>, st_mk, L1(mk1), L1(mkg), {}},   // + lin-kv and lww-kv
  {MSIM_NODE_TSO_IDS, 1, ps_none, cs_svc, ib_queues<PX_CL>, st_svc, L1(svc1), {}, {}},   // the proxy's layout with the timestamp oracle on the service lane
  {MSIM_NODE_KAFKA, 1, ps_kafka, nullptr, ib_queues<T_CLIENT_CAP>, st_kafka, L1(kafka1), L1(kafkag), {}},
  {MSIM_NODE_TXN_DATOMIC, 2, dt_scratch_words, nullptr, ib_queues<T_CLIENT_CAP>, st_dt, L1(dt1), L1(dtg), {}},
  {MSIM_NODE_BCAST_BATCH, 0, ps_bcast_batch, nullptr, ib_wide<CLIENT_INBOX_CAP>, st_sets, L1(general_d), {}, {}},
};
#undef L1
static const uint32_t MSIM_N_NODE_PROGRAMS = sizeof MSIM_NODE_PROGRAMS / sizeof MSIM_NODE_PROGRAMS[0];
// the one-cluster-per-wavefront kernel of a configuration
static inline const Launcher1 &msim_one_cluster_launcher(const NodeProgram &p, const msim_config &c) {
  return p.wide.fn && c.n_nodes > 32 ? p.wide : p.many.fn && msim_many(c) ? p.many : p.one;
}

// ---- 3. The plan of a launch --------------------------------------------------------------------------------------------------------
struct LaunchPlan {
  int rc; const char *err;       // MSIM_OK, or why this configuration cannot be launched
  const NodeProgram *program;
  size_t lds;                    // of a one-cluster kernel: [row staging][off_inbox: inboxes][off_seen: protocol state][off_misc: nemesis shuffle scratch]
  KParams kp;                    // what of the kernels' parameters follows from the configuration; the pointers are the launch's to fill
                                 // (kp.scratch_words per instance: [protocol scratch][spill area: queues x spill_capacity envelopes][client spill][packed layouts])
};
static inline LaunchPlan msim_plan_launch(const msim_config &c, uint32_t dev_flags) {
  LaunchPlan p{};
  p.rc = MSIM_OK;
  KParams &kp = p.kp;
  kp.cfg = c; kp.dev_flags = dev_flags;
  kp.N = c.n_nodes; kp.C = c.concurrency; kp.CS = msim_slots(c); kp.W = c.max_values / 32;
  kp.cap_node = c.inbox_capacity; kp.spill_cap = c.spill_capacity;
  if (c.node_program >= MSIM_N_NODE_PROGRAMS || MSIM_NODE_PROGRAMS[c.node_program].id != c.node_program) { p.rc = MSIM_E_UNSUPPORTED; p.err = "node program not built into this engine"; return p; }
  const NodeProgram &np = *(p.program = &MSIM_NODE_PROGRAMS[c.node_program]);
  kp.spill_off = (np.scratch_words(c) + 3) & ~3ull;   // keep the spill area 16-byte aligned
  uint64_t w = kp.spill_off + (uint64_t)(c.n_nodes + np.services) * c.spill_capacity * 4 + (np.client_spill_words ? np.client_spill_words(c) : 0);
  for (const PackedLayout &l : MSIM_PACKED_LAYOUTS) if (&l != &MSIM_DUO && l.eligible(c)) w += l.extra_scratch_words(c);
  // duo.hip: the nodes' sets, last and on a 128-byte boundary of the instance's scratch (the total stays a multiple of 32 words)
  if (MSIM_DUO.eligible(c)) w = ((w + 31) & ~31ull) + MSIM_DUO.extra_scratch_words(c);
  kp.scratch_words = w;
  const uint64_t period_us = 1000000000ull / (c.rate_mhz ? c.rate_mhz : 1);
  if (2 * period_us > 0xFFFFFFFFull || 2000ull * c.nemesis_interval_ms > 0xFFFFFFFFull) { p.rc = MSIM_E_INVALID; p.err = "rate too low / nemesis interval too long for u32 microseconds"; return p; }
  kp.gen_period2_us = (u32)(2 * period_us); kp.nem_period2_us = (u32)(2000ull * c.nemesis_interval_ms);
  kp.raft_log_cap = c.node_program == MSIM_NODE_RAFT ? msim_raft_log_cap(c) : 0;
  kp.mk_tcap = c.node_program == MSIM_NODE_TXN_MULTI_KEY ? msim_mk_tcap(c) : c.node_program == MSIM_NODE_TXN_DATOMIC ? dt_tcap(c) : 0;
  kp.mk_ccap = c.node_program == MSIM_NODE_TXN_MULTI_KEY ? msim_mk_ccap(c) : 0;
  const bool wide = c.n_nodes > 32;
  // no row staging where a wide cluster keeps its sets in LDS, nor for the wide CRDTs (sim_kernel_wide.inc ROWS_DIRECT)
  const bool unstaged = wide_sets_in_lds(c, dev_flags) || (wide && (c.node_program == MSIM_NODE_G_SET || c.node_program == MSIM_NODE_PN_COUNTER));
  size_t off = unstaged ? 0 : (wide ? WIDE_STAGE_ROWS : STAGE_ROWS) * 16;
  kp.off_inbox = (u32)off; off += np.inbox_bytes(c, np.services);
  kp.off_seen = (u32)off; off += np.state_bytes(c, dev_flags);
  off = (off + 15) & ~(size_t)15;
  kp.off_misc = (u32)off; if (c.nemesis_mask) off += (wide ? 128 : 64) * 4;  // shuffle scratch, only the partition nemesis needs it
  p.lds = off;
  if (p.lds > 160 * 1024) { p.rc = MSIM_E_INVALID; p.err = "cluster state exceeds the 160 KiB LDS of a CU (lower inbox_capacity / max_values)"; }
  return p;
}
#endif
