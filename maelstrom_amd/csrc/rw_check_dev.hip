// rw_check_dev.hip — the rw-register analysis of txn-rw-register histories on the device (msim_check for MSIM_WL_TXN_RW_REGISTER;
// SURVEY.md §8f rank 1).  What the reference wires in at workload/txn_rw_register.clj:138-168 is [upstream] elle.rw-register through
// jepsen.tests.cycle.wr (:wfr-keys? true), judged by --consistency-models (core.clj:115-121: read-committed for the demo node);
// txn_check.cpp (check_rw) restates it on the host.
//
// The histories of the reference's own demo node (demo/clojure/txn_rw_register_hat.clj, "highly available transactions") are full of
// cycles the consistency model ALLOWS (G-single, G2, their realtime variants), so "prove the history clean or hand it to the host" —
// what txn_check_dev.hip does for list-append — would hand nearly everything over.  This pass instead proves, one wavefront per history,
// that NOTHING THE CONSISTENCY MODEL PROSCRIBES is present:
//   * the non-cycle anomalies exactly as the host finds them (duplicate writes, internal, G1a, G1b, cyclic version orders);
//   * the cycle anomalies by Kahn's algorithm over the edge kinds whose cycles the model proscribes: read-uncommitted ww (G0),
//     read-committed ww + wr (G0, G1c); the stronger models every kind (ww, wr, rw, and the realtime order for strict-serializable) —
//     there an acyclic graph is the only thing this pass can prove, anything else goes to the host.
// A history it cannot prove valid — a proscribed anomaly, a cycle in the subgraph — goes to rw_classify_kernel, which builds every
// edge kind, accumulates the non-cycle anomalies and classifies the cycles (G0 / G1c / G-single / G2, -realtime): the record of check_rw
// byte for byte.  Only a shape beyond the capacities below (values >= 64, the key / writer / transaction / edge tables, 64 open calls)
// and duplicate writes (check_rw's writer table is last-writer-wins in row order) are handed to check_rw on the host; a strongly connected
// component may be as large as the history (up to CCAP transactions a matrix in LDS, beyond it a search in HBM).  For a history the first pass does prove
// valid the result carries :valid? and the counts of the host's analysis, the non-cycle anomalies it saw (none of them proscribed) and the
// edges it built; its ALLOWED cycle classes are not searched for unless the caller asks for every history's full record
// (msim_classify_rw_batch, msim_set_check_classify).
//
// Steps (lane = transaction unless said otherwise), tables in an HBM workspace as in txn_check_kernel:
//   A  rows -> transactions, completions paired by process (txn_pairing.inc, shared with the list-append kernels);
//   B  key / value ranges; C  writer table (key, value) -> transaction by compare-and-swap, versions seen per key;
//   D  per :ok transaction: internal consistency, G1a / G1b, wr edges, "writes follow reads" version edges (64-bit sets by atomics);
//   E  per key (lane = key): nil precedes every version; a cyclic version order is found by peeling the versions without predecessor;
//      ww edges along the version order; rw edges from the external reads (stronger models only);
//   F  Kahn's algorithm over the edges built (txn_kahn.inc; the realtime order: txn_realtime.inc);  G (rw_classify_kernel only)  the cycle classes: cycle_classify.inc.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "check_run.h"
#include "check_dev.h"

namespace {

constexpr u32 NEEDS_HOST = 3u;
constexpr u32 NONE = 0xFFFFFFFFu;
constexpr u32 KMAX = 4096u;      // keys per history
constexpr u32 WMAX = 65536u;     // writer table entries (keys x values)

struct RParams {
  const msim_op *rows; const u32 *payload; const msim_inst_meta *meta;
  const uint64_t *row_off, *pay_off;   // (null: history i at i * max_rows / i * max_pay)
  msim_check_result *out;
  u32 *ws;                       // workspace, ws_words per history of this launch
  uint64_t ws_words;
  u32 max_rows, max_pay, nmax, emax, first, cm, proscribed;
  u32 kmax, wmax;                // keys / writer-table entries the workspace of a history holds (<= KMAX / WMAX: what the configuration can name)
  const u32 *list;               // rw_classify_kernel: the histories of this launch (block b takes list[first + b])
  u32 ccap;                      // rw_classify_kernel: transactions of one strongly connected component the reachability matrix holds (<= CCAP)
  u32 big;                       // rw_classify_kernel: a larger component is searched in the workspace (0: it is the host's, MSIM_DEV_FLAGS bit 13)
  msim_cycle_result *cycles; msim_cycle_step *steps; u32 max_steps;   // rw_explain_kernel: the witness cycles (history i's steps at steps + i * max_steps)
  msim_txn_explain *fhdr; msim_txn_finding *frecs; u32 max_findings;  // rw_findings_kernel: the non-cycle findings (history i's records at frecs + i * max_findings)
};

// one micro-op = one payload word: f (1 = write), key, value (0xFF: a read of nil)
#define M_F(w_) ((w_) & 1u)
#define M_KEY(w_) (((w_) >> 1) & 0x7FFFu)
#define M_VAL(w_) (((w_) >> 16) & 0xFFu)

#include "cycle_classify.inc"
#include "txn_findings.inc"


// FULL = false: the pass that proves a history free of what the model proscribes (rw_check_kernel).  FULL = true: the classification
// (rw_classify_kernel): every edge kind whatever the model is, the non-cycle anomalies accumulated, the cycles classified — the record
// of check_rw + finish + classify + judge (txn_check.cpp), field for field.  EXPLAIN (rw_explain_kernel, with FULL): and the witness cycle
// of the record's cycle class (cycle_classify.inc).  FINDINGS (rw_findings_kernel, with FULL): and a witness for every non-cycle anomaly
// (include/maelsim_txn_findings.h), emitted where the bits are set into the history's region behind `reach` (txn_findings.inc), sorted
// and written out before the cycles are classified; a history of more than MSIM_TXN_FINDINGS_CAPACITY findings is the host's.
template <bool FULL, bool EXPLAIN = false, bool FINDINGS = false>
__device__ __forceinline__ void rw_body(const RParams &p, const u32 hist) {
  const u32 lane = threadIdx.x;
  const u64 lt = (1ull << lane) - 1ull;
  HIST_VIEW(p, hist);
  const u32 NM = p.nmax;
  const bool strong = FULL || p.cm <= MSIM_CM_SNAPSHOT_ISOLATION;            // every edge kind counts
  const bool want_rt = FULL || p.cm == MSIM_CM_STRICT_SERIALIZABLE;
  const bool want_wr = FULL || p.cm != MSIM_CM_READ_UNCOMMITTED;
  u32 *const ws = p.ws + (u64)blockIdx.x * p.ws_words;
  u32 *const t_inv = ws, *const t_cmp = t_inv + NM, *const t_off = t_cmp + NM, *const t_lt = t_off + NM;   // t_lt: words | type << 16
  u32 *const t_first = t_lt + NM;            // transactions invoked before this one's completion row
  u32 *const sm = t_first + NM, *const smf = sm + NM + 1;
  u32 *const indeg = smf + NM + 1, *const off = indeg + NM;   // off [NM + 1]
  u32 *const cur = off + NM + 1, *const queue = cur + NM;
  u32 *const vseen = queue + NM;             // [kmax][2] versions of the key that exist (bit v; bit 0 = nil)
  u32 *const writer = vseen + 2 * p.kmax;    // [wmax]
  u32 *const vsucc = writer + p.wmax;        // [wmax][2] successors of (key, version) in the key's version order
  u32 *const adj = vsucc + 2 * p.wmax;       // [emax]
  // FULL only: the edges reversed (radj / roff / rcur), a transaction's state in the searches, the pivot search's pointers
  u32 *const radj = adj + p.emax, *const roff = radj + p.emax, *const rcur = roff + NM + 1, *const st = rcur + NM, *const jump = st + NM;
  // and a 64-bit word per transaction for the search of a component beyond the matrix [NM], on an 8-byte boundary
  [[maybe_unused]] u64 *const reach_ = reinterpret_cast<u64 *>((reinterpret_cast<uintptr_t>(jump + NM) + 7u) & ~(uintptr_t)7u);
  [[maybe_unused]] const FRegion F(reinterpret_cast<u32 *>(reach_ + NM));   // FINDINGS only

  BLANK_RESULT(res, NEEDS_HOST);
#define TO_HOST() do { if (lane == 0) p.out[hist] = res; return; } while (0)
  if (n_words >= (1u << 24)) TO_HOST();
  if constexpr (FINDINGS) { if (lane == 0) *F.cnt = 0; __syncthreads(); }

  // ---- A: transactions ---------------------------------------------------------------------------------------------------------
  u32 n = 0, c_ok = 0, c_fail = 0, c_info = 0, anomalies = 0;
  {
    bool o_used = false; u32 o_proc = 0, o_txn = 0, o_len = 0; bool bad = false;   // txn_pairing.inc's open calls
    for (u32 base = 0; base < n_rows; base += 64) {
      const u32 idx = base + lane;
      uint4 row = make_uint4(0, 0, 0, 0);
      if (idx < n_rows) row = r[idx];
      const u32 type = row.z & 3u, f = (row.z >> 2) & 31u, proc = row.z >> 12, len = row.y >> 16, woff = row.w;
      const bool txn_row = idx < n_rows && proc != MSIM_PROCESS_NEMESIS && f == MSIM_F_TXN;
      const bool outside = txn_row && (u64)woff + len > n_words;   // a payload outside its area: collect() skips the row and says internal
      if (__ballot(outside)) { if constexpr (FULL) anomalies |= MSIM_ANOMALY_INTERNAL; else { bad = true; break; } }
      if constexpr (FINDINGS) if (outside) f_emit(F, F_INTERNAL, NONE, NONE, NONE, idx, NONE, NONE, NONE, NONE, NONE, NONE, 0);
      const bool is = txn_row && !outside;
      const bool inv = is && type == MSIM_T_INVOKE;
      const u64 im = __ballot(inv);
      const u32 my_t = n + (u32)__popcll(im & lt);
      if (n + (u32)__popcll(im) > NM) { bad = true; break; }
      if (inv) { t_inv[my_t] = idx; t_cmp[my_t] = NONE; t_off[my_t] = woff; t_lt[my_t] = len | (MSIM_T_INFO << 16); t_first[my_t] = 0; }   // never completed = indeterminate
#include "txn_pairing.inc"
      if (bad) break;
      n += (u32)__popcll(im);
    }
    if (bad) TO_HOST();
  }
  __syncthreads();
  res.op_count = n; res.attempt_count = n; res.ok_count = c_ok; res.stable_count = c_ok; res.fail_count = c_fail; res.info_count = c_info;

  // ---- B: ranges, and the tables cleared ----------------------------------------------------------------------------------------------
  u32 max_key = 0, max_val = 0;
  for (u32 t = lane; t < n; t += 64) {
    const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
    for (u32 i = 0; i < wn; i++) { const u32 x = w[i]; max_key = max(max_key, M_KEY(x)); if (M_VAL(x) != 0xFFu) max_val = max(max_val, M_VAL(x)); }
  }
  max_key = wv_max(max_key); max_val = wv_max(max_val);
  const u32 stride = max_val + 1u;
  if (max_val >= 64u || max_key >= p.kmax || (u64)(max_key + 1u) * stride > p.wmax) TO_HOST();   // (check_rw answers :unknown for values >= 64)
  for (u32 k = lane; k <= max_key; k += 64) { vseen[2 * k] = 0; vseen[2 * k + 1] = 0; }
  for (u32 k = lane; k < (max_key + 1u) * stride; k += 64) { writer[k] = NONE; vsucc[2 * k] = 0; vsucc[2 * k + 1] = 0; }
  for (u32 t = lane; t <= n; t += 64) { off[t] = 0; if (t < n) { indeg[t] = 0; cur[t] = 0; if constexpr (FULL) rcur[t] = 0; } }
  __syncthreads();
#define TYPE(t_) (t_lt[t_] >> 16)
#define SETBIT(arr_, idx_, v_) atomicOr(&(arr_)[2 * (idx_) + ((v_) >> 5)], 1u << ((v_) & 31u))

  // ---- C: writers (every transaction, whatever became of it); versions written by transactions that did not fail -----------------------
  bool for_host = false;
  for (u32 t = lane; t < n; t += 64) {
    const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu; const bool failed = TYPE(t) == MSIM_T_FAIL;
    for (u32 i = 0; i < wn; i++) {
      const u32 x = w[i];
      if (!M_F(x)) continue;
      if (M_VAL(x) == 0xFFu) { for_host = true; continue; }    // (a write of nil: the generator has none; let the host say what it is)
      if (atomicCAS(&writer[M_KEY(x) * stride + M_VAL(x)], NONE, t) != NONE) for_host = true;   // duplicate writes: the generator never repeats (k, v); the host's writer table is last-writer-wins
      if (!failed) SETBIT(vseen, M_KEY(x), M_VAL(x));
    }
  }
  __syncthreads();
  if (__ballot(for_host)) TO_HOST();   // (duplicate writes are proscribed by every model)

  // the last value transaction t_ writes to key k_ (NONE: it does not write it)
  auto final_of = [&](u32 t_, u32 k_) -> u32 {
    const u32 *w = pay + t_off[t_]; const u32 wn = t_lt[t_] & 0xFFFFu; u32 v = NONE;
    for (u32 i = 0; i < wn; i++) { const u32 x = w[i]; if (M_F(x) && M_KEY(x) == k_) v = M_VAL(x); }
    return v;
  };
  [[maybe_unused]] auto final_mop = [&](u32 t_, u32 k_) -> u32 {   // FINDINGS: the micro-op of that write
    const u32 *w = pay + t_off[t_]; const u32 wn = t_lt[t_] & 0xFFFFu; u32 at = NONE;
    for (u32 i = 0; i < wn; i++) { const u32 x = w[i]; if (M_F(x) && M_KEY(x) == k_) at = i; }
    return at;
  };

  // ---- D/E: edges: pass 0 counts degrees (and finds the non-cycle anomalies), pass 1 fills the CSR ----------------------------------------
  u32 n_edges = 0;
  if (want_rt) {   // the realtime order in closed form
#include "txn_realtime.inc"
    __syncthreads();
  }
  for (int pass = 0; pass < 2; pass++) {
    u32 my_edges = 0;
#define ADD(a_, b_, kind_) do { const u32 ea = (a_), eb = (b_); if (ea != eb) { if (pass == 0) { atomicAdd(&off[ea], 1u); atomicAdd(&indeg[eb], 1u); my_edges++; } \
      else if constexpr (FULL) { adj[off[ea] + atomicAdd(&cur[ea], 1u)] = eb | ((kind_) << 28); radj[roff[eb] + atomicAdd(&rcur[eb], 1u)] = ea | ((kind_) << 28); } \
      else adj[off[ea] + atomicAdd(&cur[ea], 1u)] = eb; } } while (0)
    // per :ok transaction: the reads
    for (u32 t = lane; t < n; t += 64) {
      if (TYPE(t) != MSIM_T_OK) continue;
      const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
      for (u32 k = 0; k < wn; k++) {
        const u32 x = w[k];
        if (M_F(x)) continue;
        const u32 key = M_KEY(x), val = M_VAL(x); const bool nil = val == 0xFFu;
        // internal consistency: the latest earlier micro-op on this key decides what the read must return
        int prev = -1;
        for (u32 e = 0; e < k; e++) if (M_KEY(w[e]) == key) prev = (int)e;
        if (prev >= 0) {
          const u32 px = w[prev]; const bool pnil = M_VAL(px) == 0xFFu;
          const bool same = M_F(px) ? (!nil && val == M_VAL(px)) : (nil == pnil && (nil || val == M_VAL(px)));
          if (!same) anomalies |= MSIM_ANOMALY_INTERNAL;
          if constexpr (FINDINGS) if (!same && pass == 0)
            f_emit(F, F_INTERNAL, key, t, t_inv[t], t_cmp[t], k, t_inv[t], t_cmp[t], (u32)prev, nil ? NONE : val, (!M_F(px) && pnil) ? NONE : M_VAL(px), 0);
          continue;
        }
        // an external read
        if (!nil) {
          if (pass == 0) SETBIT(vseen, key, val);
          const u32 wr = writer[key * stride + val];
          if (wr == NONE || TYPE(wr) == MSIM_T_FAIL) {   // garbage / aborted read
            anomalies |= MSIM_ANOMALY_G1A;
            if constexpr (FINDINGS) if (pass == 0) f_emit(F, F_G1A, key, t, t_inv[t], t_cmp[t], k, wr == NONE ? NONE : t_inv[wr], wr == NONE ? NONE : t_cmp[wr], NONE, val, NONE, 0);
          } else {
            if (wr != t) {
              if (final_of(wr, key) != val) anomalies |= MSIM_ANOMALY_G1B;
              if constexpr (FINDINGS) if (pass == 0 && final_of(wr, key) != val)
                f_emit(F, F_G1B, key, t, t_inv[t], t_cmp[t], k, t_inv[wr], t_cmp[wr], final_mop(wr, key), val, final_of(wr, key), 0);
              if (want_wr) ADD(wr, t, E_WR);
            }
            const u32 fw = final_of(t, key);   // writes follow reads
            if (pass == 0 && fw != NONE && fw != val) SETBIT(vsucc, key * stride + val, fw);
          }
        }
      }
      if (want_rt) {
        const u32 first = t_first[t];                          // the transactions invoked after t completed start here ...
        const u32 last = sm[first] == NONE ? n : smf[first];   // ... and end where the first of them to complete :ok did
        for (u32 v = first; v < last; v++) if (TYPE(v) != MSIM_T_FAIL) ADD(t, v, E_RT);
      }
    }
    __syncthreads();
    if (pass == 0) {
      // nil precedes every version; cyclic version orders (lane = key): peel the versions that have no predecessor among those left
      for (u32 key = lane; key <= max_key; key += 64) {
        const u64 seen = (((u64)vseen[2 * key + 1] << 32) | vseen[2 * key]) & ~1ull;
        u64 alive = seen;   // (nil precedes everything and follows nothing: it never sits on a cycle)
        if constexpr (FULL) {   // as check_rw has it: nil's successors in the table, version 0 a version like any other
          vsucc[2 * (key * stride)] |= (u32)seen; vsucc[2 * (key * stride) + 1] |= (u32)(seen >> 32);
          alive = seen | 1ull;
        }
        while (alive) {
          u64 has_in = 0;
          for (u64 b = alive; b; b &= b - 1) { const u32 v = (u32)__builtin_ctzll(b); if (v < stride) has_in |= ((u64)vsucc[2 * (key * stride + v) + 1] << 32) | vsucc[2 * (key * stride + v)]; }
          const u64 roots = alive & ~has_in;
          if (!roots) {
            anomalies |= MSIM_ANOMALY_CYCLIC_VERSIONS;
            if constexpr (FINDINGS) {   // `alive` holds the cycles and what follows them: a version is on a cycle iff it reaches itself
              u32 lowest = NONE, on_cycle = 0;
              for (u64 b = alive; b; b &= b - 1) {
                const u32 v = (u32)__builtin_ctzll(b);
                u64 r = ((u64)vsucc[2 * (key * stride + v) + 1] << 32) | vsucc[2 * (key * stride + v)];
                for (bool grown = true; grown;) {
                  u64 more = 0;
                  for (u64 c = r; c; c &= c - 1) { const u32 u = (u32)__builtin_ctzll(c); if (u < stride) more |= ((u64)vsucc[2 * (key * stride + u) + 1] << 32) | vsucc[2 * (key * stride + u)]; }
                  grown = (more & ~r) != 0; r |= more;
                }
                if ((r >> v) & 1ull) { on_cycle++; lowest = min(lowest, v); }
              }
              f_emit(F, F_VERSIONS, key, NONE, NONE, NONE, NONE, NONE, NONE, NONE, lowest, NONE, on_cycle);
            }
            if constexpr (FULL) for (u32 v = 0; v < stride; v++) { vsucc[2 * (key * stride + v)] = 0; vsucc[2 * (key * stride + v) + 1] = 0; }   // the key contributes no ww and no rw edges
            break;
          }
          alive &= ~roots;
        }
      }
    }
    if constexpr (FULL) { if (pass == 0) __syncthreads(); }   // nil's successors and the cleared keys, written by the keys' lanes, are read by the transactions' lanes below
    if constexpr (!FULL) {
      if (__ballot((anomalies & p.proscribed) != 0)) TO_HOST();
      if (__ballot((anomalies & MSIM_ANOMALY_CYCLIC_VERSIONS) != 0)) TO_HOST();
    }
    // ww along the version order of every key (lane = key); nil has no writer
    for (u32 key = lane; key <= max_key; key += 64) {
      for (u32 v1 = 1; v1 < stride; v1++) {
        u64 su = ((u64)vsucc[2 * (key * stride + v1) + 1] << 32) | vsucc[2 * (key * stride + v1)];
        if (!su) continue;
        const u32 a = writer[key * stride + v1];
        if (a == NONE || TYPE(a) == MSIM_T_FAIL) continue;
        for (; su; su &= su - 1) {
          const u32 v2 = (u32)__builtin_ctzll(su);
          const u32 b = v2 < stride ? writer[key * stride + v2] : NONE;
          if (b != NONE && TYPE(b) != MSIM_T_FAIL) ADD(a, b, E_WW);
        }
      }
    }
    // rw: a transaction's first micro-op on a key, if it is a read of v1, precedes the writers of v1's successors
    if (strong) {
      for (u32 t = lane; t < n; t += 64) {
        if (TYPE(t) != MSIM_T_OK) continue;
        const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
        for (u32 k = 0; k < wn; k++) {
          const u32 x = w[k];
          if (M_F(x)) continue;
          const u32 key = M_KEY(x);
          bool first = true;
          for (u32 e = 0; e < k; e++) if (M_KEY(w[e]) == key) first = false;
          if (!first) continue;
          const u32 v1 = M_VAL(x) == 0xFFu ? 0u : M_VAL(x);
          u64 su = (v1 == 0 && !FULL) ? ((((u64)vseen[2 * key + 1] << 32) | vseen[2 * key]) & ~1ull)
                                      : (((u64)vsucc[2 * (key * stride + v1) + 1] << 32) | vsucc[2 * (key * stride + v1)]);
          for (; su; su &= su - 1) {
            const u32 v2 = (u32)__builtin_ctzll(su);
            const u32 b = v2 < stride ? writer[key * stride + v2] : NONE;
            if (b != NONE && TYPE(b) != MSIM_T_FAIL) ADD(t, b, E_RW);
          }
        }
      }
    }
#undef ADD
    __syncthreads();
    if (pass == 0) {
      n_edges = wv_sum(my_edges);
      if (n_edges > p.emax) TO_HOST();
      u32 carry = 0;   // out-degrees -> CSR offsets (exclusive prefix sums, 64 at a time)
      for (u32 base = 0; base <= n; base += 64) {
        const u32 t = base + lane;
        const u32 d = t < n ? off[t] : 0u;
        const u32 ex = wv_excl_scan(d, lane);
        if (t <= n) off[t] = carry + ex;
        carry += wv_sum(d);
      }
      if constexpr (FULL) {   // in-degrees -> offsets of the reversed edges
        carry = 0;
        for (u32 base = 0; base <= n; base += 64) {
          const u32 t = base + lane;
          const u32 d = t < n ? indeg[t] : 0u;
          const u32 ex = wv_excl_scan(d, lane);
          if (t <= n) roff[t] = carry + ex;
          carry += wv_sum(d);
        }
      }
      __syncthreads();
    }
  }
  anomalies = wv_or(anomalies);

  if constexpr (FINDINGS) { if (!f_finish(F, FOut{p.fhdr, p.frecs, p.max_findings}, hist)) TO_HOST(); }   // (more than the region holds: the host walk's)
  if constexpr (FULL) {
    u64 *const reach = reinterpret_cast<u64 *>((reinterpret_cast<uintptr_t>(jump + NM) + 7u) & ~(uintptr_t)7u);
    const CycleParams cp = {p.out, p.cm, p.proscribed, p.ccap, p.big};
    if constexpr (EXPLAIN) {
      const CycleWitness cw = {p.cycles, p.steps, p.max_steps, t_inv, t_cmp};
      cycle_classify<true>(cp, hist, res, anomalies, n, n_edges, flags, c_ok, indeg, off, adj, roff, radj, st, jump, queue, reach, &cw);
    } else cycle_classify(cp, hist, res, anomalies, n, n_edges, flags, c_ok, indeg, off, adj, roff, radj, st, jump, queue, reach);
    return;
  }
  // ---- F: acyclic?  Kahn's algorithm, 64 ready transactions per step ---------------------------------------------------------------------
#include "txn_kahn.inc"
  if (tail != n) TO_HOST();   // a cycle over edge kinds the model proscribes cycles of (or, for the stronger models, any cycle): the host classifies it

  if (lane == 0) {
    res.lost_count = n_edges;      // edges of the subgraph built
    res.error_count = anomalies;   // non-cycle anomalies seen (none of them proscribed)
    res.valid = flags ? 0u : (c_ok == 0 ? 2u : 1u);
    p.out[hist] = res;
  }
#undef TO_HOST
#undef TYPE
#undef SETBIT
}

__global__ void __launch_bounds__(64) rw_check_kernel(const RParams p) { rw_body<false>(p, p.first + blockIdx.x); }
__global__ void __launch_bounds__(64) rw_classify_kernel(const RParams p) { rw_body<true>(p, p.list[p.first + blockIdx.x]); }
__global__ void __launch_bounds__(64) rw_explain_kernel(const RParams p) { rw_body<true, true>(p, p.list[p.first + blockIdx.x]); }
__global__ void __launch_bounds__(64) rw_findings_kernel(const RParams p) { rw_body<true, false, true>(p, p.list[p.first + blockIdx.x]); }

uint64_t rw_ws_words(u32 nmax, u32 emax, u32 kmax, u32 wmax) { return (uint64_t)nmax * 11 + 4 + 2 * (uint64_t)kmax + 3 * (uint64_t)wmax + emax; }

uint64_t rw_ws_words_full(u32 nmax, u32 emax, u32 kmax, u32 wmax) { return rw_ws_words(nmax, emax, kmax, wmax) + emax + 6 * (uint64_t)nmax + 6; }   // (reach: 2 words each, 2 to align it)

// full: every history's record comes from the classification (msim_classify_rw_batch, msim_set_check_classify); otherwise only the
// records of the histories that rw_check_kernel could not prove valid do
int rw_dev_run(msim_ctx *ctx, RParams rp, u32 n, const std::vector<msim_inst_meta> *hmeta, msim_check_result *h_out, hipStream_t st, u32 *n_host,
               void **ws_buf, size_t *ws_cap, const CycleMode mode = {}) {
  // mode.witness (msim_explain_rw_batch, msim_explain_txn; with full): the witness cycles, found by rw_explain_kernel in rp.cycles / rp.steps
  CycleSlabs *const wit = mode.full ? mode.witness : nullptr;
  if (wit) { bind_cycles(rp, *wit); if (int rc = wit->clear(ctx, st)) return rc; }
  // mode.findings (msim_explain_txn_findings*; with full, without witness): the non-cycle findings, written by rw_findings_kernel
  FindingSlabs *const fnd = mode.full && !wit ? mode.findings : nullptr;
  if (fnd) { rp.fhdr = fnd->hdr(); rp.frecs = fnd->rec(); rp.max_findings = fnd->max_k; if (int rc = fnd->clear(ctx, st)) return rc; }
  const PassTimer tm(ctx);
  if (rp.kmax == 0 || rp.kmax > KMAX) rp.kmax = KMAX;
  if (rp.wmax == 0 || rp.wmax > WMAX) rp.wmax = WMAX;
  rp.ws_words = rw_ws_words(rp.nmax, rp.emax, rp.kmax, rp.wmax);
  const uint64_t budget = 6ull << 30;   // as many histories per launch as a few GB of workspace hold
  const auto for_host = [](u32 valid) { return valid == NEEDS_HOST; };
  // one pass of `kernel` over m histories (those of `list`, or all): chunked_pass with rp.ws_words of workspace each
  const auto pass = [&](u32 m, const std::vector<u32> *list, auto kernel) {
    return chunked_pass(ctx, m, rp.ws_words * 4, budget, list, ws_buf, ws_cap, [&](const u32 *d_list, void *ws, u32 first, u32 count) {
      rp.list = d_list; rp.ws = static_cast<u32 *>(ws); rp.first = first;
      hipLaunchKernelGGL(kernel, dim3(count), dim3(64), 0, st, rp);
    }, rp.out, h_out, n, st);
  };
  std::vector<u32> todo;
  int rc;
  if (!mode.full) {
    if ((rc = pass(n, nullptr, rw_check_kernel)) < 0) return rc;
    todo = needs(h_out, n, for_host);
    if (tm.trace) std::fprintf(stderr, "[rw-check] device pass (%u launches): %.2f ms, %zu of %u histories not proved valid\n", (u32)rc, tm.ms(), todo.size(), n);
  } else todo = needs(h_out, n, [](u32) { return true; });
  if (!todo.empty()) {   // the classification, over the list of histories that need it
    const u32 m = (u32)todo.size();
    rp.ws_words = rw_ws_words_full(rp.nmax, rp.emax, rp.kmax, rp.wmax) + (fnd ? FWORDS : 0u);   // (the region of findings behind `reach`)
    // MSIM_DEV_FLAGS bit 13: a tiny matrix and no search beyond it, so that tests reach the host; bit 17: a tiny matrix, so that small
    // histories reach the search
    rp.ccap = (msim_dev_flags(ctx) & 0x22000u) ? 16u : CCAP;
    rp.big = (msim_dev_flags(ctx) & 0x2000u) ? 0u : 1u;
    if ((rc = pass(m, &todo, fnd ? rw_findings_kernel : wit ? rw_explain_kernel : rw_classify_kernel)) < 0) return rc;
    todo = needs(h_out, n, for_host);
    if (tm.trace) std::fprintf(stderr, "[rw-check] cycle classes of %u histories (%u launches): done at %.2f ms, %zu for the host\n", m, (u32)rc, tm.ms(), todo.size());
  }
  if (wit && (rc = wit->fetch(ctx, st)) != MSIM_OK) return rc;
  if (fnd && (rc = fnd->fetch(ctx, st)) != MSIM_OK) return rc;
  if (!todo.empty()) {
    rc = hand_off(ctx, source_of(rp, hmeta), n, todo, h_out, rp.out, [&](const msim_op *rows, u32 nr, const u32 *pay, u32 nw, u32 flags, u32 i) {
      if (fnd) msim_txn_findings_instance_host(rows, nr, pay, nw, flags, rp.cm, &h_out[i], fnd->hdr(i), fnd->rec(i), fnd->max_k, true);
      else if (wit) msim_txn_explain_instance_host(rows, nr, pay, nw, flags, rp.cm, &h_out[i], wit->hdr(i), wit->rec(i), rp.max_steps, true);
      else msim_rw_check_instance_host(rows, nr, pay, nw, flags, rp.cm, &h_out[i]);
    });
    if (rc != MSIM_OK) return rc;
    if (tm.trace) std::fprintf(stderr, "[rw-check] host analysis of those: done at %.2f ms\n", tm.ms());
  }
  if (n_host) *n_host = (u32)todo.size();
  return MSIM_OK;
}

}  // namespace

// msim_check for txn-rw-register: the histories of the last run, where they lie in HBM.
// (cycles / steps / max_steps: msim_explain_txn's witness cycles with every history's full record, whatever msim_set_check_classify says)
static int rw_device(msim_ctx *ctx, msim_cycle_result *cycles, msim_cycle_step *steps, uint32_t max_steps, msim_txn_explain *fhdr, msim_txn_finding *frecs,
                     uint32_t max_findings) {
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const u32 n = ctx->n_inst;
  std::chrono::steady_clock::time_point t0;
  std::vector<msim_inst_meta> hm;
  if (int rc = begin_check(ctx, &t0, &hm)) return rc;
  RParams rp;
  std::memset(&rp, 0, sizeof rp);
  rp.rows = ctx->d_rows; rp.payload = ctx->d_payload; rp.meta = ctx->d_meta; rp.out = ctx->d_check;
  rp.max_rows = ctx->cfg.max_rows; rp.max_pay = ctx->cfg.max_payload_words;
  rp.nmax = ctx->cfg.max_rows / 2 + 1; rp.emax = rp.nmax * 16;
  rp.cm = ctx->cfg.consistency_model; rp.proscribed = msim_proscribed_anomalies(rp.cm);
  // a run names keys below max_values and values up to max-writes-per-key (<= 63): tables of that size instead of the 4096 x 16 a caller's
  // histories may need — 1 MB of workspace per history was four launches of 4096 for the demo shape, each waiting for its slowest history
  rp.kmax = ctx->cfg.max_values ? ctx->cfg.max_values : 1u;
  rp.wmax = (u32)std::min<uint64_t>(WMAX, (uint64_t)rp.kmax * (ctx->cfg.max_writes_per_key + 2u));
  CycleSlabs wit;
  if (cycles) if (int rc = wit.alloc(ctx, n, max_steps, cycles, steps)) return rc;
  FindingSlabs fnd;
  if (fhdr) if (int rc = fnd.alloc(ctx, n, max_findings, fhdr, frecs)) return rc;
  u32 redone = 0;
  int rc = rw_dev_run(ctx, rp, n, &hm, ctx->h_check, ctx->stream, &redone, &ctx->d_check_scratch, &ctx->cap_check_scratch,
                      CycleMode{ctx->check_classify || cycles || fhdr, cycles ? &wit : nullptr, fhdr ? &fnd : nullptr});
  if (rc != MSIM_OK) return rc;
  finish_check(ctx, t0, redone);
  return MSIM_OK;
}
int msim_check_rw_device(msim_ctx *ctx, msim_cycle_result *cycles, msim_cycle_step *steps, uint32_t max_steps) {
  return rw_device(ctx, cycles, steps, max_steps, nullptr, nullptr, 0);
}
int msim_rw_findings_device(msim_ctx *ctx, msim_txn_explain *hdr, msim_txn_finding *findings, uint32_t max_findings) {
  return rw_device(ctx, nullptr, nullptr, 0, hdr, findings, max_findings);
}

// Checks `n_histories` rw-register histories given on the host (rows / payload words of history i at row_offsets[i] /
// payload_offsets[i]) as msim_check does for the histories of a run.
static int rw_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                    uint32_t n_histories, uint32_t consistency_model, msim_check_result *out, uint32_t *n_host, bool full,
                    msim_cycle_result *cycles = nullptr, msim_cycle_step *steps = nullptr, uint32_t max_steps = 0,
                    msim_txn_explain *fhdr = nullptr, msim_txn_finding *frecs = nullptr, uint32_t max_findings = 0) {
  if (!rows || !row_offsets || !payload_offsets || !out || n_histories == 0 || consistency_model > MSIM_CM_READ_UNCOMMITTED) return MSIM_E_INVALID;
  BatchFrame<OffsetsBatch> f(device); msim_ctx *ctx = &f.ctx;
  if (int rc = f.begin(n_histories, sizeof(msim_check_result), rows, row_offsets, payload, payload_offsets, n_histories, 0x7FFFFFFFull)) return rc;
  DevBuf ws; size_t ws_cap = 0;
  CycleSlabs wit;
  if (cycles) if (int rc = wit.alloc(ctx, n_histories, max_steps, cycles, steps)) return rc;
  FindingSlabs fnd;
  if (fhdr) if (int rc = fnd.alloc(ctx, n_histories, max_findings, fhdr, frecs)) return rc;
  RParams rp;
  std::memset(&rp, 0, sizeof rp);
  f.bind(rp);
  rp.nmax = f.b.longest / 2 + 65; rp.emax = rp.nmax * 64; rp.cm = consistency_model;   // (a caller's histories may be dense: a few keys, reads of nil precede every version)
  rp.proscribed = msim_proscribed_anomalies(consistency_model);
  return rw_dev_run(ctx, rp, n_histories, nullptr, out, nullptr, n_host, ws.addr(), &ws_cap, CycleMode{full, cycles ? &wit : nullptr, fhdr ? &fnd : nullptr});
}
int msim_rw_findings_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets, uint32_t n_histories,
                           uint32_t consistency_model, msim_check_result *out, uint32_t *n_host, msim_txn_explain *hdr, msim_txn_finding *findings, uint32_t max_findings) {
  return rw_batch(device, rows, row_offsets, payload, payload_offsets, n_histories, consistency_model, out, n_host, true, nullptr, nullptr, 0, hdr, findings, max_findings);
}

extern "C" int msim_check_rw_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                                   uint32_t n_histories, uint32_t consistency_model, msim_check_result *out, uint32_t *n_host) {
  return rw_batch(device, rows, row_offsets, payload, payload_offsets, n_histories, consistency_model, out, n_host, false);
}

// As msim_check_rw_batch, but every record is the full one of msim_check_rw_rows: the histories the model accepts name their allowed
// cycle classes too.
extern "C" int msim_classify_rw_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                                      uint32_t n_histories, uint32_t consistency_model, msim_check_result *out, uint32_t *n_host) {
  return rw_batch(device, rows, row_offsets, payload, payload_offsets, n_histories, consistency_model, out, n_host, true);
}

// msim_classify_rw_batch with the witness cycles (rw_explain_kernel; include/maelsim.h msim_cycle_result).
extern "C" int msim_explain_rw_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                                     uint32_t n_histories, uint32_t consistency_model, msim_check_result *out, uint32_t *n_host,
                                     msim_cycle_result *cycles, msim_cycle_step *steps, uint32_t max_steps) {
  if (!cycles || !steps || max_steps == 0) return MSIM_E_INVALID;
  return rw_batch(device, rows, row_offsets, payload, payload_offsets, n_histories, consistency_model, out, n_host, true, cycles, steps, max_steps);
}

extern "C" int msim_set_check_classify(msim_ctx *ctx, uint32_t on) {
  if (!ctx) return MSIM_E_INVALID;
  if (ctx->cfg.workload != MSIM_WL_TXN_RW_REGISTER && ctx->cfg.workload != MSIM_WL_TXN_LIST_APPEND && ctx->cfg.workload != MSIM_WL_KAFKA) {
    ctx->err = "msim_set_check_classify: only txn-rw-register, txn-list-append and kafka have a classification"; return MSIM_E_UNSUPPORTED;
  }
  ctx->check_classify = on != 0;
  return MSIM_OK;
}
