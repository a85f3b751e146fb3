// kafka_check_dev.hip — the kafka checker on the device (msim_check for MSIM_WL_KAFKA), one workgroup per history.
//
// kafka_check.cpp restates the anomalies workload/kafka.clj:21-70 describes and runs on the host cores after the histories crossed
// PCIe (139 ms per 16384 histories of the bench shape, all of them clean).  This file does for it what txn_check_dev.hip does for the
// list-append analysis: the device PROVES a history free of every anomaly and then reports what the host reports for such a history
// (the op counts, sends attempted / acknowledged, the unobserved writes — "there is no recency requirement", :25-28 —, :valid?);
// anything else — an observation that disagrees with another one, a lost write, an aborted read, a process whose offsets do not
// strictly increase or jump over a known offset, a row that does not decode, an offset or message beyond the tables — is answered
// NEEDS_HOST and the host checker classifies it (kafka_dev_run below): never approximated.  A caller whose histories are not clean
// (msim_classify_kafka_batch, msim_set_check_classify) has them classified by kafka_classify_kernel instead, see there.  The two kernels
// are two instantiations of one body, kafka_body<MODE>; the third, kafka_explain_kernel, is the classification that keeps WHERE it set a
// bit (msim_explain_kafka_batch, msim_explain_kafka), see there.
//
// Layout.  The tables of kafka_check.cpp (the key's log as observed, where each message was seen, polled / acknowledged / failed
// flags) live in LDS, `T` entries per key (the configuration bounds offsets and messages by max-writes-per-key; a first pass over
// the launch's histories finds the highest one they name, kafka_bound_kernel: the bench shape needs 288 of the 1056 its configuration
// allows, 27 KB of LDS per history instead of 77):
//   pass 1  the workgroup's threads stride over the rows: every :ok send and every pair of every :ok poll is one observation — a
//           compare-and-swap on the log entry and one on the message's home, an atomic OR for the flags, an atomic max for the
//           highest polled offset of the key;
//   pass 1b threads stride over (key, offset): acknowledged and never polled -> lost if something above it was polled, else
//           unobserved; polled with a message whose send failed -> aborted read;
//   pass 2  a process's own sequence of offsets (:30-62).  A worker thread's processes follow one another in the history (a crash gives
//           the worker process + concurrency), so worker w's rows are one sequential stream: wavefront (w mod 4) walks the rows 64 at
//           a time, takes its workers' relevant rows in order (a ballot), and lane k holds key k's last polled / sent offset of the
//           worker in LDS; a poll's payload is staged into LDS with one coalesced load.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "check_run.h"
#include "check_dev.h"

namespace {

constexpr u32 NEEDS_HOST = 3u;
constexpr u32 EMPTY = 0xFFFFFFFFu;
constexpr u32 KEYS = 8u;          // kafka_check.cpp's bound (a poll block names its key in 3 bits)
constexpr u32 OFFS = 2048u;       // kafka_check.cpp's bound on offsets and messages
constexpr u32 NT = 512u, NWV = NT / 64u;   // (round 6: 256 -> 512 threads per history: 14.1 -> 10.0 ms per 16384 at the bench shape; 1024: 21.8)
constexpr u32 STAGE = 128u;       // payload words of a poll staged per wavefront (longer polls read the rest from HBM)
constexpr u32 CMAX = 64u;         // worker threads
constexpr u32 WST = 17u;          // per worker: last polled offset x 8, last sent offset x 8, current process

struct KCParams {
  const msim_op *rows; const u32 *payload; const msim_inst_meta *meta;
  const uint64_t *row_off, *pay_off;   // (null: history i at i * max_rows / i * max_pay)
  msim_check_result *out;
  u32 max_rows, max_pay;
  u32 T;      // table entries per key (a multiple of 32, <= OFFS)
  u32 C;      // worker threads: process p belongs to worker p mod C
};

// A poll's payload is a sequence of blocks: a header word (key, count, first offset), then the messages of offsets o0, o0 + 1, ...,
// two a word.  A block whose words run past the row's len does not decode.
struct PollBlock { u32 k, cnt, o0, words; };
__device__ __forceinline__ PollBlock poll_block(u32 h) { const u32 cnt = (h >> 8) & 0xFFu; return PollBlock{h & 7u, cnt, h >> 16, (cnt + 1) / 2}; }
__device__ __forceinline__ u32 block_msg(const u32 *w, u32 e) { return (w[e / 2] >> (16 * (e & 1))) & 0xFFFFu; }   // w: the block's first message word

size_t kafka_lds_bytes(u32 T) { return ((size_t)KEYS * T * 2 + 3 * (size_t)KEYS * T / 32 + KEYS + 16 + CMAX * WST + NWV * STAGE) * 4; }

// ---- the classification of unclean histories (msim_classify_kafka_batch, msim_set_check_classify) -------------------------------------
// kafka_check_kernel leaves at the first anomaly; a caller whose node is buggy then pays a PCIe copy and a host check per history.
// kafka_classify_kernel takes the histories that kernel answered NEEDS_HOST (`list`, compacted on the device) and writes the record
// check_kafka (kafka_check.cpp) writes, field for field: every MSIM_KAFKA_* bit, the lost / unobserved / duplicate counts.  An anomaly
// is never a reason to leave.  The host's record depends on the order of the observations in two places (observe() there): msg[k][o]
// keeps the LAST observation's message (only the aborted-read test reads the value), where[k][m] keeps the FIRST observation's offset
// and every later observation of m elsewhere marks ITS offset a duplicate.  So the table cells are ordered keys of 64 bits,
//   row index (31 bits) | ordinal of the observation inside its row (17 bits: a poll's len is 16 bits of words, two pairs a word) | value (11),
// written with an atomic max (msg, bit 63 = seen) and an atomic min (where): the order of the threads does not matter.
//   pass 1   every observation: the two ordered cells, the polled / acknowledged / failed bits, the key's highest polled offset;
//   pass 1'  the same observations again: m differs from the last message at (k, o) -> inconsistent-offsets (two different messages
//            at a cell: at least one differs from the last); o differs from m's first home -> a bit of dup_at (its popcount =
//            duplicated_count, duplicate iff non-zero);
//   pass 1b  acknowledged and never polled: lost below the key's highest polled offset, else unobserved; polled and the last message's
//            send failed: aborted-read;
//   pass 2   the walk of the worker streams, setting bits: nonmonotonic-send, (int-)nonmonotonic-poll, (int-)poll-skip (int-: the key
//            already had a block in this poll).
// Handed to the host checker (NEEDS_HOST, counted in n_host), and nothing else is:
//   * a row or poll block that does not decode, an :ok send of a key >= 8, an offset or message >= OFFS: the host's MALFORMED;
//   * a process that returns after a later process of its worker: not one stream per worker;
//   * an observation that names an offset or message >= TC_MAX = 1152: the cells take 128 bytes per offset, (132 T + 8544) bytes in all,
//     and a CU has 160 KB of LDS (T = 288 at the bench shape: 46 KB).
constexpr u32 TC_MAX = 1152u;
constexpr u64 SEEN = 1ull << 63;

size_t kafka_classify_lds_bytes(u32 T) { return (size_t)KEYS * T * 16 + (4 * (size_t)KEYS * T / 32 + KEYS + 16 + CMAX * WST + NWV * STAGE) * 4; }

// ---- the explanation of unclean histories (msim_explain_kafka_batch, msim_explain_kafka; include/maelsim.h, "kafka: the explanation of a
// verdict") ----------------------------------------------------------------------------------------------------------------------------
// kafka_explain_kernel is the classification (the same passes, the same record) that emits a finding wherever a bit is set:
//   pass 1   also keeps, per (key, offset), the lowest :ok send row and the lowest :ok poll row, per (key, message) the lowest :fail send
//            row (atomic minima of the row index);
//   pass 1'  also keeps, per (key, offset), the first observation whose message differs from the last one's and the first one whose
//            message has its home elsewhere (atomic minima of order << 11 | message, the cells' idiom), and marks the offset inconsistent;
//   pass 1b  one finding per lost offset, inconsistent offset, duplicate's other home and aborted read, read off those cells;
//   pass 2   a worker's state also holds the row that left each last polled / sent offset (WSTX = WST + 16 words), a skip counts the known
//            offsets it jumps over; one finding per nonmonotonic send, per block that does not advance, per block that skips.
// A finding is appended to the history's slab of the workspace in HBM (an atomic counter: wavefronts interleave).  Behind pass 2 the tables
// are dead: the workgroup writes the record, gathers the findings into LDS, sorts them by the contract's key (a bitonic network over the
// 512 threads, the slab padded with all-ones records to a power of two) and writes the first max_findings with the header.
// Capacities — a history beyond either is handed to the host walk (NEEDS_HOST, counted in n_host), as for the classification's reasons:
//   * TX_MAX = 384: an observation that names an offset or message from there on.  The explaining cells take (44 + 5/8) bytes per (key,
//     offset) — 357 per offset —, 149792 bytes in all at 384 of a CU's 163840 (T = 288 at the bench shape: 115520);
//   * FX_MAX = 1024 findings: what the sort holds (32 KB of the LDS the tables occupied; the smallest launch takes that much).
constexpr u32 TX_MAX = 384u, FX_MAX = 1024u;
constexpr u32 WSTX = WST + 16u;   // + the rows behind the last polled offset x 8, the last sent offset x 8
constexpr u32 HDRX = 32u;         // the explaining header: [11] findings emitted, [16 .. 25] findings per anomaly

struct KXOut {   // what kafka_explain_kernel writes beside p.out
  msim_kafka_explain *hdr; msim_kafka_finding *findings; u32 max_findings;
  uint4 *ws;     // FX_MAX findings (two uint4 each) per launched workgroup
};

size_t kafka_explain_lds_bytes(u32 T) {
  const size_t tables = (size_t)KEYS * T * (32 + 12) + (5 * (size_t)KEYS * T / 32 + KEYS + HDRX + CMAX * WSTX + NWV * STAGE) * 4;
  return std::max(tables, (size_t)FX_MAX * sizeof(msim_kafka_finding));
}

// ascending by (anomaly, key, offset, value, other, row_a, row_b, reserved): a = (a0, a1) before b
__device__ __forceinline__ bool finding_before(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  if (a0.x != b0.x) return a0.x < b0.x;
  if (a0.y != b0.y) return a0.y < b0.y;
  if (a0.z != b0.z) return a0.z < b0.z;
  if (a0.w != b0.w) return a0.w < b0.w;
  if (a1.x != b1.x) return a1.x < b1.x;
  if (a1.y != b1.y) return a1.y < b1.y;
  if (a1.z != b1.z) return a1.z < b1.z;
  return a1.w < b1.w;
}

// The one body of kafka_check_kernel (MODE 0: the first finding decides, the history is the host's), kafka_classify_kernel (MODE 1,
// CLASSIFY: every finding is a bit or a count of the record) and kafka_explain_kernel (MODE 2, CLASSIFY and EXPLAIN: and a record of
// `x`, through slab `slot` of the workspace).  The row loop, pass 1b's scan and pass 2's walk are the same; what a mode does with an
// observation and with a finding stands behind the switches.  `smem`: kafka_lds_bytes / kafka_classify_lds_bytes / kafka_explain_lds_bytes.
template <int MODE>
__device__ __forceinline__ void kafka_body(const KCParams &p, const u32 hist, unsigned char *const smem, const KXOut &x = KXOut{}, const u32 slot = 0) {
  constexpr bool CLASSIFY = MODE >= 1, EXPLAIN = MODE == 2;
  using Cell = std::conditional_t<CLASSIFY, unsigned long long, u32>;
  constexpr Cell UNSEEN = CLASSIFY ? 0u : EMPTY;          // msg of an offset never seen
  constexpr u32 BITMAPS = EXPLAIN ? 5u : CLASSIFY ? 4u : 3u;
  constexpr u32 WS = EXPLAIN ? WSTX : WST, HDRW = EXPLAIN ? HDRX : 16u;
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 T = p.T, KT = KEYS * T, C = p.C;
  // [KEYS][T] the key's log as observed.  Clean: the message (EMPTY: offset never seen).  CLASSIFY: SEEN | order | the message: the
  // max is the last observation (0: offset never seen)
  Cell *const msg = reinterpret_cast<Cell *>(smem);
  // [KEYS][T] by message.  Clean: 1 + the offset it was seen at.  CLASSIFY: order | the offset: the min is the first observation (~0: never seen)
  Cell *const where = msg + KT;
  // EXPLAIN, [KEYS][T] by offset, order | the message, minima (~0: none): the first observation that differs from the last one's message,
  // the first one whose message has its home elsewhere
  [[maybe_unused]] Cell *const fdiff = where + KT;
  [[maybe_unused]] Cell *const fdup = fdiff + KT;
  u32 *const polled = reinterpret_cast<u32 *>(where + (EXPLAIN ? 3u : 1u) * KT);   // [KEYS * T / 32] bits
  u32 *const acked = polled + KT / 32;
  u32 *const failed = acked + KT / 32;                    // by message: its send definitely failed
  u32 *const dup_at = failed + KT / 32;                   // CLASSIFY only, by offset: some message seen here has its first home elsewhere
  [[maybe_unused]] u32 *const incons = dup_at + KT / 32;  // EXPLAIN only, by offset: seen with two different messages
  u32 *const top1 = polled + BITMAPS * (KT / 32);         // [KEYS] 1 + the highest polled offset
  u32 *const hdr = top1 + KEYS;                           // [HDRW]: [0] the host's, [1..7] counters; CLASSIFY: [8] lost, [9] duplicates, [10] MSIM_KAFKA_* bits
  u32 *const wst = hdr + HDRW;                            // [CMAX][WS]
  u32 *const stg = wst + CMAX * WS + wave * STAGE;        // this wavefront's staging area
  // EXPLAIN, [KEYS][T] each, minima of the row index (EMPTY: none): the :ok sends of (key, offset), the :ok polls of it, the :fail sends of (key, message)
  [[maybe_unused]] u32 *const fack = wst + CMAX * WS + NWV * STAGE;
  [[maybe_unused]] u32 *const fpoll = fack + KT;
  [[maybe_unused]] u32 *const ffail = fpoll + KT;
  HIST_VIEW(p, hist);

  for (u32 i = tid; i < KT; i += NT) { msg[i] = UNSEEN; where[i] = CLASSIFY ? ~(Cell)0 : (Cell)0; }
  if constexpr (EXPLAIN) for (u32 i = tid; i < KT; i += NT) { fdiff[i] = ~(Cell)0; fdup[i] = ~(Cell)0; fack[i] = EMPTY; fpoll[i] = EMPTY; ffail[i] = EMPTY; }
  for (u32 i = tid; i < BITMAPS * KT / 32 + KEYS + HDRW; i += NT) polled[i] = 0;
  for (u32 i = tid; i < CMAX * WS; i += NT) wst[i] = EMPTY;
  __syncthreads();

#define TO_HOST() do { hdr[0] = 1u; } while (0)
#define SETBIT(a_, i_) atomicOr(&(a_)[(i_) >> 5], 1u << ((i_) & 31u))
#define GETBIT(a_, i_) (((a_)[(i_) >> 5] >> ((i_) & 31u)) & 1u)
  u32 bits = 0;
  // an anomaly: the clean pass proves nothing about such a history, the classification names it
  auto finding = [&](u32 bit) __attribute__((always_inline)) { if constexpr (CLASSIFY) bits |= bit; else TO_HOST(); };
  // EXPLAIN: the finding itself, appended to the workspace slab (more than the sort holds: the host's)
  [[maybe_unused]] auto emit = [&](u32 bit, u32 key, u32 offset, u32 value, u32 other, u32 row_a, u32 row_b) __attribute__((always_inline)) {
    atomicAdd(&hdr[16u + (u32)__builtin_ctz(bit)], 1u);
    const u32 at = atomicAdd(&hdr[11], 1u);
    if (at >= FX_MAX) { TO_HOST(); return; }
    uint4 *const w = x.ws + ((size_t)slot * FX_MAX + at) * 2u;
    w[0] = make_uint4(bit, key, offset, value);
    w[1] = make_uint4(other, row_a, row_b, 0u);
  };
  [[maybe_unused]] auto row_of = [](u64 cell) __attribute__((always_inline)) { return (u32)(cell >> 28) & 0x7FFFFFFFu; };   // of SEEN | order << 11 | value
  // Clean: every observation of (key, offset, message) must agree with every other one (inconsistent offsets, duplicates: the host's).
  // CLASSIFY, `ord` = row index << 17 | ordinal inside the row: sweep 0 records the observation, sweep 1 compares it with what all of them left
  auto observe = [&](u32 sweep, u32 k, u32 o, u32 m, u64 ord) __attribute__((always_inline)) {
    if (k >= KEYS || o >= T || m >= T) { TO_HOST(); return; }
    if constexpr (!CLASSIFY) {
      const u32 was = atomicCAS(&msg[k * T + o], EMPTY, m);
      if (was != EMPTY && was != m) TO_HOST();
      const u32 home = atomicCAS(&where[k * T + m], 0u, o + 1u);
      if (home != 0u && home != o + 1u) TO_HOST();
    } else if (sweep == 0) {
      atomicMax(&msg[k * T + o], (unsigned long long)(SEEN | (ord << 11) | m));
      atomicMin(&where[k * T + m], (unsigned long long)((ord << 11) | o));
    } else {
      if ((u32)(msg[k * T + o] & 0x7FFull) != m) {
        bits |= MSIM_KAFKA_INCONSISTENT_OFFSETS;
        if constexpr (EXPLAIN) { SETBIT(incons, k * T + o); atomicMin(&fdiff[k * T + o], (unsigned long long)((ord << 11) | m)); }
      }
      if ((u32)(where[k * T + m] & 0x7FFull) != o) {
        SETBIT(dup_at, k * T + o);
        if constexpr (EXPLAIN) atomicMin(&fdup[k * T + o], (unsigned long long)((ord << 11) | m));
      }
    }
  };

  BLANK_RESULT(res, NEEDS_HOST);

  // ---- pass 1 (sweep 0): what exists, what was acknowledged, what was polled, which sends failed; CLASSIFY: and pass 1' (sweep 1) ----
  for (u32 sweep = 0; sweep < (CLASSIFY ? 2u : 1u); sweep++) {
    u32 c_inv = 0, c_ok = 0, c_fail = 0, c_info = 0, c_att = 0, c_stable = 0;
    for (u32 idx = tid; idx < n_rows; idx += NT) {
      const uint4 row = r[idx];
      const u32 type = row.z & 3u, f = (row.z >> 2) & 31u, proc = row.z >> 12;
      if (proc == MSIM_PROCESS_NEMESIS) continue;
      c_inv += type == MSIM_T_INVOKE; c_ok += type == MSIM_T_OK; c_fail += type == MSIM_T_FAIL; c_info += type == MSIM_T_INFO;
      if (f == MSIM_F_SEND) {
        const u32 k = row.w & 63u, m = (row.w >> 6) & 0x7FFu, o = row.w >> 17;
        if (type == MSIM_T_INVOKE) c_att++;
        else if (type == MSIM_T_OK) {
          if (o == 0x7FFu || k >= KEYS) { TO_HOST(); continue; }
          c_stable++;
          observe(sweep, k, o, m, (u64)idx << 17);
          if (sweep == 0 && o < T) { SETBIT(acked, k * T + o); if constexpr (EXPLAIN) atomicMin(&fack[k * T + o], idx); }
        } else if (type == MSIM_T_FAIL && sweep == 0) {
          if (k < KEYS && m < T) { SETBIT(failed, k * T + m); if constexpr (EXPLAIN) atomicMin(&ffail[k * T + m], idx); }
          // (CLASSIFY: a message beyond the tables is never the last one of a cell: such an observation is the host's)
          else if constexpr (!CLASSIFY) { if (k < KEYS && m < OFFS) TO_HOST(); }
        }
      } else if (f == MSIM_F_POLL && type == MSIM_T_OK) {
        const u32 len = row.y >> 16;
        if (len == 0) continue;
        if ((u64)row.w + len > n_words) { TO_HOST(); continue; }
        const u32 *const w = pay + row.w;
        u64 ord = (u64)idx << 17;
        for (u32 q = 0; q < len;) {
          const PollBlock b = poll_block(w[q++]);
          if (q + b.words > len) { TO_HOST(); break; }
          for (u32 e = 0; e < b.cnt; e++, ord++) {
            observe(sweep, b.k, b.o0 + e, block_msg(w + q, e), ord);
            if (sweep == 0 && b.o0 + e < T) {
              SETBIT(polled, b.k * T + b.o0 + e); atomicMax(&top1[b.k], b.o0 + e + 1u);
              if constexpr (EXPLAIN) atomicMin(&fpoll[b.k * T + b.o0 + e], idx);
            }
          }
          q += b.words;
        }
      }
    }
    if (sweep == 0) {
      atomicAdd(&hdr[1], c_inv); atomicAdd(&hdr[2], c_ok); atomicAdd(&hdr[3], c_fail); atomicAdd(&hdr[4], c_info);
      atomicAdd(&hdr[5], c_att); atomicAdd(&hdr[6], c_stable);
    }
    __syncthreads();
    // does not decode, or beyond the tables (clean: or any disagreement): the host's (pass 2 reads only payload that decodes).  Asked after
    // sweep 0 only: sweep 1 finds nothing sweep 0 did not, and behind its barrier pass 2 of a faster wavefront may already be writing hdr[0]
    if (sweep == 0 && hdr[0]) { if (tid == 0) p.out[hist] = res; return; }
  }

  // ---- pass 1b: lost / unobserved writes, aborted reads; CLASSIFY: the duplicates' offsets ----
  {
    u32 unobs = 0, lost = 0;
    for (u32 i = tid; i < KT; i += NT) {
      const u32 k = i / T, o = i - k * T;
      const bool pl = GETBIT(polled, i) != 0;
      if (GETBIT(acked, i) && !pl) { if (o + 1u < top1[k]) { lost++; finding(MSIM_KAFKA_LOST_WRITE); } else unobs++; }
      if (pl) { const Cell c = msg[i]; if (c != UNSEEN && GETBIT(failed, k * T + (CLASSIFY ? (u32)(c & 0x7FFull) : (u32)c))) finding(MSIM_KAFKA_ABORTED_READ); }
      if constexpr (EXPLAIN) {
        const u64 last = msg[i];
        const u32 lm = (u32)(last & 0x7FFull);
        if (GETBIT(acked, i) && !pl && o + 1u < top1[k]) {
          const u32 top = top1[k] - 1u, writer = fack[i];
          emit(MSIM_KAFKA_LOST_WRITE, k, o, (r[writer].w >> 6) & 0x7FFu, top, writer, fpoll[k * T + top]);
        }
        if (GETBIT(incons, i)) { const u64 d = fdiff[i]; emit(MSIM_KAFKA_INCONSISTENT_OFFSETS, k, o, lm, (u32)(d & 0x7FFull), row_of(d), row_of(last)); }
        if (GETBIT(dup_at, i)) {
          const u64 d = fdup[i], home = where[k * T + (u32)(d & 0x7FFull)];
          emit(MSIM_KAFKA_DUPLICATE, k, o, (u32)(d & 0x7FFull), (u32)(home & 0x7FFull), row_of(home), row_of(d));
        }
        if (pl && last != UNSEEN && GETBIT(failed, k * T + lm)) emit(MSIM_KAFKA_ABORTED_READ, k, o, lm, 0u, ffail[k * T + lm], fpoll[i]);
      }
    }
    if constexpr (CLASSIFY) {
      u32 dups = 0;
      for (u32 i = tid; i < KT / 32; i += NT) dups += (u32)__popc(dup_at[i]);
      if (lost) atomicAdd(&hdr[8], lost);
      if (dups) { bits |= MSIM_KAFKA_DUPLICATE; atomicAdd(&hdr[9], dups); }
    }
    atomicAdd(&hdr[7], unobs);
  }

  // ---- pass 2: every process's own sequence of offsets per key (lane k holds key k) ----
  for (u32 base = 0; base < n_rows; base += 64) {
    const u32 idx = base + lane;
    uint4 row = make_uint4(0, 0, 0, 0);
    if (idx < n_rows) row = r[idx];
    const u32 proc_l = row.z >> 12, type_l = row.z & 3u, f_l = (row.z >> 2) & 31u;
    const bool rel = idx < n_rows && proc_l != MSIM_PROCESS_NEMESIS && (proc_l % C) % NWV == wave &&
                     ((f_l == MSIM_F_ASSIGN && type_l == MSIM_T_INVOKE) || (f_l == MSIM_F_POLL && (type_l == MSIM_T_FAIL || type_l == MSIM_T_INFO)) ||
                      (type_l == MSIM_T_OK && (f_l == MSIM_F_SEND || f_l == MSIM_F_POLL)));
    u64 todo = __ballot(rel);
    while (todo) {
      const u32 j = (u32)__builtin_ctzll(todo);
      todo &= todo - 1;
      const u32 rz = wv_rl(row.z, j), rw = wv_rl(row.w, j), ry = wv_rl(row.y, j);
      const u32 type = rz & 3u, f = (rz >> 2) & 31u, proc = rz >> 12;
      u32 *const s = wst + (proc % C) * WS;   // EXPLAIN: [17 + k] / [25 + k] the row that left s[k] / s[8 + k]
      const u32 cur = s[16];
      if (cur != proc) {   // the worker's next process starts with nothing remembered; a process that RETURNS is not a worker's stream
        if (cur != EMPTY && proc < cur) TO_HOST();
        wv_fence();
        if (lane < 16) s[lane] = EMPTY; else if (lane == 16) s[16] = proc;
        wv_fence();
      }
      // the positions change: nothing is tracked across an assign, nor across a poll that failed or crashed (kafka_check.cpp)
      if (type != MSIM_T_OK) { if (lane < 8) s[lane] = EMPTY; continue; }
      if (f == MSIM_F_SEND) {
        const u32 k = rw & 63u, o = rw >> 17;
        if (k >= KEYS || o >= OFFS) continue;
        if (lane == k) {
          const u32 last = s[8 + k];
          if (last != EMPTY && o <= last) {
            finding(MSIM_KAFKA_NONMONOTONIC_SEND);
            if constexpr (EXPLAIN) emit(MSIM_KAFKA_NONMONOTONIC_SEND, k, o, (rw >> 6) & 0x7FFu, last, s[25 + k], base + j);
          }
          s[8 + k] = o;
          if constexpr (EXPLAIN) s[25 + k] = base + j;
        }
        continue;
      }
      const u32 len = ry >> 16;
      if (len == 0) continue;
      for (u32 q = lane; q < len && q < STAGE; q += 64) stg[q] = pay[rw + q];
      wv_fence();
      bool internal = false;   // this lane's key already had a block in this poll: what follows is judged as an internal error
      for (u32 q = 0; q < len;) {
        const PollBlock b = poll_block(q < STAGE ? stg[q] : pay[rw + q]);
        q++;
        if (q + b.words > len) break;
        [[maybe_unused]] const u32 q0 = q;   // the block's first message word
        q += b.words;
        if (!b.cnt) continue;
        // a block holds one run o0, o0 + 1, ...: it must start above the worker's last offset of the key and skip nothing known
        if (lane == b.k) {
          const u32 lp = s[b.k];
          if constexpr (!EXPLAIN) {
            if (lp != EMPTY) {
              if (b.o0 <= lp) finding(internal ? MSIM_KAFKA_INT_NONMONOTONIC_POLL : MSIM_KAFKA_NONMONOTONIC_POLL);
              else for (u32 o = lp + 1; o < b.o0; o++) if (o < T && msg[b.k * T + o] != UNSEEN) { finding(internal ? MSIM_KAFKA_INT_POLL_SKIP : MSIM_KAFKA_POLL_SKIP); break; }
            }
          } else if (lp != EMPTY) {
            if (b.o0 <= lp) {
              const u32 bit = internal ? MSIM_KAFKA_INT_NONMONOTONIC_POLL : MSIM_KAFKA_NONMONOTONIC_POLL;
              finding(bit);
              emit(bit, b.k, b.o0, (q0 < STAGE ? stg[q0] : pay[rw + q0]) & 0xFFFFu, lp, s[17 + b.k], base + j);
            } else {
              u32 skipped = 0;   // the known offsets strictly between (the offsets beyond the tables were never observed)
              for (u32 o = lp + 1; o < b.o0 && o < T; o++) skipped += msg[b.k * T + o] != UNSEEN;
              if (skipped) {
                const u32 bit = internal ? MSIM_KAFKA_INT_POLL_SKIP : MSIM_KAFKA_POLL_SKIP;
                finding(bit);
                emit(bit, b.k, b.o0, skipped, lp, s[17 + b.k], base + j);
              }
            }
          }
          s[b.k] = b.o0 + b.cnt - 1u;
          if constexpr (EXPLAIN) s[17 + b.k] = base + j;
          internal = true;
        }
      }
      wv_fence();   // (the staging area is rewritten by the next poll)
    }
  }
  if constexpr (CLASSIFY) { if (bits) atomicOr(&hdr[10], bits); }
  __syncthreads();

  if (tid == 0) {
    if (!hdr[0]) {
      res.op_count = hdr[1]; res.ok_count = hdr[2]; res.fail_count = hdr[3]; res.info_count = hdr[4];
      res.attempt_count = hdr[5]; res.stable_count = hdr[6]; res.never_read_count = hdr[7];
      if constexpr (CLASSIFY) { res.lost_count = hdr[8]; res.duplicated_count = hdr[9]; res.error_count = hdr[10]; }
      res.valid = (flags || (CLASSIFY && hdr[10])) ? 0u : ((hdr[6] == 0 && hdr[2] == 0) ? 2u : 1u);
    }
    p.out[hist] = res;
  }
  if constexpr (EXPLAIN) {
    // the tables and the header are dead behind this barrier: the findings come from the workspace into LDS, are sorted there and written
    const u32 handed = hdr[0], n_found = hdr[11], n_kind = tid < 10u ? hdr[16u + tid] : 0u;
    __syncthreads();
    if (handed) return;   // (the record says NEEDS_HOST: the host walk writes this history's header and findings)
    u32 n2 = 1;
    while (n2 < n_found) n2 <<= 1;   // (n_found <= FX_MAX, else handed)
    uint4 *const srt = reinterpret_cast<uint4 *>(smem);
    const uint4 *const w = x.ws + (size_t)slot * FX_MAX * 2u;
    for (u32 i = tid; i < n2; i += NT) {
      const bool real = i < n_found;
      srt[2 * i] = real ? w[2 * i] : make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
      srt[2 * i + 1] = real ? w[2 * i + 1] : make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
    }
    __syncthreads();
    for (u32 k = 2; k <= n2; k <<= 1)
      for (u32 j = k >> 1; j; j >>= 1) {
        for (u32 i = tid; i < n2; i += NT) {
          const u32 l = i ^ j;
          if (l > i) {
            const uint4 a0 = srt[2 * i], a1 = srt[2 * i + 1], b0 = srt[2 * l], b1 = srt[2 * l + 1];
            if (finding_before(b0, b1, a0, a1) == ((i & k) == 0)) { srt[2 * i] = b0; srt[2 * i + 1] = b1; srt[2 * l] = a0; srt[2 * l + 1] = a1; }
          }
        }
        __syncthreads();
      }
    const u32 n_out = min(n_found, x.max_findings);
    uint4 *const dst = reinterpret_cast<uint4 *>(x.findings + (size_t)hist * x.max_findings);
    for (u32 i = tid; i < 2u * n_out; i += NT) dst[i] = srt[i];
    u32 *const xh = reinterpret_cast<u32 *>(x.hdr + hist);
    if (tid < 10u) xh[2u + tid] = n_kind;   // (count[9]: a history that does not decode is the host's)
    if (tid == 0) { xh[0] = n_out; xh[1] = n_found > x.max_findings ? 1u : 0u; }
  }
#undef TO_HOST
#undef SETBIT
#undef GETBIT
}

__global__ void __launch_bounds__(NT) kafka_check_kernel(const KCParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  kafka_body<0>(p, blockIdx.x, smem);
}

// the histories the clean pass could not prove clean: list[0] = how many, list[1 ..] = which (in no particular order)
__global__ void __launch_bounds__(256) kafka_todo_kernel(const msim_check_result *out, u32 n, u32 *list) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i < n && out[i].valid == NEEDS_HOST) list[1u + atomicAdd(&list[0], 1u)] = i;
}

__global__ void __launch_bounds__(NT) kafka_classify_kernel(const KCParams p, const u32 *list) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  kafka_body<1>(p, list[blockIdx.x], smem);
}

__global__ void __launch_bounds__(NT) kafka_explain_kernel(const KCParams p, const u32 *list, const KXOut x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  kafka_body<2>(p, list[blockIdx.x], smem, x, blockIdx.x);
}

// The highest offset / message value any :ok send or poll of the launch names: sizes the tables (most tests use a fraction of what
// max-writes-per-key allows, and the LDS a history's tables take decides how many histories a CU works on at once).
__global__ void __launch_bounds__(NT) kafka_bound_kernel(const KCParams p, u32 *bound) {
  const u32 tid = threadIdx.x;
  HIST_VIEW(p, blockIdx.x);
  u32 hi = 0;
  for (u32 idx = tid; idx < n_rows; idx += NT) {
    const uint4 row = r[idx];
    const u32 type = row.z & 3u, f = (row.z >> 2) & 31u;
    if ((row.z >> 12) == MSIM_PROCESS_NEMESIS || type == MSIM_T_INVOKE) continue;
    if (f == MSIM_F_SEND) { hi = max(hi, (row.w >> 6) & 0x7FFu); if (type == MSIM_T_OK && (row.w >> 17) != 0x7FFu) hi = max(hi, row.w >> 17); }
    else if (f == MSIM_F_POLL && type == MSIM_T_OK) {
      const u32 len = row.y >> 16;
      if (len == 0 || (u64)row.w + len > n_words) continue;
      const u32 *const w = pay + row.w;
      for (u32 q = 0; q < len;) {
        const PollBlock b = poll_block(w[q++]);
        if (q + b.words > len) break;
        if (b.cnt) hi = max(hi, b.o0 + b.cnt - 1u);
        for (u32 e = 0; e < b.cnt; e++) hi = max(hi, block_msg(w + q, e));
        q += b.words;
      }
    }
  }
  hi = wv_max(hi);
  if ((tid & 63u) == 0 && hi) atomicMax(bound, hi);
}

// the caller's arrays of an explaining run: a header per history, max_findings records per history
struct KafkaExplainRun { msim_kafka_explain *hdr; msim_kafka_finding *findings; u32 max_findings; };

// classify: what kafka_check_kernel cannot prove clean goes to kafka_classify_kernel first, and only what THAT hands over to the host.
// xr: to kafka_explain_kernel instead, which also writes its findings; what it hands over is explained by the host walk.  A launch whose
// histories are all proved clean runs the two kernels of the plain check and nothing else.
int kafka_dev_run(msim_ctx *ctx, KCParams kp, u32 n, const std::vector<msim_inst_meta> *hmeta, msim_check_result *h_out, hipStream_t st, u32 *n_host,
                  bool classify = false, const KafkaExplainRun *xr = nullptr) {
  const PassTimer tm(ctx);
  u32 h_bound = 0;
  {   // tables no larger than the launch's histories need (kp.T: what the configuration / the checker's own bound allows)
    DevBuf bound;
    MSIM_HIP_TRY(ctx, bound.alloc(4));
    u32 *const d_bound = bound.get<u32>();
    MSIM_HIP_TRY(ctx, hipMemsetAsync(d_bound, 0, 4, st));
    hipLaunchKernelGGL(kafka_bound_kernel, dim3(n), dim3(NT), 0, st, kp, d_bound);
    MSIM_HIP_TRY(ctx, hipGetLastError());
    MSIM_HIP_TRY(ctx, hipMemcpyAsync(&h_bound, d_bound, 4, hipMemcpyDeviceToHost, st));
    MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
    const u32 t = ((h_bound + 1u + 31u) & ~31u);
    if (t < kp.T) kp.T = t < 32u ? 32u : t;
  }
  const size_t lds = kafka_lds_bytes(kp.T);
  if (lds > 64 * 1024) MSIM_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&kafka_check_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kafka_check_kernel, dim3(n), dim3(NT), lds, st, kp);
  MSIM_HIP_TRY(ctx, hipGetLastError());
  u32 n_unclean = 0;
  if (xr) {
    std::memset(xr->hdr, 0, (size_t)n * sizeof(msim_kafka_explain));
    const size_t f_bytes = (size_t)n * xr->max_findings * sizeof(msim_kafka_finding);
    if (f_bytes) std::memset(xr->findings, 0, f_bytes);
    MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_out, kp.out, (size_t)n * sizeof(msim_check_result), hipMemcpyDeviceToHost, st));
    MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
    n_unclean = (u32)needs(h_out, n, [](u32 valid) { return valid == NEEDS_HOST; }).size();
    if (n_unclean) {
      DevBuf list, ws;
      ExplainSlabs<msim_kafka_explain, msim_kafka_finding> xs;   // (on the device only now that some history is unclean)
      const u32 chunk = chunk_for(n_unclean, (uint64_t)FX_MAX * sizeof(msim_kafka_finding), 64ull << 20, msim_dev_flags(ctx));
      MSIM_HIP_TRY(ctx, list.alloc(((size_t)n + 1) * 4));
      if (int rc = xs.alloc(ctx, n, xr->max_findings, xr->hdr, xr->findings)) return rc;
      MSIM_HIP_TRY(ctx, ws.alloc((size_t)chunk * FX_MAX * sizeof(msim_kafka_finding)));
      u32 *const d_list = list.get<u32>();
      MSIM_HIP_TRY(ctx, hipMemsetAsync(d_list, 0, 4, st));
      if (int rc = xs.clear(ctx, st)) return rc;
      hipLaunchKernelGGL(kafka_todo_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, kp.out, n, d_list);
      MSIM_HIP_TRY(ctx, hipGetLastError());
      KCParams cp = kp;   // tables for what the launch names, up to what LDS holds beside the explaining cells
      cp.T = std::min(TX_MAX, std::max(32u, (h_bound + 1u + 31u) & ~31u));
      const size_t xlds = kafka_explain_lds_bytes(cp.T);
      if (xlds > 64 * 1024) MSIM_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&kafka_explain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)xlds));
      const KXOut x{xs.hdr(), xs.rec(), xr->max_findings, ws.get<uint4>()};
      hipError_t err;
      for_chunks(n_unclean, chunk, &err, [&](u32 first, u32 count) {   // (one workspace: the chunks follow one another on the stream)
        hipLaunchKernelGGL(kafka_explain_kernel, dim3(count), dim3(NT), xlds, st, cp, d_list + 1 + first, x);
      });
      MSIM_HIP_TRY(ctx, err);
      if (int rc = xs.fetch(ctx, st)) return rc;   // (waits: the buffers are freed with this block)
    }
  } else if (classify) {   // the histories not proved clean, listed on the device, each to a workgroup of kafka_classify_kernel
    DevBuf list;
    MSIM_HIP_TRY(ctx, list.alloc(((size_t)n + 1) * 4));
    u32 *const d_list = list.get<u32>();
    MSIM_HIP_TRY(ctx, hipMemsetAsync(d_list, 0, 4, st));
    hipLaunchKernelGGL(kafka_todo_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, kp.out, n, d_list);
    MSIM_HIP_TRY(ctx, hipGetLastError());
    MSIM_HIP_TRY(ctx, hipMemcpyAsync(&n_unclean, d_list, 4, hipMemcpyDeviceToHost, st));
    MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (n_unclean) {
      KCParams cp = kp;   // tables for what the launch names (the configuration's bound does not hold for an unclean history), up to what LDS holds
      cp.T = std::min(TC_MAX, std::max(32u, (h_bound + 1u + 31u) & ~31u));
      const size_t clds = kafka_classify_lds_bytes(cp.T);
      if (clds > 64 * 1024) MSIM_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&kafka_classify_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)clds));
      hipLaunchKernelGGL(kafka_classify_kernel, dim3(n_unclean), dim3(NT), clds, st, cp, d_list + 1);
      MSIM_HIP_TRY(ctx, hipGetLastError());
      MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));   // (the list is freed with this block)
    }
  }
  MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_out, kp.out, (size_t)n * sizeof(msim_check_result), hipMemcpyDeviceToHost, st));
  MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
  const std::vector<u32> todo = needs(h_out, n, [](u32 valid) { return valid == NEEDS_HOST; });
  if (tm.trace) {
    if (classify || xr) std::fprintf(stderr, "[kafka-check] device pass (%zu B of LDS per history): %.2f ms, %u of %u histories %s on the device, %zu of those for the host\n",
                                     lds, tm.ms(), n_unclean, n, xr ? "explained" : "classified", todo.size());
    else std::fprintf(stderr, "[kafka-check] device pass (%zu B of LDS per history): %.2f ms, %zu of %u histories for the host\n", lds, tm.ms(), todo.size(), n);
  }
  if (!todo.empty()) {
    const int rc = hand_off(ctx, source_of(kp, hmeta), n, todo, h_out, kp.out, [&](const msim_op *rows, u32 nr, const u32 *pay, u32 nw, u32 flags, u32 i) {
      if (xr) msim_kafka_explain_instance_host(rows, nr, pay, nw, flags, &h_out[i], &xr->hdr[i], xr->findings + (size_t)i * xr->max_findings, xr->max_findings);
      else msim_kafka_check_instance_host(rows, nr, pay, nw, flags, &h_out[i]);
    });
    if (rc != MSIM_OK) return rc;
    if (tm.trace) std::fprintf(stderr, "[kafka-check] host checker on those: done at %.2f ms\n", tm.ms());
  }
  if (n_host) *n_host = (u32)todo.size();
  return MSIM_OK;
}

// table entries per key that cover offsets / messages below `bound`
u32 kafka_table_entries(u32 bound) { const u32 t = (bound + 31u) & ~31u; return t < 32u ? 32u : (t > OFFS ? OFFS : t); }

}  // namespace

// msim_check for kafka: the histories of the last run, where they lie in HBM (xr: msim_explain_kafka's arrays).
static int kafka_device(msim_ctx *ctx, const KafkaExplainRun *xr) {
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const u32 n = ctx->n_inst;
  if (ctx->cfg.concurrency == 0 || ctx->cfg.concurrency > CMAX) return xr ? msim_explain_kafka_host(ctx, xr->hdr, xr->findings, xr->max_findings) : msim_check_kafka_host(ctx);
  std::chrono::steady_clock::time_point t0;
  std::vector<msim_inst_meta> hm;
  if (int rc = begin_check(ctx, &t0, &hm)) return rc;
  KCParams kp;
  std::memset(&kp, 0, sizeof kp);
  kp.rows = ctx->d_rows; kp.payload = ctx->d_payload; kp.meta = ctx->d_meta; kp.out = ctx->d_check;
  kp.max_rows = ctx->cfg.max_rows; kp.max_pay = ctx->cfg.max_payload_words;
  // a key takes max-writes-per-key sends before it is retired: its offsets and messages stay below that (+ slack: what exceeds the
  // tables goes to the host checker, whose own bound is 2048)
  kp.T = kafka_table_entries(ctx->cfg.max_writes_per_key + 8u);
  kp.C = ctx->cfg.concurrency;
  u32 redone = 0;
  int rc = kafka_dev_run(ctx, kp, n, &hm, ctx->h_check, ctx->stream, &redone, ctx->check_classify, xr);
  if (rc != MSIM_OK) return rc;
  finish_check(ctx, t0, redone);
  return MSIM_OK;
}
int msim_check_kafka_device(msim_ctx *ctx) { return kafka_device(ctx, nullptr); }

// msim_check that also explains.  Towards the context it is msim_check: the records, check_ms and the count of hand-overs are left as
// msim_check leaves them; where msim_check keeps to the host cores (a concurrency beyond 64, developer flag 0x800) the walk explains.
extern "C" int msim_explain_kafka(msim_ctx *ctx, msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings, uint32_t n_out) {
  if (!ctx || !hdr || (!findings && max_findings)) return MSIM_E_INVALID;
  if (int rc = explain_refusal(ctx, "msim_explain_kafka", ctx->cfg.workload == MSIM_WL_KAFKA, "a kafka", n_out)) return rc;
  if (msim_dev_flags(ctx) & 0x800u) return msim_explain_kafka_host(ctx, hdr, findings, max_findings);
  const KafkaExplainRun xr{hdr, findings, max_findings};
  return kafka_device(ctx, &xr);
}

// Checks `n_histories` kafka histories given on the host (rows / payload words of history i at row_offsets[i] / payload_offsets[i]) as
// msim_check does for the histories of a run; `concurrency` = the worker threads of the test (process mod concurrency).
static int kafka_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                       uint32_t n_histories, uint32_t concurrency, msim_check_result *out, uint32_t *n_host, bool classify, const KafkaExplainRun *xr = nullptr) {
  if (!rows || !row_offsets || !payload_offsets || !out || n_histories == 0 || concurrency == 0 || concurrency > CMAX) return MSIM_E_INVALID;
  if (payload_offsets[n_histories] != 0 && !payload) return MSIM_E_INVALID;   // (as msim_check_kafka_rows: payload words announced, none given)
  BatchFrame<OffsetsBatch> f(device); msim_ctx *ctx = &f.ctx;
  if (int rc = f.begin(n_histories, sizeof(msim_check_result), rows, row_offsets, payload, payload_offsets, n_histories, 0x7FFFFFFFull, 0x7FFFFFFFull)) return rc;
  KCParams kp;
  std::memset(&kp, 0, sizeof kp);
  f.bind(kp);
  kp.T = OFFS; kp.C = concurrency;
  return kafka_dev_run(ctx, kp, n_histories, nullptr, out, nullptr, n_host, classify, xr);
}

extern "C" int msim_check_kafka_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                                      uint32_t n_histories, uint32_t concurrency, msim_check_result *out, uint32_t *n_host) {
  return kafka_batch(device, rows, row_offsets, payload, payload_offsets, n_histories, concurrency, out, n_host, false);
}

// As msim_check_kafka_batch, but what the clean pass cannot prove clean is classified by kafka_classify_kernel: only that kernel's
// hand-overs (its header comment) reach the host checker and are counted in *n_host.
extern "C" int msim_classify_kafka_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                                         uint32_t n_histories, uint32_t concurrency, msim_check_result *out, uint32_t *n_host) {
  return kafka_batch(device, rows, row_offsets, payload, payload_offsets, n_histories, concurrency, out, n_host, true);
}

// As msim_classify_kafka_batch, with kafka_explain_kernel in place of kafka_classify_kernel: hdr[i] and history i's findings at
// findings + i * max_findings (include/maelsim.h, "kafka: the explanation of a verdict"); that kernel's hand-overs (its header comment)
// are explained by the host walk and counted in *n_host.
extern "C" int msim_explain_kafka_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                                        uint32_t n_histories, uint32_t concurrency, msim_check_result *out, msim_kafka_explain *hdr,
                                        msim_kafka_finding *findings, uint32_t max_findings, uint32_t *n_host) {
  if (!hdr || (!findings && max_findings)) return MSIM_E_INVALID;
  const KafkaExplainRun xr{hdr, findings, max_findings};
  return kafka_batch(device, rows, row_offsets, payload, payload_offsets, n_histories, concurrency, out, n_host, true, &xr);
}
