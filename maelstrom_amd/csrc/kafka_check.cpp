// kafka_check.cpp — the checker of the kafka workload (msim_check for MSIM_WL_KAFKA), on the host cores.
//
// What the reference wires in is [upstream] jepsen.tests.kafka's checker (workload/kafka.clj:288-311 takes the whole workload from
// it); it is not vendored.  What IS in the reference is the description of the anomalies it looks for, workload/kafka.clj:21-70, and
// this file restates exactly those (PARITY UNPINNED beyond the one example the reference prints, :42-60, which tests/ reproduces):
//   * the log of a key is what all observations agree on: every :ok send gives (offset, message), every :ok poll a run of them.
//     An offset seen with two different messages is `inconsistent-offsets`, a message seen at two offsets of a key `duplicate`;
//   * lost write (:23-25): an acknowledged send whose offset no poll ever returned although some poll returned a HIGHER offset of
//     that key; unobserved (:25-28): acknowledged, never polled, and nothing above it polled either — reported, not an error
//     ("there is no recency requirement");
//   * nonmonotonic (:30-37): a client's offsets of a key must strictly increase — inside one poll (`int-nonmonotonic-poll`),
//     between two polls of one process (`nonmonotonic-poll`), between two acknowledged sends of one process (`nonmonotonic-send`);
//   * skip (:39-62): a client's polls of a key jump over an offset that is known to exist — inside one poll (`int-poll-skip`) or
//     between two polls of one process (`poll-skip`, the example at :42-60);
//   * "external nonmonotonic and skip errors are not tracked across assign operations" (:64-70) — nor across a crash, which gives the
//     worker a new process and a new client, nor across a poll that did not complete :ok (its client has already moved on, see below);
//   * aborted read: a poll returns a message whose send definitely failed (the cas lost: error 30).
// out: valid = 1 iff none of the errors above (2 = :unknown when nothing was acknowledged and nothing polled), attempt_count = sends
// invoked, stable_count = sends acknowledged, lost_count = lost writes, never_read_count = unobserved, duplicated_count = duplicates,
// error_count = MSIM_KAFKA_* bits, op / ok / fail / info counts as everywhere.
// msim_explain_kafka_rows is the same walk handed an `Explain`: wherever it sets a bit it also records the witness — key, offsets, the
// rows of the two ops — that include/maelsim.h defines ("kafka: the explanation of a verdict"); the verdict does not depend on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "check_run.h"

namespace {

constexpr uint32_t KEYS = 8, OFFS = 2048, NOMSG = 0xFFFFu;

struct Tables {
  uint16_t msg[KEYS][OFFS];            // the key's log as observed (NOMSG: offset never seen)
  uint8_t polled[KEYS][OFFS], acked[KEYS][OFFS];
  uint16_t where[KEYS][OFFS];          // message value -> 1 + offset it was seen at
  uint8_t failed[KEYS][OFFS];          // message value: its send definitely failed
  uint8_t dup_at[KEYS][OFFS];          // offset already counted as a duplicate's second home
};

struct Proc { uint32_t process; bool open; int32_t last_poll[KEYS], last_send[KEYS]; uint32_t poll_row[KEYS], send_row[KEYS]; };

// What the explanation keeps beside the tables (msim_explain_kafka_rows; include/maelsim.h, "kafka: the explanation of a verdict"): the
// rows behind the cells, and the findings of the walk as it judges them.  check_kafka fills it where it is given one, and decides nothing
// by it.
constexpr uint32_t NOROW = MSIM_NO_VALUE;
struct Explain {
  struct Cell { uint32_t first_row, first_msg, alt_row, alt_msg, last_row; };   // per (key, offset): the first observation, the first one with another message, the last
  std::vector<Cell> at;                       // [KEYS * OFFS]
  std::vector<uint32_t> home_row;             // [KEYS * OFFS] by message: the row of its first observation
  std::vector<uint32_t> dup_row, dup_msg;     // [KEYS * OFFS] by offset: the first observation whose home is elsewhere
  std::vector<uint32_t> ack_row, poll_row, fail_row;   // the lowest :ok send row / :ok poll row of (key, offset), :fail send row of (key, message)
  std::vector<msim_kafka_finding> found;
  Explain() : at(KEYS * OFFS, Cell{NOROW, 0, NOROW, 0, NOROW}), home_row(KEYS * OFFS, NOROW), dup_row(KEYS * OFFS, NOROW), dup_msg(KEYS * OFFS, 0),
              ack_row(KEYS * OFFS, NOROW), poll_row(KEYS * OFFS, NOROW), fail_row(KEYS * OFFS, NOROW) {}
  void add(uint32_t anomaly, uint32_t key, uint32_t offset, uint32_t value, uint32_t other, uint32_t row_a, uint32_t row_b) {
    found.push_back(msim_kafka_finding{anomaly, key, offset, value, other, row_a, row_b, 0u});
  }
};

// the observation observe() is about to take (before it: where[k][m] still says whether m was seen)
void note(Explain &x, const Tables &t, uint32_t k, uint32_t o, uint32_t m, uint32_t row) {
  if (k >= KEYS || o >= OFFS || m >= OFFS) return;
  if (!t.where[k][m]) x.home_row[k * OFFS + m] = row;
  else if (t.where[k][m] != o + 1 && x.dup_row[k * OFFS + o] == NOROW) { x.dup_row[k * OFFS + o] = row; x.dup_msg[k * OFFS + o] = m; }
  Explain::Cell &c = x.at[k * OFFS + o];
  if (c.first_row == NOROW) { c.first_row = row; c.first_msg = m; }
  else if (c.alt_row == NOROW && m != c.first_msg) { c.alt_row = row; c.alt_msg = m; }
  c.last_row = row;
}

void observe(Tables &t, uint32_t k, uint32_t o, uint32_t m, uint32_t &bits, uint32_t &dups) {
  if (k >= KEYS || o >= OFFS || m >= OFFS) { bits |= MSIM_KAFKA_MALFORMED; return; }
  if (t.msg[k][o] != NOMSG && t.msg[k][o] != m) bits |= MSIM_KAFKA_INCONSISTENT_OFFSETS;
  t.msg[k][o] = (uint16_t)m;
  if (t.where[k][m] && t.where[k][m] != o + 1) { bits |= MSIM_KAFKA_DUPLICATE; if (!t.dup_at[k][o]) { t.dup_at[k][o] = 1; dups++; } }
  else t.where[k][m] = (uint16_t)(o + 1);
}

// is some offset strictly between a and b known to exist?
bool known_between(const Tables &t, uint32_t k, int32_t a, int32_t b) {
  for (int32_t o = a + 1; o < b; o++) if (o >= 0 && (uint32_t)o < OFFS && t.msg[k][o] != NOMSG) return true;
  return false;
}

void check_kafka(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, msim_check_result *out, Tables &t,
                 Explain *x = nullptr) {
  std::memset(out, 0, sizeof *out);
  std::memset(t.msg, 0xFF, sizeof t.msg);
  std::memset(t.polled, 0, sizeof t.polled); std::memset(t.acked, 0, sizeof t.acked);
  std::memset(t.where, 0, sizeof t.where); std::memset(t.failed, 0, sizeof t.failed); std::memset(t.dup_at, 0, sizeof t.dup_at);
  uint32_t bits = 0, dups = 0;

  // pass 1: what exists (every observation), what was acknowledged, what was polled, which sends failed
  for (uint32_t i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    const uint32_t type = MSIM_OP_TYPE(r), f = MSIM_OP_F(r);
    if (MSIM_OP_PROCESS(r) == MSIM_PROCESS_NEMESIS) continue;
    if (type == MSIM_T_INVOKE) out->op_count++;
    else if (type == MSIM_T_OK) out->ok_count++; else if (type == MSIM_T_FAIL) out->fail_count++; else out->info_count++;
    if (f == MSIM_F_SEND) {
      const uint32_t k = r.value & 63u, m = (r.value >> 6) & 0x7FFu, o = r.value >> 17;
      if (type == MSIM_T_INVOKE) out->attempt_count++;
      else if (type == MSIM_T_OK) {
        if (o == 0x7FFu || k >= KEYS) { bits |= MSIM_KAFKA_MALFORMED; continue; }
        out->stable_count++;
        if (x) note(*x, t, k, o, m, i);
        observe(t, k, o, m, bits, dups);
        if (k < KEYS && o < OFFS) { t.acked[k][o] = 1; if (x && x->ack_row[k * OFFS + o] == NOROW) x->ack_row[k * OFFS + o] = i; }
      } else if (type == MSIM_T_FAIL && k < KEYS && m < OFFS) { t.failed[k][m] = 1; if (x && x->fail_row[k * OFFS + m] == NOROW) x->fail_row[k * OFFS + m] = i; }
    } else if (f == MSIM_F_POLL && type == MSIM_T_OK) {
      const uint32_t len = MSIM_OP_LEN(r);
      if (len == 0) continue;
      if ((uint64_t)r.value + len > n_words) { bits |= MSIM_KAFKA_MALFORMED; continue; }
      const uint32_t *w = payload + r.value;
      for (uint32_t p = 0; p < len;) {
        const uint32_t h = w[p++], k = h & 7u, n = (h >> 8) & 0xFFu, o0 = h >> 16;
        if (p + (n + 1) / 2 > len) { bits |= MSIM_KAFKA_MALFORMED; break; }
        for (uint32_t e = 0; e < n; e++) {
          const uint32_t m = (w[p + e / 2] >> (16 * (e & 1))) & 0xFFFFu;
          if (x) note(*x, t, k, o0 + e, m, i);
          observe(t, k, o0 + e, m, bits, dups);
          if (o0 + e < OFFS) { t.polled[k][o0 + e] = 1; if (x && x->poll_row[k * OFFS + o0 + e] == NOROW) x->poll_row[k * OFFS + o0 + e] = i; }
        }
        p += (n + 1) / 2;
      }
    }
  }

  // lost / unobserved writes; aborted reads
  for (uint32_t k = 0; k < KEYS; k++) {
    int32_t top = -1;
    for (uint32_t o = 0; o < OFFS; o++) if (t.polled[k][o]) top = (int32_t)o;
    for (uint32_t o = 0; o < OFFS; o++) {
      if (t.acked[k][o] && !t.polled[k][o]) { if ((int32_t)o < top) { out->lost_count++; bits |= MSIM_KAFKA_LOST_WRITE; } else out->never_read_count++; }
      if (t.polled[k][o] && t.msg[k][o] != NOMSG && t.failed[k][t.msg[k][o]]) bits |= MSIM_KAFKA_ABORTED_READ;
      if (!x) continue;
      const uint32_t i = k * OFFS + o;
      if (t.acked[k][o] && !t.polled[k][o] && (int32_t)o < top)
        x->add(MSIM_KAFKA_LOST_WRITE, k, o, (rows[x->ack_row[i]].value >> 6) & 0x7FFu, (uint32_t)top, x->ack_row[i], x->poll_row[k * OFFS + (uint32_t)top]);
      const Explain::Cell &c = x->at[i];
      if (c.alt_row != NOROW) {   // two different messages: the first observation that differs from the last one is the first one, or the first other one
        const bool first = c.first_msg != t.msg[k][o];
        x->add(MSIM_KAFKA_INCONSISTENT_OFFSETS, k, o, t.msg[k][o], first ? c.first_msg : c.alt_msg, first ? c.first_row : c.alt_row, c.last_row);
      }
      if (t.dup_at[k][o]) { const uint32_t m = x->dup_msg[i]; x->add(MSIM_KAFKA_DUPLICATE, k, o, m, t.where[k][m] - 1u, x->home_row[k * OFFS + m], x->dup_row[i]); }
      if (t.polled[k][o] && t.msg[k][o] != NOMSG && t.failed[k][t.msg[k][o]])
        x->add(MSIM_KAFKA_ABORTED_READ, k, o, t.msg[k][o], 0u, x->fail_row[k * OFFS + t.msg[k][o]], x->poll_row[i]);
    }
  }

  // pass 2: every process's own sequence of offsets per key
  std::vector<Proc> procs;
  auto proc_of = [&](uint32_t process) -> Proc & {
    for (Proc &p : procs) if (p.process == process) return p;
    Proc p; p.process = process; p.open = true;
    for (uint32_t k = 0; k < KEYS; k++) { p.last_poll[k] = -1; p.last_send[k] = -1; p.poll_row[k] = NOROW; p.send_row[k] = NOROW; }
    procs.push_back(p);
    return procs.back();
  };
  for (uint32_t i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    const uint32_t type = MSIM_OP_TYPE(r), f = MSIM_OP_F(r), process = MSIM_OP_PROCESS(r);
    if (process == MSIM_PROCESS_NEMESIS) continue;
    // the positions change: nothing is tracked across an assign — nor across a poll that failed or crashed: the client has moved its
    // offsets past what that poll brought (workload/kafka.clj:181-186 runs before the commit that can fail, :223-230), the history never shows it
    if ((f == MSIM_F_ASSIGN && type == MSIM_T_INVOKE) || (f == MSIM_F_POLL && (type == MSIM_T_FAIL || type == MSIM_T_INFO))) {
      Proc &p = proc_of(process);
      for (uint32_t k = 0; k < KEYS; k++) p.last_poll[k] = -1;
      continue;
    }
    if (type != MSIM_T_OK) continue;
    if (f == MSIM_F_SEND) {
      const uint32_t k = r.value & 63u, o = r.value >> 17;
      if (k >= KEYS || o >= OFFS) continue;
      Proc &p = proc_of(process);
      if (p.last_send[k] >= 0 && (int32_t)o <= p.last_send[k]) {
        bits |= MSIM_KAFKA_NONMONOTONIC_SEND;
        if (x) x->add(MSIM_KAFKA_NONMONOTONIC_SEND, k, o, (r.value >> 6) & 0x7FFu, (uint32_t)p.last_send[k], p.send_row[k], i);
      }
      p.last_send[k] = (int32_t)o; p.send_row[k] = i;
    } else if (f == MSIM_F_POLL) {
      const uint32_t len = MSIM_OP_LEN(r);
      if (len == 0 || (uint64_t)r.value + len > n_words) continue;
      Proc &p = proc_of(process);
      const uint32_t *w = payload + r.value;
      uint32_t in_this_poll = 0;   // keys that already had a run in this poll: what follows is judged as an internal error
      for (uint32_t q = 0; q < len;) {
        const uint32_t h = w[q++], k = h & 7u, n = (h >> 8) & 0xFFu, o0 = h >> 16;
        if (q + (n + 1) / 2 > len) break;
        const uint32_t m0 = n ? w[q] & 0xFFFFu : 0u;   // the block's first message
        q += (n + 1) / 2;
        if (!n) continue;
        // a block holds one run o0, o0 + 1, ...: a key's pairs that do not continue the run start another block of the same key
        const int32_t first = (int32_t)o0, last = (int32_t)(o0 + n - 1);
        const bool internal = (in_this_poll >> k) & 1u;
        if (p.last_poll[k] >= 0) {
          if (first <= p.last_poll[k]) {
            bits |= internal ? MSIM_KAFKA_INT_NONMONOTONIC_POLL : MSIM_KAFKA_NONMONOTONIC_POLL;
            if (x) x->add(internal ? MSIM_KAFKA_INT_NONMONOTONIC_POLL : MSIM_KAFKA_NONMONOTONIC_POLL, k, o0, m0, (uint32_t)p.last_poll[k], p.poll_row[k], i);
          } else if (first > p.last_poll[k] + 1 && known_between(t, k, p.last_poll[k], first)) {
            bits |= internal ? MSIM_KAFKA_INT_POLL_SKIP : MSIM_KAFKA_POLL_SKIP;
            if (x) {
              uint32_t skipped = 0;
              for (int32_t o = p.last_poll[k] + 1; o < first; o++) skipped += (uint32_t)o < OFFS && t.msg[k][o] != NOMSG;
              x->add(internal ? MSIM_KAFKA_INT_POLL_SKIP : MSIM_KAFKA_POLL_SKIP, k, o0, skipped, (uint32_t)p.last_poll[k], p.poll_row[k], i);
            }
          }
        }
        p.last_poll[k] = last; p.poll_row[k] = i; in_this_poll |= 1u << k;
      }
    }
  }

  out->duplicated_count = dups;
  out->error_count = bits;
  const uint32_t errors = bits & ~0u;
  if (flags || errors) out->valid = 0;
  else out->valid = (out->stable_count == 0 && out->ok_count == 0) ? 2u : 1u;
}

}  // namespace

// one history on the calling thread (kafka_check_dev.hip: what the device pass could not prove clean)
void msim_kafka_check_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, msim_check_result *out) {
  std::vector<Tables> t(1);
  check_kafka(rows, n_rows, payload, n_words, flags, out, t[0]);
}

// The findings of one history in the contract's order, cut to max_findings (include/maelsim.h, "kafka: the explanation of a verdict").
static void explain_kafka(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, msim_check_result *out,
                          msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings) {
  std::vector<Tables> t(1);
  Explain x;
  check_kafka(rows, n_rows, payload, n_words, flags, out, t[0], &x);
  std::memset(hdr, 0, sizeof *hdr);
  if (max_findings) std::memset(findings, 0, (size_t)max_findings * sizeof *findings);
  for (const msim_kafka_finding &f : x.found) hdr->count[__builtin_ctz(f.anomaly)]++;
  hdr->count[9] = (out->error_count & MSIM_KAFKA_MALFORMED) ? 1u : 0u;
  std::sort(x.found.begin(), x.found.end(), [](const msim_kafka_finding &a, const msim_kafka_finding &b) {
    const uint32_t u[7] = {a.anomaly, a.key, a.offset, a.value, a.other, a.row_a, a.row_b}, v[7] = {b.anomaly, b.key, b.offset, b.value, b.other, b.row_a, b.row_b};
    return std::lexicographical_compare(u, u + 7, v, v + 7);
  });
  hdr->n_findings = (uint32_t)std::min<size_t>(x.found.size(), max_findings);
  hdr->truncated = x.found.size() > max_findings ? 1u : 0u;
  std::copy(x.found.begin(), x.found.begin() + hdr->n_findings, findings);
}

// one history on the calling thread, explained (kafka_check_dev.hip: what kafka_explain_kernel hands over)
void msim_kafka_explain_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, msim_check_result *out,
                                      msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings) {
  explain_kafka(rows, n_rows, payload, n_words, flags, out, hdr, findings, max_findings);
}

extern "C" int msim_explain_kafka_rows(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, msim_check_result *out,
                                       msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings) {
  if ((!rows && n_rows) || !out || (!payload && n_words) || !hdr || (!findings && max_findings)) return MSIM_E_INVALID;
  explain_kafka(rows, n_rows, payload, n_words, 0, out, hdr, findings, max_findings);
  return MSIM_OK;
}

extern "C" int msim_check_kafka_rows(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, msim_check_result *out) {
  if ((!rows && n_rows) || !out || (!payload && n_words)) return MSIM_E_INVALID;
  std::vector<Tables> t(1);
  check_kafka(rows, n_rows, payload, n_words, 0, out, t[0]);
  return MSIM_OK;
}

// (hdr: msim_explain_kafka's arrays — every history explained by the walk; null: msim_check)
int msim_explain_kafka_host(msim_ctx *ctx, msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings) {
  return host_check_run(ctx, []() { return std::vector<Tables>(1); }, [=](std::vector<Tables> &t, uint32_t i, const msim_op *rows, uint32_t n_rows, const uint32_t *pay, uint32_t n_words,
                                                                          uint32_t flags, msim_check_result *res) {
    if (hdr) explain_kafka(rows, n_rows, pay, n_words, flags, res, &hdr[i], findings + (size_t)i * max_findings, max_findings);
    else check_kafka(rows, n_rows, pay, n_words, flags, res, t[0]);
  });
}

int msim_check_kafka_host(msim_ctx *ctx) { return msim_explain_kafka_host(ctx, nullptr, nullptr, 0); }
