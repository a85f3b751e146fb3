// set_check.cpp — [upstream] jepsen.checker/set-full on the host, one history, with its explanation (include/maelsim.h msim_set_explain):
// the plain walk over the ops that the definitions there describe, op by op and element by element.  The device kernels
// (csrc/set_full_body.inc) are held against it byte for byte; callers without a device get the lists from it.  The record itself follows
// the rules at the head of checker.hip (counts, quantiles, op_count, :stats).
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "engine_internal.h"

namespace {

constexpr u32 NIL = MSIM_NO_VALUE;

struct Element { u32 known = NIL, last_present = NIL, last_absent = NIL; };

// points {0 .5 .95 .99 1} -> sorted[min(n-1, floor(n*q))]; all 0 for an empty list
void quantiles(std::vector<u32> v, u32 *q) {
  const double pts[5] = {0.0, 0.5, 0.95, 0.99, 1.0};
  std::sort(v.begin(), v.end());
  for (int i = 0; i < 5; i++) q[i] = v.empty() ? 0u : v[std::min<size_t>(v.size() - 1, (size_t)((double)v.size() * pts[i]))];
}

// long(nanos->ms(max(0, (time(row) + 1 | 0 without one) - time(known))))
u32 latency_ms(const msim_op *rows, u32 row, u32 known) {
  const uint64_t t = row == NIL ? 0 : MSIM_OP_TIME_NS(rows[row]) + 1, tk = MSIM_OP_TIME_NS(rows[known]);
  return t > tk ? (u32)((t - tk) / 1000000ull) : 0u;
}

}  // namespace

extern "C" int msim_explain_set_full_rows(uint32_t workload, const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words,
                                          msim_check_result *out, msim_set_explain *hdr, msim_set_element *elements, uint32_t max_elements) {
  if ((!rows && n_rows) || (!payload && n_words) || !out || !hdr || (!elements && max_elements)) return MSIM_E_INVALID;
  if (workload != MSIM_WL_BROADCAST && workload != MSIM_WL_G_SET) return MSIM_E_UNSUPPORTED;
  std::vector<Element> els;
  std::unordered_map<u32, u32> reads;   // process -> the row of its pending read invocation
  u32 op_count = 0, n_ok = 0, n_fail = 0, n_info = 0;
  for (u32 i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    const u32 type = MSIM_OP_TYPE(r), f = MSIM_OP_F(r), process = MSIM_OP_PROCESS(r);
    if (process == MSIM_PROCESS_NEMESIS) continue;   // (r/filter (comp number? :process))
    if (type == MSIM_T_INVOKE) op_count++; else if (type == MSIM_T_OK) n_ok++; else if (type == MSIM_T_FAIL) n_fail++; else n_info++;
    if (f == MSIM_F_ADD || f == MSIM_F_BROADCAST) {
      if (type == MSIM_T_INVOKE) els.emplace_back();   // elements are numbered in invocation order
      else if (type == MSIM_T_OK && r.value < els.size() && els[r.value].known == NIL) els[r.value].known = i;
    } else if (f == MSIM_F_READ) {
      if (type == MSIM_T_INVOKE) { reads[process] = i; continue; }
      const auto it = reads.find(process);
      if (it == reads.end()) continue;
      const u32 inv = it->second;
      reads.erase(it);
      if (type != MSIM_T_OK) continue;
      const u32 nw = MSIM_OP_LEN(r) & 0xFFu;
      if (nw && ((uint64_t)r.value + nw > n_words)) return MSIM_E_RANGE;   // a bitmap outside the payload
      for (u32 e = 0; e < els.size(); e++) {   // every element that exists when the read completes
        Element &el = els[e];
        const bool has = e / 32 < nw && ((payload[r.value + e / 32] >> (e % 32)) & 1u);
        if (has) {
          if (el.known == NIL) el.known = i;
          if (el.last_present == NIL || el.last_present < inv) el.last_present = inv;
        } else if (el.last_absent == NIL || el.last_absent < inv) el.last_absent = inv;
      }
    }
  }
  std::vector<msim_set_element> lost, never, stale;
  std::vector<u32> stable_lat, lost_lat;
  for (u32 e = 0; e < els.size(); e++) {
    const Element &el = els[e];
    const u32 kn = el.known, lp = el.last_present, la = el.last_absent;
    const bool is_stable = lp != NIL && (la == NIL || la < lp);
    const bool is_lost = kn != NIL && la != NIL && (lp == NIL || lp < la) && kn < la;
    msim_set_element rec = {e, MSIM_SET_NEVER_READ, NIL, kn, lp, la};
    if (is_stable) {
      rec.outcome = MSIM_SET_STABLE; rec.latency_ms = latency_ms(rows, la, kn);
      stable_lat.push_back(rec.latency_ms);
      if (rec.latency_ms > 0) stale.push_back(rec);
    } else if (is_lost) {
      rec.outcome = MSIM_SET_LOST; rec.latency_ms = latency_ms(rows, lp, kn);
      lost_lat.push_back(rec.latency_ms);
      lost.push_back(rec);
    } else never.push_back(rec);
  }
  std::memset(out, 0, sizeof *out);
  out->attempt_count = (u32)els.size(); out->stable_count = (u32)stable_lat.size(); out->lost_count = (u32)lost.size();
  out->never_read_count = (u32)never.size(); out->stale_count = (u32)stale.size();
  quantiles(stable_lat, out->stable_latency_ms);
  out->op_count = op_count; out->ok_count = n_ok; out->fail_count = n_fail; out->info_count = n_info;
  out->valid = !lost.empty() ? 0u : (stable_lat.empty() ? 2u : 1u);

  std::memset(hdr, 0, sizeof *hdr);
  if (max_elements) std::memset(elements, 0, (size_t)max_elements * sizeof *elements);
  // the three segments, each with the room the ones before it leave
  const u32 w_lost = std::min<u32>((u32)lost.size(), max_elements), w_never = std::min<u32>((u32)never.size(), max_elements - w_lost),
            w_stale = std::min<u32>((u32)stale.size(), max_elements - w_lost - w_never);
  std::copy_n(lost.begin(), w_lost, elements);
  std::copy_n(never.begin(), w_never, elements + w_lost);
  std::copy_n(stale.begin(), w_stale, elements + w_lost + w_never);
  hdr->n_lost = w_lost; hdr->n_never_read = w_never; hdr->n_stale = w_stale;
  hdr->truncated = (size_t)w_lost + w_never + w_stale < lost.size() + never.size() + stale.size() ? 1u : 0u;
  quantiles(lost_lat, hdr->lost_latency_ms);
  // (->> stale (sort-by :stable-latency) reverse (take 8)) over ascending elements: a stable sort, reversed
  std::stable_sort(stale.begin(), stale.end(), [](const msim_set_element &a, const msim_set_element &b) { return a.latency_ms < b.latency_ms; });
  std::reverse(stale.begin(), stale.end());
  hdr->n_worst_stale = (u32)std::min<size_t>(8, stale.size());
  std::copy_n(stale.begin(), hdr->n_worst_stale, hdr->worst_stale);
  return MSIM_OK;
}
