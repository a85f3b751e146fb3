// pn_check.cpp — the small host-side checkers: pn-counter / g-counter (workload/pn_counter.clj:84-123) and unique-ids
// ([upstream] jepsen.checker/unique-ids, unique_ids.clj:67).
//
// "Every final read is the sum of all known-completed adds plus any number of possibly-completed adds": the acceptable
// set starts as {sum of :ok adds}; every :info add (a timed-out add may or may not have happened) unions in the set
// shifted by its delta.  The reference keeps the set in a Guava TreeRangeSet of open ranges (lower-1, upper+1) so that
// adjacent integers merge; the same set is kept here as sorted closed integer ranges, merged when they touch.  Reads
// marked :final? that completed :ok must lie in it.  Pinned by the reference's own vectors (test/maelstrom/workload/
// pn_counter_test.clj:10-36) in tests/test_pn_counter.py.
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "check_run.h"

namespace {

typedef std::vector<std::pair<int64_t, int64_t>> Ranges;

void merge_in(Ranges &r) {
  std::sort(r.begin(), r.end());
  size_t w = 0;
  for (size_t i = 0; i < r.size(); i++) {
    if (w && r[i].first <= r[w - 1].second + 1) r[w - 1].second = std::max(r[w - 1].second, r[i].second);
    else r[w++] = r[i];
  }
  r.resize(w);
}

// the explanation a walk is handed beside its record (include/maelsim_small_explain.h); null: the plain check
template <class Hdr> struct Sink { Hdr *hdr; void *records; uint32_t max; };
template <class Hdr> void clear_sink(const Sink<Hdr> *x) {
  std::memset(x->hdr, 0, sizeof(Hdr));
  if (x->max) std::memset(x->records, 0, (size_t)x->max * 16);
}

void check_history(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *out, Ranges &acc, const Sink<msim_pn_explain> *x = nullptr) {
  std::memset(out, 0, sizeof *out);
  if (x) clear_sink(x);
  int64_t definite = 0;
  for (uint32_t i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    if (MSIM_OP_PROCESS(r) == MSIM_PROCESS_NEMESIS) continue;
    const uint32_t t = MSIM_OP_TYPE(r);
    if (t == MSIM_T_INVOKE) out->op_count++; else if (t == MSIM_T_OK) out->ok_count++; else if (t == MSIM_T_FAIL) out->fail_count++; else out->info_count++;
    if (MSIM_OP_F(r) == MSIM_F_ADD && t == MSIM_T_OK) definite += (int32_t)r.value;
  }
  acc.clear();
  acc.emplace_back(definite, definite);
  for (uint32_t i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    if (MSIM_OP_PROCESS(r) == MSIM_PROCESS_NEMESIS || MSIM_OP_F(r) != MSIM_F_ADD || MSIM_OP_TYPE(r) != MSIM_T_INFO) continue;
    const int64_t d = (int32_t)r.value;
    const size_t n = acc.size();
    for (size_t k = 0; k < n; k++) acc.emplace_back(acc[k].first + d, acc[k].second + d);
    merge_in(acc);
  }
  for (uint32_t i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    if (MSIM_OP_PROCESS(r) == MSIM_PROCESS_NEMESIS || !MSIM_OP_FINAL(r) || MSIM_OP_TYPE(r) != MSIM_T_OK) continue;
    out->attempt_count++;
    const int64_t v = (int32_t)r.value;
    bool ok = false;
    for (const auto &g : acc) if (g.first <= v && v <= g.second) { ok = true; break; }
    if (!ok) out->error_count++;
    if (x && x->hdr->n_reads < x->max) static_cast<msim_pn_read *>(x->records)[x->hdr->n_reads++] = msim_pn_read{i, (int32_t)r.value, MSIM_OP_PROCESS(r), ok ? 1u : 0u};
  }
  if (x) {   // the ranges take the room the reads left
    const uint32_t room = x->max - x->hdr->n_reads;
    msim_pn_range *const g = static_cast<msim_pn_range *>(x->records) + x->hdr->n_reads;
    for (size_t k = 0; k < acc.size() && k < room; k++) g[x->hdr->n_ranges++] = msim_pn_range{acc[k].first, acc[k].second};
    x->hdr->truncated = x->hdr->n_reads < out->attempt_count || x->hdr->n_ranges < acc.size() ? 1u : 0u;
    x->hdr->definite_sum = definite;
  }
  out->stable_count = (uint32_t)acc.size();
  out->valid = flags ? 0u : (out->error_count == 0 ? 1u : 0u);
}

// [upstream] jepsen.checker/unique-ids: :attempted-count = :invoke :generate ops, :acknowledged-count = :ok ones,
// :duplicated = values acknowledged more than once, :range = [min max]; valid iff nothing is duplicated.
void check_unique(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *out, std::vector<uint32_t> &ids, const Sink<msim_unique_explain> *x = nullptr) {
  std::memset(out, 0, sizeof *out);
  if (x) clear_sink(x);
  ids.clear();
  for (uint32_t i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    if (MSIM_OP_PROCESS(r) == MSIM_PROCESS_NEMESIS) continue;
    const uint32_t t = MSIM_OP_TYPE(r);
    if (t == MSIM_T_INVOKE) out->op_count++; else if (t == MSIM_T_OK) out->ok_count++; else if (t == MSIM_T_FAIL) out->fail_count++; else out->info_count++;
    if (MSIM_OP_F(r) != MSIM_F_GENERATE) continue;
    if (t == MSIM_T_INVOKE) out->attempt_count++;
    if (t == MSIM_T_OK) ids.push_back(r.value);
  }
  std::sort(ids.begin(), ids.end());
  uint32_t dups = 0;
  for (size_t i = 1; i < ids.size(); i++) if (ids[i] == ids[i - 1] && (i < 2 || ids[i] != ids[i - 2])) dups++;
  out->duplicated_count = dups;
  if (!ids.empty()) { out->stable_latency_ms[0] = ids.front(); out->stable_latency_ms[1] = ids.back(); }
  out->valid = flags ? 0u : (dups == 0 ? 1u : 0u);
  if (x && dups) {   // the duplicated ids with the rows of their first two acknowledgements, by (count descending, id descending)
    std::vector<std::pair<uint32_t, uint32_t>> acks;   // (id, row): sorted, an id's rows ascend
    for (uint32_t i = 0; i < n_rows; i++) {
      const msim_op &r = rows[i];
      if (MSIM_OP_PROCESS(r) != MSIM_PROCESS_NEMESIS && MSIM_OP_F(r) == MSIM_F_GENERATE && MSIM_OP_TYPE(r) == MSIM_T_OK) acks.emplace_back(r.value, i);
    }
    std::sort(acks.begin(), acks.end());
    std::vector<msim_unique_dup> d;
    for (size_t i = 0, j; i < acks.size(); i = j) {
      for (j = i + 1; j < acks.size() && acks[j].first == acks[i].first;) j++;
      if (j - i >= 2) d.push_back(msim_unique_dup{acks[i].first, (uint32_t)(j - i), acks[i].second, acks[i + 1].second});
    }
    std::sort(d.begin(), d.end(), [](const msim_unique_dup &a, const msim_unique_dup &b) { return a.count != b.count ? a.count > b.count : a.id > b.id; });
    x->hdr->n_dups = (uint32_t)std::min<size_t>(d.size(), x->max);
    x->hdr->truncated = d.size() > x->max ? 1u : 0u;
    if (x->hdr->n_dups) std::memcpy(x->records, d.data(), (size_t)x->hdr->n_dups * sizeof(msim_unique_dup));
  }
}

// echo (workload/echo.clj:44-63) as checker.hip's check_kernel judges it: the record msim_check writes for an echo history, and the
// invocations it counts as errors (include/maelsim_small_explain.h: paired by worker thread = process mod concurrency)
void check_echo(const msim_op *rows, uint32_t n_rows, uint32_t concurrency, uint32_t flags, msim_check_result *out, const Sink<msim_echo_explain> *x) {
  std::memset(out, 0, sizeof *out);
  if (x) clear_sink(x);
  std::vector<uint32_t> open(concurrency, MSIM_NO_VALUE);   // the thread's open invocation
  std::vector<msim_echo_error> errs;
  for (uint32_t i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    if (MSIM_OP_PROCESS(r) == MSIM_PROCESS_NEMESIS) continue;
    const uint32_t t = MSIM_OP_TYPE(r), th = MSIM_OP_PROCESS(r) % concurrency;
    if (t == MSIM_T_INVOKE) out->op_count++; else if (t == MSIM_T_OK) out->ok_count++; else if (t == MSIM_T_FAIL) out->fail_count++; else out->info_count++;
    if (MSIM_OP_F(r) != MSIM_F_ECHO) continue;
    if (t == MSIM_T_INVOKE) { open[th] = i; continue; }
    const uint32_t inv = open[th];
    open[th] = MSIM_NO_VALUE;
    if (inv == MSIM_NO_VALUE) continue;
    if (t != MSIM_T_OK) errs.push_back(msim_echo_error{inv, MSIM_NO_VALUE, rows[inv].value, MSIM_NO_VALUE});
    else if (r.value != rows[inv].value) errs.push_back(msim_echo_error{inv, i, rows[inv].value, r.value});
  }
  for (uint32_t inv : open) if (inv != MSIM_NO_VALUE) errs.push_back(msim_echo_error{inv, MSIM_NO_VALUE, rows[inv].value, MSIM_NO_VALUE});
  std::sort(errs.begin(), errs.end(), [](const msim_echo_error &a, const msim_echo_error &b) { return a.invoke_row < b.invoke_row; });
  out->error_count = (uint32_t)errs.size();
  out->valid = flags ? 0u : (errs.empty() ? 1u : 0u);
  if (x) {
    x->hdr->n_errors = (uint32_t)std::min<size_t>(errs.size(), x->max);
    x->hdr->truncated = errs.size() > x->max ? 1u : 0u;
    if (x->hdr->n_errors) std::memcpy(x->records, errs.data(), (size_t)x->hdr->n_errors * sizeof(msim_echo_error));
  }
}

}  // namespace

// the explaining host walks on one history: what the device kernels hand over (pn_check_dev.hip, unique_check_dev.hip)
void msim_pn_explain_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res, msim_pn_explain *hdr, void *records, uint32_t max_records) {
  Ranges acc; const Sink<msim_pn_explain> x{hdr, records, max_records};
  check_history(rows, n_rows, flags, res, acc, &x);
}
void msim_unique_explain_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res, msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups) {
  std::vector<uint32_t> ids; const Sink<msim_unique_explain> x{hdr, dups, max_dups};
  check_unique(rows, n_rows, flags, res, ids, &x);
}

extern "C" int msim_explain_pn_rows(const msim_op *rows, uint32_t n_rows, msim_check_result *out, msim_pn_explain *hdr, void *records, uint32_t max_records) {
  if ((!rows && n_rows) || !out || !hdr || (!records && max_records)) return MSIM_E_INVALID;
  msim_pn_explain_instance_host(rows, n_rows, 0, out, hdr, records, max_records);
  return MSIM_OK;
}
extern "C" int msim_explain_unique_rows(const msim_op *rows, uint32_t n_rows, msim_check_result *out, msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups) {
  if ((!rows && n_rows) || !out || !hdr || (!dups && max_dups)) return MSIM_E_INVALID;
  msim_unique_explain_instance_host(rows, n_rows, 0, out, hdr, dups, max_dups);
  return MSIM_OK;
}
extern "C" int msim_explain_echo_rows(const msim_op *rows, uint32_t n_rows, uint32_t concurrency, msim_check_result *out, msim_echo_explain *hdr, msim_echo_error *errors, uint32_t max_errors) {
  if ((!rows && n_rows) || !out || !hdr || (!errors && max_errors) || concurrency == 0) return MSIM_E_INVALID;
  const Sink<msim_echo_explain> x{hdr, errors, max_errors};
  check_echo(rows, n_rows, concurrency, 0, out, &x);
  return MSIM_OK;
}

// the host checker for one pn-counter / g-counter history (pn_check_dev.hip hands over what its bitmap does not cover)
void msim_pn_check_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res) { Ranges acc; check_history(rows, n_rows, flags, res, acc); }

extern "C" int msim_check_unique_rows(const msim_op *rows, uint32_t n_rows, msim_check_result *out) {
  if ((!rows && n_rows) || !out) return MSIM_E_INVALID;
  std::vector<uint32_t> ids;
  check_unique(rows, n_rows, 0, out, ids);
  return MSIM_OK;
}

int msim_check_unique_host(msim_ctx *ctx) {
  return host_check_run(ctx, []() { return std::vector<uint32_t>(); }, [](std::vector<uint32_t> &ids, uint32_t, const msim_op *rows, uint32_t n_rows, const uint32_t *, uint32_t, uint32_t flags,
                                                                          msim_check_result *res) { check_unique(rows, n_rows, flags, res, ids); });
}

extern "C" int msim_check_pn_rows(const msim_op *rows, uint32_t n_rows, msim_check_result *out, int64_t *ranges, uint32_t cap, uint32_t *n_ranges) {
  if ((!rows && n_rows) || !out) return MSIM_E_INVALID;
  Ranges acc;
  check_history(rows, n_rows, 0, out, acc);
  if (n_ranges) *n_ranges = (uint32_t)acc.size();
  if (ranges) for (uint32_t i = 0; i < cap && i < acc.size(); i++) { ranges[2 * i] = acc[i].first; ranges[2 * i + 1] = acc[i].second; }
  return MSIM_OK;
}

int msim_check_pn_host(msim_ctx *ctx) {
  return host_check_run(ctx, []() { return Ranges(); }, [](Ranges &acc, uint32_t, const msim_op *rows, uint32_t n_rows, const uint32_t *, uint32_t, uint32_t flags, msim_check_result *res) {
    check_history(rows, n_rows, flags, res, acc);
  });
}

// msim_explain_pn / msim_explain_unique where msim_check keeps to the host cores (developer flag 0x800): the walks explain
int msim_explain_pn_host(msim_ctx *ctx, msim_pn_explain *hdr, void *records, uint32_t max_records) {
  return host_check_run(ctx, []() { return 0; }, [=](int &, uint32_t i, const msim_op *rows, uint32_t n_rows, const uint32_t *, uint32_t, uint32_t flags, msim_check_result *res) {
    msim_pn_explain_instance_host(rows, n_rows, flags, res, hdr + i, static_cast<char *>(records) + (size_t)i * max_records * 16, max_records);
  });
}
int msim_explain_unique_host(msim_ctx *ctx, msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups) {
  return host_check_run(ctx, []() { return 0; }, [=](int &, uint32_t i, const msim_op *rows, uint32_t n_rows, const uint32_t *, uint32_t, uint32_t flags, msim_check_result *res) {
    msim_unique_explain_instance_host(rows, n_rows, flags, res, hdr + i, dups + (size_t)i * max_dups, max_dups);
  });
}
