// check_batch_asan.cpp — every batch entry of the device checkers once, as a stand-alone program over the wavefront emulator's build of
// the checker units (tools/check_batch_asan.py compiles those units and this file with -fsanitize=address,undefined and runs it): what
// the host side of the checkers (csrc/check_run.h) allocates, it frees — LeakSanitizer at exit — and nothing reads or writes beside an
// allocation.  The batch of each entry is the five histories of tests/test_check_batch_edges_gpu.py: [no rows, one the device hands to
// the host, no rows, rows without payload words, no rows]; the explaining kafka and set-full entries have a history whose records the
// explaining kernel writes among the five.  Developer tool; prints one line per entry, exits 0 when every entry returned
// MSIM_OK.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../include/maelsim.h"

namespace {

struct History { std::vector<msim_op> rows; std::vector<uint32_t> pay; };

msim_op row(size_t i, uint32_t type, uint32_t f, uint32_t process, uint32_t value, uint32_t len = 0, bool final_read = false) {
  msim_op r;
  r.time_len = (uint64_t)i * 1000 | ((uint64_t)len << 48);
  r.packed = type | (f << 2) | ((final_read ? 1u : 0u) << 11) | (process << 12);
  r.value = value;
  return r;
}

// a transactional history of completed transactions, one after the other: {process, payload words}
History txns(std::initializer_list<std::pair<uint32_t, std::vector<uint32_t>>> ts) {
  History h;
  for (const auto &t : ts)
    for (uint32_t type : {(uint32_t)MSIM_T_INVOKE, (uint32_t)MSIM_T_OK}) {
      h.rows.push_back(row(h.rows.size(), type, MSIM_F_TXN, t.first, (uint32_t)h.pay.size(), (uint32_t)t.second.size()));
      h.pay.insert(h.pay.end(), t.second.begin(), t.second.end());
    }
  return h;
}
uint32_t append(uint32_t k, uint32_t v) { return 1u | (k << 1) | (v << 16); }   // (rw-register: a write)
uint32_t read_nil(uint32_t k) { return (k << 1) | (0xFFu << 16); }

struct Offsets {   // the offsets layout of a batch
  std::vector<msim_op> rows; std::vector<uint32_t> pay; std::vector<uint64_t> ro{0}, po{0};
  explicit Offsets(const std::vector<History> &hs) {
    for (const History &h : hs) {
      rows.insert(rows.end(), h.rows.begin(), h.rows.end()); pay.insert(pay.end(), h.pay.begin(), h.pay.end());
      ro.push_back(rows.size()); po.push_back(pay.size());
    }
    if (rows.empty()) rows.resize(1);
    if (pay.empty()) pay.resize(1);
  }
};

struct Slabs {   // the slab layout of a batch (the payload words alike, for the set-full entries)
  std::vector<msim_op> rows; std::vector<uint32_t> n_rows, pay; uint32_t max_rows = 1, max_pay = 1;
  explicit Slabs(const std::vector<History> &hs) {
    for (const History &h : hs) { if (h.rows.size() > max_rows) max_rows = (uint32_t)h.rows.size(); if (h.pay.size() > max_pay) max_pay = (uint32_t)h.pay.size(); }
    rows.resize(hs.size() * max_rows); pay.resize(hs.size() * max_pay);
    for (size_t i = 0; i < hs.size(); i++) {
      n_rows.push_back((uint32_t)hs[i].rows.size());
      std::copy(hs[i].rows.begin(), hs[i].rows.end(), rows.begin() + i * max_rows); std::copy(hs[i].pay.begin(), hs[i].pay.end(), pay.begin() + i * max_pay);
    }
  }
};

int failures = 0;
void report(const char *entry, int rc, const std::vector<msim_check_result> &out, const uint32_t *n_host = nullptr) {   // (n_host read after the call)
  std::printf("%-28s rc %d, n_host %u, valid", entry, rc, n_host ? *n_host : 0u);
  for (const auto &o : out) std::printf(" %u", o.valid);
  std::printf("\n");
  failures += rc != MSIM_OK;
}

}  // namespace

int main() {
  const History none;
  const uint32_t N = 5, STEPS = 8;
  std::vector<msim_check_result> out(N);
  std::vector<msim_cycle_result> cycles(N);
  std::vector<msim_cycle_step> steps(N * STEPS);
  uint32_t n_host = 0;
  {   // txn-list-append: element 1 appended to key 1 twice is the host's; transactions without micro-ops
    const Offsets b({none, txns({{0, {append(1, 1)}}, {1, {append(1, 1)}}, {2, {read_nil(1)}}}), none, txns({{0, {}}, {1, {}}}), none});
    report("msim_check_txn_batch", msim_check_txn_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, out.data()), out);
    report("msim_classify_txn_batch", msim_classify_txn_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, MSIM_CM_STRICT_SERIALIZABLE, out.data(), &n_host), out, &n_host);
    report("msim_explain_txn_batch", msim_explain_txn_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, MSIM_CM_STRICT_SERIALIZABLE, out.data(), &n_host,
                                                             cycles.data(), steps.data(), STEPS), out, &n_host);
  }
  {   // txn-rw-register: value 1 written to key 1 twice is the host's
    const Offsets b({none, txns({{0, {append(1, 1)}}, {1, {append(1, 1)}}}), none, txns({{0, {}}, {1, {}}}), none});
    report("msim_check_rw_batch", msim_check_rw_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, MSIM_CM_SERIALIZABLE, out.data(), &n_host), out, &n_host);
    report("msim_classify_rw_batch", msim_classify_rw_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, MSIM_CM_SERIALIZABLE, out.data(), &n_host), out, &n_host);
    report("msim_explain_rw_batch", msim_explain_rw_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, MSIM_CM_SERIALIZABLE, out.data(), &n_host,
                                                           cycles.data(), steps.data(), STEPS), out, &n_host);
  }
  {   // kafka: a send acknowledged at offset 1152 and a poll that sees another message there (the host's either way); sends alone
    History far, sends;
    far.rows = {row(0, MSIM_T_INVOKE, MSIM_F_SEND, 0, 1u | (5u << 6) | (0x7FFu << 17)), row(1, MSIM_T_OK, MSIM_F_SEND, 0, 1u | (5u << 6) | (1152u << 17)),
                row(2, MSIM_T_INVOKE, MSIM_F_POLL, 1, 0xFFFFFFFFu), row(3, MSIM_T_OK, MSIM_F_POLL, 1, 0, 2)};
    far.pay = {1u | (1u << 8) | (1152u << 16), 7u};
    sends.rows = {row(0, MSIM_T_INVOKE, MSIM_F_SEND, 0, 1u | (5u << 6) | (0x7FFu << 17)), row(1, MSIM_T_OK, MSIM_F_SEND, 0, 1u | (5u << 6))};
    const Offsets b({none, far, none, sends, none});
    report("msim_check_kafka_batch", msim_check_kafka_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, 3, out.data(), &n_host), out, &n_host);
    report("msim_classify_kafka_batch", msim_classify_kafka_batch(0, b.rows.data(), b.ro.data(), b.pay.data(), b.po.data(), N, 3, out.data(), &n_host), out, &n_host);
    // the explanation: offset 3 acknowledged twice, with two messages, is the explaining kernel's (it writes findings); `far` stays the host walk's
    History twice;
    for (uint32_t m : {5u, 6u}) { twice.rows.push_back(row(twice.rows.size(), MSIM_T_INVOKE, MSIM_F_SEND, 0, 1u | (m << 6) | (0x7FFu << 17))); twice.rows.push_back(row(twice.rows.size(), MSIM_T_OK, MSIM_F_SEND, 0, 1u | (m << 6) | (3u << 17))); }
    const Offsets x({none, far, none, twice, none});
    std::vector<msim_kafka_explain> hdr(N);
    std::vector<msim_kafka_finding> findings(N * STEPS);
    report("msim_explain_kafka_batch", msim_explain_kafka_batch(0, x.rows.data(), x.ro.data(), x.pay.data(), x.po.data(), N, 3, out.data(), hdr.data(), findings.data(), STEPS, &n_host), out, &n_host);
    std::printf("%-28s findings %u %u (truncated %u %u)\n", "", hdr[1].n_findings, hdr[3].n_findings, hdr[1].truncated, hdr[3].truncated);
    failures += hdr[3].n_findings == 0;
  }
  {   // set-full (g-set): element 1 is read once and then missing from a later read (lost), element 2 is never read; adds alone
    History lost, adds;
    auto op = [&](History &h, uint32_t type, uint32_t f, uint32_t p, uint32_t v, uint32_t len = 0) { h.rows.push_back(row(h.rows.size(), type, f, p, v, len)); };
    for (uint32_t e = 0; e < 3; e++) { op(lost, MSIM_T_INVOKE, MSIM_F_ADD, e, e); op(lost, MSIM_T_OK, MSIM_F_ADD, e, e); }
    for (uint32_t bits : {3u, 1u}) { op(lost, MSIM_T_INVOKE, MSIM_F_READ, 0, 0xFFFFFFFFu); op(lost, MSIM_T_OK, MSIM_F_READ, 0, (uint32_t)lost.pay.size(), 1); lost.pay.push_back(bits); }
    for (uint32_t e = 0; e < 2; e++) { op(adds, MSIM_T_INVOKE, MSIM_F_ADD, e, e); op(adds, MSIM_T_OK, MSIM_F_ADD, e, e); }
    const Slabs b({none, lost, none, adds, none});
    std::vector<msim_set_explain> hdr(N);
    std::vector<msim_set_element> elements(N * STEPS);
    report("msim_check_set_full_batch", msim_check_set_full_batch(0, MSIM_WL_G_SET, 3, b.rows.data(), b.n_rows.data(), b.max_rows, b.pay.data(), b.max_pay, 32, N, out.data()), out);
    report("msim_explain_set_full_batch", msim_explain_set_full_batch(0, MSIM_WL_G_SET, 3, b.rows.data(), b.n_rows.data(), b.max_rows, b.pay.data(), b.max_pay, 32, N, out.data(),
                                                                       hdr.data(), elements.data(), STEPS), out);
    std::printf("%-28s lost %u, never read %u, stale %u\n", "", hdr[1].n_lost, hdr[1].n_never_read, hdr[1].n_stale);
    failures += hdr[1].n_lost + hdr[1].n_never_read + hdr[1].n_stale == 0;
  }
  {   // lin-kv: key 0 holds 1, nine writes overlap, a read of a value nobody wrote; a stale read
    History wide, stale;
    auto kv = [](uint32_t k, uint32_t v) { return k | (v << 8) | (0xFFu << 16); };
    auto op = [&](History &h, uint32_t type, uint32_t f, uint32_t p, uint32_t v) { h.rows.push_back(row(h.rows.size(), type, f, p, v)); };
    op(wide, MSIM_T_INVOKE, MSIM_F_WRITE, 1, kv(0, 1)); op(wide, MSIM_T_OK, MSIM_F_WRITE, 1, kv(0, 1));
    for (uint32_t i = 0; i < 9; i++) op(wide, MSIM_T_INVOKE, MSIM_F_WRITE, 100 + i, kv(0, 10 + i));
    for (uint32_t i = 0; i < 3; i++) op(wide, MSIM_T_OK, MSIM_F_WRITE, 100 + i, kv(0, 10 + i));
    op(wide, MSIM_T_INVOKE, MSIM_F_READ, 1, kv(0, 0xFF)); op(wide, MSIM_T_OK, MSIM_F_READ, 1, kv(0, 99));
    for (uint32_t i = 3; i < 9; i++) op(wide, MSIM_T_OK, MSIM_F_WRITE, 100 + i, kv(0, 10 + i));
    for (uint32_t v : {1u, 2u}) { op(stale, MSIM_T_INVOKE, MSIM_F_WRITE, 0, kv(0, v)); op(stale, MSIM_T_OK, MSIM_F_WRITE, 0, kv(0, v)); }
    op(stale, MSIM_T_INVOKE, MSIM_F_READ, 1, kv(0, 0xFF)); op(stale, MSIM_T_OK, MSIM_F_READ, 1, kv(0, 1));
    const Offsets b({none, wide, none, stale, none});
    std::vector<msim_lin_key_result> keys(N * 4);
    std::vector<uint32_t> n_keys(N);
    report("msim_check_lin_kv_batch", msim_check_lin_kv_batch(0, b.rows.data(), b.ro.data(), N, out.data()), out);
    report("msim_explain_lin_kv_batch", msim_explain_lin_kv_batch(0, b.rows.data(), b.ro.data(), N, out.data(), keys.data(), 4, n_keys.data(), &n_host), out, &n_host);
  }
  {   // the slab entries.  pn-counter: an indeterminate add of 5000 (a window wider than the 4096-value bitmap: the host's)
    History wide, narrow, ids;
    wide.rows = {row(0, MSIM_T_OK, MSIM_F_ADD, 0, 7), row(1, MSIM_T_INFO, MSIM_F_ADD, 0, 5000), row(2, MSIM_T_OK, MSIM_F_READ, 0, 5007, 0, true), row(3, MSIM_T_OK, MSIM_F_READ, 0, 9, 0, true)};
    narrow.rows = {row(0, MSIM_T_OK, MSIM_F_ADD, 0, 1), row(1, MSIM_T_INFO, MSIM_F_ADD, 0, 2), row(2, MSIM_T_OK, MSIM_F_READ, 0, 3, 0, true)};
    const Slabs pn({none, wide, none, narrow, none});
    report("msim_check_pn_batch", msim_check_pn_batch(0, pn.rows.data(), pn.n_rows.data(), pn.max_rows, N, out.data()), out);
    for (uint32_t i = 0; i < 4; i++) { ids.rows.push_back(row(2 * i, MSIM_T_INVOKE, MSIM_F_GENERATE, i % 3, 0xFFFFFFFFu)); ids.rows.push_back(row(2 * i + 1, MSIM_T_OK, MSIM_F_GENERATE, i % 3, 5 + (i & 1))); }
    const Slabs un({none, ids, none, ids, none});
    report("msim_check_unique_batch", msim_check_unique_batch(0, un.rows.data(), un.n_rows.data(), un.max_rows, N, out.data()), out);
    {   // the explained verdicts of the three small checkers: the pn history the host explains beside one of the device's, duplicated ids, echo errors
      std::vector<msim_pn_explain> ph(N);
      std::vector<msim_pn_range> pr(N * STEPS);
      report("msim_explain_pn_batch", msim_explain_pn_batch(0, pn.rows.data(), pn.n_rows.data(), pn.max_rows, N, out.data(), ph.data(), pr.data(), STEPS, &n_host), out, &n_host);
      std::printf("%-28s reads %u %u, ranges %u %u\n", "", ph[1].n_reads, ph[3].n_reads, ph[1].n_ranges, ph[3].n_ranges);
      failures += ph[1].n_ranges != 2 || ph[3].n_ranges != 2 || ph[0].n_ranges != 1;
      std::vector<msim_unique_explain> uh(N);
      std::vector<msim_unique_dup> ud(N * STEPS);
      report("msim_explain_unique_batch", msim_explain_unique_batch(0, un.rows.data(), un.n_rows.data(), un.max_rows, N, out.data(), uh.data(), ud.data(), STEPS, &n_host), out, &n_host);
      std::printf("%-28s duplicated ids %u %u\n", "", uh[1].n_dups, uh[3].n_dups);
      failures += uh[1].n_dups != 2 || ud[STEPS].id != 6 || ud[STEPS].second_row != 7;
      History echoes;
      echoes.rows = {row(0, MSIM_T_INVOKE, MSIM_F_ECHO, 0, 1), row(1, MSIM_T_INVOKE, MSIM_F_ECHO, 1, 2), row(2, MSIM_T_OK, MSIM_F_ECHO, 1, 3), row(3, MSIM_T_FAIL, MSIM_F_ECHO, 0, 1)};
      const Slabs ec({none, echoes, none, echoes, none});
      std::vector<msim_echo_explain> eh(N);
      std::vector<msim_echo_error> ee(N * STEPS);
      report("msim_explain_echo_batch", msim_explain_echo_batch(0, 3, ec.rows.data(), ec.n_rows.data(), ec.max_rows, N, out.data(), eh.data(), ee.data(), STEPS, &n_host), out, &n_host);
      std::printf("%-28s errors %u %u\n", "", eh[1].n_errors, eh[3].n_errors);
      failures += eh[1].n_errors != 2 || ee[STEPS + 1].complete_row != 2;
    }
    std::vector<msim_perf_result> perf(N);
    std::vector<msim_latency_dist> windows((size_t)N * 4 * MSIM_PERF_MAX_F * 3);
    int rc = msim_check_perf_batch(0, un.rows.data(), un.n_rows.data(), un.max_rows, N, 3, 0, 0, perf.data(), nullptr);
    std::printf("%-28s rc %d\n", "msim_check_perf_batch", rc); failures += rc != MSIM_OK;
    rc = msim_check_perf_batch(0, un.rows.data(), un.n_rows.data(), un.max_rows, N, 3, 1, 4, perf.data(), windows.data());
    std::printf("%-28s rc %d (4 windows)\n", "msim_check_perf_batch", rc); failures += rc != MSIM_OK;
  }
  return failures ? 1 : 0;
}
