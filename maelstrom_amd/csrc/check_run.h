// check_run.h — the host side the checkers share (checker.hip, lin / txn / rw / kafka / pn / unique / perf _check_dev.hip, and the host
// checkers lin / txn / kafka / pn _check.cpp): device buffers that free themselves, the grow-only workspace, a caller's histories
// uploaded and the frame of a batch entry, the chunked pass, the slabs of an explanation, the hand-off of what the device leaves to the
// host checkers, the checker on the host cores, the frames of msim_check_*_device and msim_explain_*.  Host only: nothing here is seen
// by a kernel (the device side is check_dev.h).  A new checker mode supplies its kernel launch and its host callable; docs/KERNELS.md,
// "the host side of the device checkers".
#ifndef MSIM_CHECK_RUN_H
#define MSIM_CHECK_RUN_H

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "engine_internal.h"

// A device allocation of msim_dev_malloc that is freed with its owner (move-only).
class DevBuf {
  void *p_ = nullptr;
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
  ~DevBuf() { reset(); }
  void reset() { if (p_) (void)msim_dev_free(p_); p_ = nullptr; }
  hipError_t alloc(size_t bytes) { reset(); return msim_dev_malloc(&p_, bytes); }
  // room for `bytes` (at least one row's) with src's `bytes` copied there
  hipError_t upload(const void *src, size_t bytes) {
    const hipError_t e = alloc(bytes ? bytes : sizeof(msim_op));
    return e == hipSuccess && bytes ? hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice) : e;
  }
  template <typename T> T *get() const { return static_cast<T *>(p_); }
  void **addr() { return &p_; }   // for grow_ws
};

// the grow-only workspace: *buf holds at least `need` bytes afterwards (what it held before is not kept)
static inline int grow_ws(msim_ctx *ctx, void **buf, size_t *cap, size_t need) {
  if (*cap >= need) return MSIM_OK;
  if (*buf) (void)msim_dev_free(*buf);
  *buf = nullptr; *cap = 0;
  MSIM_HIP_TRY(ctx, msim_dev_malloc(buf, need));
  *cap = need;
  return MSIM_OK;
}

// a batch entry's stand-in for the context of a run: only for error text (and the device lin-kv's host workers select)
struct BatchCtx : msim_ctx { explicit BatchCtx(int dev) { device = dev; } };

// A caller's histories in the offsets layout, on the device: rows (payload words) of history i at row_offsets[i] (payload_offsets[i]).
struct OffsetsBatch {
  DevBuf rows, pay, row_off, pay_off;
  u32 longest = 1;   // rows of the longest history (at least 1)
  // MSIM_E_RANGE: a history of more than `limit` rows (`pay_limit` payload words; 0: not looked at).  payload_offsets null: rows only.
  int upload(msim_ctx *ctx, const msim_op *h_rows, const uint64_t *row_offsets, const u32 *payload, const uint64_t *payload_offsets, u32 n,
             uint64_t limit, uint64_t pay_limit = 0) {
    for (u32 i = 0; i < n; i++) {
      const uint64_t c = row_offsets[i + 1] - row_offsets[i];
      if (c > limit || (pay_limit && payload_offsets[i + 1] - payload_offsets[i] > pay_limit)) return MSIM_E_RANGE;
      if (c > longest) longest = (u32)c;
    }
    MSIM_HIP_TRY(ctx, rows.upload(h_rows, (size_t)row_offsets[n] * sizeof(msim_op)));
    MSIM_HIP_TRY(ctx, row_off.upload(row_offsets, (size_t)(n + 1) * 8));
    if (!payload_offsets) return MSIM_OK;
    MSIM_HIP_TRY(ctx, pay.upload(payload, payload ? (size_t)payload_offsets[n] * 4 : 0));
    MSIM_HIP_TRY(ctx, pay_off.upload(payload_offsets, (size_t)(n + 1) * 8));
    return MSIM_OK;
  }
};

// A caller's histories in the slab layout, on the device: history i in rows + i * max_rows, n_rows[i] of them used; the
// msim_inst_meta records of a run made up for them.  With max_pay, the payload words alike: history i's in payload + i * max_pay.
struct SlabBatch {
  DevBuf rows, meta, pay;
  int upload(msim_ctx *ctx, const msim_op *h_rows, const u32 *n_rows, u32 max_rows, u32 n) {   // MSIM_E_RANGE: n_rows[i] > max_rows
    std::vector<msim_inst_meta> hm(n);
    for (u32 i = 0; i < n; i++) { std::memset(&hm[i], 0, sizeof hm[i]); if (n_rows[i] > max_rows) return MSIM_E_RANGE; hm[i].n_rows = n_rows[i]; }
    MSIM_HIP_TRY(ctx, rows.upload(h_rows, (size_t)n * max_rows * sizeof(msim_op)));
    MSIM_HIP_TRY(ctx, meta.upload(hm.data(), (size_t)n * sizeof(msim_inst_meta)));
    return MSIM_OK;
  }
  int upload_payload(msim_ctx *ctx, const u32 *payload, u32 max_pay, u32 n) {   // (max_pay 0: an allocation all the same, the kernels are handed a pointer)
    MSIM_HIP_TRY(ctx, pay.upload(payload, (size_t)n * max_pay * 4));
    return MSIM_OK;
  }
};

// The frame of a batch entry, behind its argument checks: the stand-in context, the caller's histories on the device (B: OffsetsBatch
// or SlabBatch; begin passes B::upload its arguments) and the slab of n records of `rec_bytes` the kernels write.
template <class B> struct BatchFrame {
  BatchCtx ctx;
  B b;
  DevBuf d_out;
  explicit BatchFrame(int device) : ctx(device) {}
  template <class... A> int begin(u32 n, size_t rec_bytes, const A &...upload_args) {
    if (hipSetDevice(ctx.device) != hipSuccess) return MSIM_E_HIP;
    if (int rc = b.upload(&ctx, upload_args...)) return rc;
    MSIM_HIP_TRY(&ctx, d_out.alloc((size_t)n * rec_bytes));
    return MSIM_OK;
  }
  // (of a checker's *Params over an OffsetsBatch with payload: they name these alike)
  template <class P> void bind(P &p) const {
    p.rows = b.rows.template get<msim_op>(); p.payload = b.pay.template get<u32>(); p.row_off = b.row_off.template get<uint64_t>(); p.pay_off = b.pay_off.template get<uint64_t>();
    p.out = d_out.get<msim_check_result>();
  }
};

// histories per launch: as many as `budget` bytes of workspace hold at `bytes_per_history`; MSIM_DEV_FLAGS bit 16 (0x10000): at most 7,
// so that small batches reach the chunk loops (a partial last chunk, first > 0)
static inline u32 chunk_for(u32 n, uint64_t bytes_per_history, uint64_t budget, uint32_t flags) {
  return (u32)std::min<uint64_t>({n, (flags & 0x10000u) ? 7 : ~0ull, std::max<uint64_t>(1, budget / bytes_per_history)});
}

// launch(first, count) for every chunk of n, until one fails (*err); returns the launches made
template <class F> static inline u32 for_chunks(u32 n, u32 chunk, hipError_t *err, F launch) {
  u32 launches = 0;
  *err = hipSuccess;
  for (u32 first = 0; first < n && *err == hipSuccess; first += chunk, launches++) { launch(first, std::min(chunk, n - first)); *err = hipGetLastError(); }
  return launches;
}

// the histories whose record says pred(valid): what the next pass (or the host) still has to do
template <class P> static inline std::vector<u32> needs(const msim_check_result *h_out, u32 n, P pred) {
  std::vector<u32> todo;
  for (u32 i = 0; i < n; i++) if (pred(h_out[i].valid)) todo.push_back(i);
  return todo;
}

// developer: the passes' times on stderr (MSIM_DEV_FLAGS bit 12)
struct PassTimer {
  const bool trace;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit PassTimer(const msim_ctx *ctx) : trace((msim_dev_flags(ctx) & 0x1000u) != 0) {}
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Where n histories lie on the device: the slabs of a run with the meta records on the host (hmeta), or a caller's offsets.
struct HistorySource {
  const msim_op *rows; const u32 *payload;   // payload null: rows only
  const std::vector<msim_inst_meta> *hmeta; u32 max_rows, max_pay;
  const uint64_t *row_off, *pay_off;
};
// (of a checker's *Params: they name these alike)
template <class P> static inline HistorySource source_of(const P &p, const std::vector<msim_inst_meta> *hmeta) {
  return HistorySource{p.rows, p.payload, hmeta, p.max_rows, p.max_pay, p.row_off, p.pay_off};
}

// The host checkers on one history, on the calling thread: what a hand-off's `analyse` calls (lin_check.cpp, txn_check.cpp,
// kafka_check.cpp, pn_check.cpp).
void msim_lin_check_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res);
void msim_lin_explain_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res, msim_lin_key_result *keys, uint32_t max_keys,
                                    uint32_t *n_keys);
void msim_txn_check_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, uint32_t cm,
                                  msim_check_result *res);
void msim_rw_check_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, uint32_t cm,
                                 msim_check_result *res);
void msim_txn_explain_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, uint32_t cm, msim_check_result *res,
                                    msim_cycle_result *cycle, msim_cycle_step *steps, uint32_t max_steps, bool rw);
void msim_txn_findings_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, uint32_t cm, msim_check_result *res,
                                     msim_txn_explain *hdr, msim_txn_finding *findings, uint32_t max_findings, bool rw);
void msim_kafka_check_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, msim_check_result *out);
void msim_kafka_explain_instance_host(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, uint32_t flags, msim_check_result *out,
                                      msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings);
void msim_pn_check_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res);
void msim_pn_explain_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res, msim_pn_explain *hdr, void *records, uint32_t max_records);
void msim_unique_explain_instance_host(const msim_op *rows, uint32_t n_rows, uint32_t flags, msim_check_result *res, msim_unique_explain *hdr, msim_unique_dup *dups,
                                       uint32_t max_dups);

// The hand-off: the rows and payload words of the histories `todo` come to the host, analyse(rows, n_rows, payload, n_words, flags, i)
// — which writes h_out[i] — runs on up to msim_host_threads() threads, the finished records go back to d_out + i.  (R: the record of
// a history — msim_check_result, or journal_dev.hip's msim_journal_summary over journals, whose 16-byte events go as rows.)
template <class R, class F>
static inline int hand_off(msim_ctx *ctx, const HistorySource &s, u32 n, const std::vector<u32> &todo, const R *h_out, R *d_out, F analyse) {
  if (todo.empty()) return MSIM_OK;
  std::vector<uint64_t> ro, po;
  if (!s.hmeta) {
    ro.resize(n + 1); po.resize(n + 1);
    MSIM_HIP_TRY(ctx, hipMemcpy(ro.data(), s.row_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
    if (s.payload) MSIM_HIP_TRY(ctx, hipMemcpy(po.data(), s.pay_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
  }
  auto n_rows = [&](u32 i) { return s.hmeta ? (*s.hmeta)[i].n_rows : (u32)(ro[i + 1] - ro[i]); };
  auto n_words = [&](u32 i) { return !s.payload ? 0u : s.hmeta ? (*s.hmeta)[i].n_payload_words : (u32)(po[i + 1] - po[i]); };
  std::vector<std::vector<msim_op>> rows(todo.size());
  std::vector<std::vector<u32>> pays(todo.size());
  for (size_t k = 0; k < todo.size(); k++) {
    const u32 i = todo[k], nr = n_rows(i), nw = n_words(i);
    rows[k].resize(nr ? nr : 1); pays[k].resize(nw ? nw : 1);
    if (nr) MSIM_HIP_TRY(ctx, hipMemcpy(rows[k].data(), s.rows + (s.hmeta ? (uint64_t)i * s.max_rows : ro[i]), (size_t)nr * sizeof(msim_op), hipMemcpyDeviceToHost));
    if (nw) MSIM_HIP_TRY(ctx, hipMemcpy(pays[k].data(), s.payload + (s.hmeta ? (uint64_t)i * s.max_pay : po[i]), (size_t)nw * 4, hipMemcpyDeviceToHost));
  }
  unsigned nt = msim_host_threads();
  if (nt > todo.size()) nt = (unsigned)todo.size();
  std::vector<std::thread> th;
  for (unsigned w = 0; w < nt; w++)
    th.emplace_back([&, w]() {
      for (size_t k = w; k < todo.size(); k += nt) {
        const u32 i = todo[k];
        analyse(rows[k].data(), n_rows(i), pays[k].data(), n_words(i), s.hmeta ? (*s.hmeta)[i].flags : 0u, i);
      }
    });
  for (auto &x : th) x.join();
  for (u32 i : todo) MSIM_HIP_TRY(ctx, hipMemcpy(d_out + i, &h_out[i], sizeof(R), hipMemcpyHostToDevice));
  return MSIM_OK;
}

// The explanation of an explaining check: an optional header record per history (Hdr; void: records only, lin-kv's keys) and max_k
// records per history (Rec) in two device slabs, cleared on the stream before the kernels that fill them and copied to the caller's
// arrays behind them.  A max_k of 0 keeps one record allocated (the kernels are handed a pointer) and neither clears nor copies it.
template <class T> struct SizeOr0 { static constexpr size_t value = sizeof(T); };
template <> struct SizeOr0<void> { static constexpr size_t value = 0; };
template <class Hdr, class Rec> struct ExplainSlabs {
  static constexpr size_t hdr_size = SizeOr0<Hdr>::value;
  DevBuf h, r;
  u32 n = 0, max_k = 0;
  Hdr *h_hdr = nullptr; Rec *h_rec = nullptr;   // the caller's arrays
  size_t hdr_bytes() const { return (size_t)n * hdr_size; }
  size_t rec_bytes() const { return (size_t)n * max_k * sizeof(Rec); }
  int alloc(msim_ctx *ctx, u32 n_, u32 max_k_, Hdr *hdr, Rec *rec) {
    n = n_; max_k = max_k_; h_hdr = hdr; h_rec = rec;
    if (hdr_bytes()) MSIM_HIP_TRY(ctx, h.alloc(hdr_bytes()));
    MSIM_HIP_TRY(ctx, r.alloc(std::max(rec_bytes(), sizeof(Rec))));
    return MSIM_OK;
  }
  Hdr *hdr() const { return h.get<Hdr>(); }   // on the device
  Rec *rec() const { return r.get<Rec>(); }
  Hdr *hdr(u32 i) const { return h_hdr + i; }   // history i's, in the caller's arrays
  Rec *rec(u32 i) const { return h_rec + (size_t)i * max_k; }
  int clear(msim_ctx *ctx, hipStream_t st) {
    if (hdr_bytes()) MSIM_HIP_TRY(ctx, hipMemsetAsync(h.get<void>(), 0, hdr_bytes(), st));
    if (rec_bytes()) MSIM_HIP_TRY(ctx, hipMemsetAsync(r.get<void>(), 0, rec_bytes(), st));
    return MSIM_OK;
  }
  int fetch(msim_ctx *ctx, hipStream_t st) {
    if (hdr_bytes()) MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_hdr, h.get<void>(), hdr_bytes(), hipMemcpyDeviceToHost, st));
    if (rec_bytes()) MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_rec, r.get<void>(), rec_bytes(), hipMemcpyDeviceToHost, st));
    MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
    return MSIM_OK;
  }
};

// the witness cycles of an explaining rw / txn check: a cycle record, max_steps steps per history
typedef ExplainSlabs<msim_cycle_result, msim_cycle_step> CycleSlabs;
template <class P> static inline void bind_cycles(P &p, const CycleSlabs &w) { p.cycles = w.hdr(); p.steps = w.rec(); p.max_steps = w.max_k; }

// how rw_dev_run / txn_dev_run go beyond the clean passes: `full` the classification on the device; with `witness` its EXPLAIN kernel
// the non-cycle findings of an explaining rw / txn check (include/maelsim_txn_findings.h): a header, max_findings records per history
typedef ExplainSlabs<msim_txn_explain, msim_txn_finding> FindingSlabs;
struct CycleMode {
  bool full = false;
  CycleSlabs *witness = nullptr;
  FindingSlabs *findings = nullptr;   // (instead of the witness: the *_findings_kernel flavour)
};
// rw_check_dev.hip's share of msim_explain_txn_findings_batch / msim_explain_txn_findings (txn_check_dev.hip holds the entries)
int msim_rw_findings_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets, uint32_t n_histories,
                           uint32_t consistency_model, msim_check_result *out, uint32_t *n_host, msim_txn_explain *hdr, msim_txn_finding *findings, uint32_t max_findings);
int msim_rw_findings_device(msim_ctx *ctx, msim_txn_explain *hdr, msim_txn_finding *findings, uint32_t max_findings);

// One chunked pass over `m` histories — all of the launch, or those `list` names (m of them: the list goes to the device in front of the
// workspace, rounded to 256 bytes) —, each with `bytes_per_history` of the grow-only workspace, as many per launch as `budget` holds:
// launch(d_list, ws, first, count) for every chunk, then the n records of the launch to h_out, waited for.  Returns the launches made,
// or an error (< 0).
template <class F, class R>
static inline int chunked_pass(msim_ctx *ctx, u32 m, uint64_t bytes_per_history, uint64_t budget, const std::vector<u32> *list, void **ws_buf, size_t *ws_cap, F launch,
                               const R *d_out, R *h_out, u32 n, hipStream_t st) {
  const size_t list_bytes = list ? ((size_t)m * 4 + 255) & ~(size_t)255 : 0;
  const u32 chunk = chunk_for(m, bytes_per_history, budget, msim_dev_flags(ctx));
  if (int rc = grow_ws(ctx, ws_buf, ws_cap, list_bytes + (size_t)chunk * bytes_per_history)) return rc;
  if (list) MSIM_HIP_TRY(ctx, hipMemcpyAsync(*ws_buf, list->data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  const u32 *const d_list = list ? static_cast<const u32 *>(*ws_buf) : nullptr;
  void *const ws = static_cast<char *>(*ws_buf) + list_bytes;
  hipError_t e;
  const u32 launches = for_chunks(m, chunk, &e, [&](u32 first, u32 count) { launch(d_list, ws, first, count); });
  MSIM_HIP_TRY(ctx, e);
  MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(R), hipMemcpyDeviceToHost, st));
  MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
  return (int)launches;
}

// The frame of msim_check_{rw,txn,kafka,pn}_device.  begin_check: the pinned records of the run anew; with `hm`, the meta records on the
// host — behind the context's stream: the simulation may still be running (msim_run_async), the context's stream does not block against
// the null stream, so the copy of the meta is ordered behind it here and by nothing else.  Returns in *t0 where check_ms starts.
static inline int renew_h_check(msim_ctx *ctx) {
  if (ctx->h_check) { (void)hipHostFree(ctx->h_check); ctx->h_check = nullptr; }
  MSIM_HIP_TRY(ctx, hipHostMalloc(&ctx->h_check, (size_t)ctx->n_inst * sizeof(msim_check_result)));
  return MSIM_OK;
}
static inline int begin_check(msim_ctx *ctx, std::chrono::steady_clock::time_point *t0, std::vector<msim_inst_meta> *hm) {
  const u32 n = ctx->n_inst;
  if (int rc = renew_h_check(ctx)) return rc;
  if (hm) MSIM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *t0 = std::chrono::steady_clock::now();
  if (hm) { hm->resize(n); MSIM_HIP_TRY(ctx, hipMemcpy(hm->data(), ctx->d_meta, (size_t)n * sizeof(msim_inst_meta), hipMemcpyDeviceToHost)); }
  return MSIM_OK;
}
static inline void finish_check(msim_ctx *ctx, std::chrono::steady_clock::time_point t0, u32 redone) {
  ctx->check_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ctx->lin_host_rechecks = redone;
  ctx->checked = true; ctx->check_fetched = true;
}

// The checker on the host cores (msim_check under developer flag 0x800, and where a device checker does not take a configuration): the
// histories of the last run fetched, analyse(state, i, rows, n_rows, payload, n_words, flags, &h_check[i]) for every history i on up to
// msim_host_threads() threads that stride over them — `state` one make_state() per thread, made on the calling thread before the first
// starts —, the records to d_check.  check_ms is all of it, the fetch included; lin_host_rechecks is the caller's.  times (may be null):
// the fetch, the threads' work, their number.
struct HostRunTimes { float fetch_ms = 0.f, work_ms = 0.f; unsigned threads = 0; };
template <class M, class A> static inline int host_check_run(msim_ctx *ctx, M make_state, A analyse, HostRunTimes *times = nullptr) {
  typedef std::chrono::duration<float, std::milli> ms;
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = msim_fetch(ctx)) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  const u32 n = ctx->n_inst;
  if (int rc = renew_h_check(ctx)) return rc;
  const unsigned nt = std::min<unsigned>(msim_host_threads(), n);
  std::vector<decltype(make_state())> states;
  for (unsigned t = 0; t < nt; t++) states.push_back(make_state());
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++)
    th.emplace_back([&, t]() {
      auto state = std::move(states[t]);   // (on this thread's stack: the threads' states do not share cache lines)
      for (u32 i = t; i < n; i += nt) {
        const msim_inst_meta &m = ctx->h_meta[i];
        analyse(state, i,ctx->h_rows + ctx->h_row_off[i], m.n_rows, ctx->h_payload + ctx->h_pay_off[i], m.n_payload_words, m.flags, &ctx->h_check[i]);
      }
    });
  for (auto &x : th) x.join();
  const auto t2 = std::chrono::steady_clock::now();
  MSIM_HIP_TRY(ctx, hipMemcpy(ctx->d_check, ctx->h_check, (size_t)n * sizeof(msim_check_result), hipMemcpyHostToDevice));
  ctx->checked = true; ctx->check_fetched = true;
  ctx->check_ms = ms(std::chrono::steady_clock::now() - t0).count();
  if (times) *times = HostRunTimes{ms(t1 - t0).count(), ms(t2 - t1).count(), nt};
  return MSIM_OK;
}

// What the msim_explain_* entries of a run refuse alike, in this order: a context of another workload (`what`: "a lin-kv", ...), nothing
// run yet, output arrays shorter than the run.  (Their null arguments differ and stay with each.)
static inline int explain_refusal(msim_ctx *ctx, const char *entry, bool workload_ok, const char *what, u32 n_out) {
  if (!workload_ok) { ctx->err = std::string(entry) + ": not " + what + " context"; return MSIM_E_UNSUPPORTED; }
  if (!ctx->ran) { ctx->err = std::string(entry) + " before msim_run"; return MSIM_E_RANGE; }
  if (n_out < ctx->n_inst) { ctx->err = std::string(entry) + ": output arrays shorter than the run"; return MSIM_E_RANGE; }
  return MSIM_OK;
}

#endif
