// checker.hip — workload checkers at ensemble scale, on the device.
//
// The reference hands each history to `(checker/check (:checker test) test history opts)` (core.clj:91-100).
// For broadcast / g-set that is jepsen's `checker/set-full` (workload/broadcast.clj:216-228 maps
// :broadcast -> :add; workload/g_set.clj:62); for echo the pair comparison of workload/echo.clj:44-63;
// checker/stats counts ok/fail/info.  [upstream] jepsen.checker/set-full is restated here from its
// published algorithm (result-map shape: doc/03-broadcast/01-broadcast.md:564-577):
//   per element: known        = first :ok add completion or first :ok read containing it
//                last-present = latest-invoked :ok read containing it (by invoke :index)
//                last-absent  = latest-invoked :ok read (completed after the add's invoke) lacking it
//   stable  <=> last-present and index(last-absent, -1) < index(last-present)
//   lost    <=> known and last-absent and index(last-present, -1) < index(last-absent) and index(known) < index(last-absent)
//   stable-latency = long(nanos->ms(max(0, (time(last-absent)+1 | 0) - time(known))));  stale <=> stable-latency > 0
//   :valid? = false if any lost, :unknown if nothing stable, else true
//   :stable-latencies = points {0 .5 .95 .99 1} -> sorted[min(n-1, floor(n*q))]
//
// One wavefront checks one history, bit-parallel over the read bitmaps:
//   pass 1  rows are read back from HBM 64 at a time (1 KiB, coalesced, the next chunk in flight); every lane classifies its own
//           row.  A completion is paired with its invocation — the previous row of the same worker thread — without a serial walk
//           (round 2 walked the read rows one by one with v_readlane: 2/3 of the kernel's instructions were scalar): the read rows of
//           a chunk are taken in rounds, in each round the EARLIEST pending row of every worker thread (ds_min over the thread's
//           slot) acts on the thread's table entry in LDS — an invocation leaves {row, rank}, a completion takes it — so a chunk costs
//           as many rounds as its busiest thread has read rows in it (2-3), not one step per row.  A read :ok RECORDS itself at the
//           rank of its invocation {payload ref, invoke index, elements existing at completion, :ok index} (12 B, HBM scratch).  Four chunks
//           of rows are in flight.
//   pass 2  ONE sweep over the recorded reads in invocation order, 64 reads at a time, lane r = read r of the chunk (round 6; before: lane w =
//           word w of one read's bitmap at a time).  Every lane loads its own read's bitmap 16 bytes at a time; per word the highest / lowest
//           lane with a bit decides all its bits at once, words every read of the chunk holds completely are only noted — see the comment
//           at the sweep.
// Per-element state: three u16 row indices in LDS (8.4 KB for 1408 elements keeps 4096 histories resident).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "check_dev.h"
#include "check_run.h"
#include "engine_internal.h"

#define NONE 0xFFFFu      /* per-element row index: none */
#define NONE32 0xFFFFFFFFu /* per-thread table entry: no invocation pending */
#define NOLAT 0xFFFFFFFFu  /* per-element latency: not stable */

struct CParams {
  const msim_op *rows;
  const u32 *payload;
  const msim_inst_meta *meta;
  msim_check_result *out;
  u32 *recs;    // per instance: max_reads records of 3 words, at the rank of the read's invocation
  u32 max_rows, max_pay, max_values, C, workload, max_reads;
  u32 off_valid, off_tbl;   // LDS offsets (bytes): the valid bitmap, the per-thread tables
  float rcp_C;
};
// what set_explain_kernel writes beside p.out (msim_explain_set_full*; include/maelsim.h msim_set_explain): check_kernel has an empty one
struct SetExplainOut {
  msim_set_explain *hdr;        // one per history
  msim_set_element *elements;   // per history: max_elements records, zeroed by the host
  u32 max_elements;
  u32 off_lat;                  // LDS offset (bytes) of the two latency arrays: the u16 row indices stay where they are
};

#ifdef MSIM_HIPEMU
struct __attribute__((packed, aligned(4))) ck_u32x4 { u32 x, y, z, w; };
#else
typedef u32 ck_u32x4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes of a u32 array from any word on: global memory takes one dwordx4 at a 4-byte boundary
#endif
__device__ __forceinline__ u32 c_rdlane(u32 v, u32 l) { return (u32)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ u32 c_wave_sum(u32 v) {
  for (int o = 32; o; o >>= 1) v += (u32)__shfl_xor((int)v, o);
  return v;
}

// maximum over the 64 lanes (uniform) / inclusive prefix maximum, by DPP
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ u32 c_dpp(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, BOUND); }
__device__ __forceinline__ u32 c_wave_incl_max(u32 v) {
  v = max(v, c_dpp<0x111, 0xF, true>(v));   // row_shr:1 (lanes without a source read 0)
  v = max(v, c_dpp<0x112, 0xF, true>(v));   // row_shr:2
  v = max(v, c_dpp<0x114, 0xF, true>(v));   // row_shr:4
  v = max(v, c_dpp<0x118, 0xF, true>(v));   // row_shr:8
  v = max(v, c_dpp<0x142, 0xA, false>(v));  // row_bcast:15 -> rows 1, 3
  v = max(v, c_dpp<0x143, 0xC, false>(v));  // row_bcast:31 -> rows 2, 3
  return v;
}
// OR over the lanes BELOW this one
__device__ __forceinline__ u32 c_wave_excl_or(u32 v) {
  v = c_dpp<0x138, 0xF, true>(v);           // wave_shr:1 (lane 0 reads 0)
  v |= c_dpp<0x111, 0xF, true>(v);
  v |= c_dpp<0x112, 0xF, true>(v);
  v |= c_dpp<0x114, 0xF, true>(v);
  v |= c_dpp<0x118, 0xF, true>(v);
  v |= c_dpp<0x142, 0xA, false>(v);
  v |= c_dpp<0x143, 0xC, false>(v);
  return v;
}
// orders this wavefront's LDS traffic across its lanes (LDS operations of one wavefront execute in order: the compiler must not move them)
__device__ __forceinline__ void c_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ u32 c_wave_max(u32 v) { return c_rdlane(c_wave_incl_max(v), 63); }

__global__ void __launch_bounds__(64) check_kernel(const CParams p) {
  constexpr bool EXPLAIN = false;
  const SetExplainOut x = SetExplainOut();
#include "set_full_body.inc"
}
// The same check with its explanation (msim_explain_set_full*): the lost / never-read / stale elements, the eight stalest, the lost
// latencies.  Set-full only (the entries refuse echo).
__global__ void __launch_bounds__(64) set_explain_kernel(const CParams p, const SetExplainOut x) {
  constexpr bool EXPLAIN = true;
#include "set_full_body.inc"
}

// The launch's derived parameters and the LDS of one wavefront: three u16 indices per element (reused as one u32 latency per element),
// the valid bitmap over the read ranks (read one word past the last chunk), the per-thread tables slot / first / slotv.
// set_explain_kernel (off_lat given) keeps the indices and has two u32 latencies per element behind them.
static size_t check_layout(CParams &cp, u32 *off_lat = nullptr) {
  cp.max_reads = cp.max_rows / 2 + 1;  // every :ok read has its own :invoke row
  cp.rcp_C = 1.0f / (float)cp.C;
  size_t lds = (size_t)cp.max_values * 3 * 2 < (size_t)cp.max_values * 4 ? (size_t)cp.max_values * 4 : (size_t)cp.max_values * 3 * 2;
  lds = (lds + 3) & ~(size_t)3;
  if (off_lat) { lds = ((size_t)cp.max_values * 3 * 2 + 3) & ~(size_t)3; *off_lat = (u32)lds; lds += (size_t)cp.max_values * 2 * 4; }
  cp.off_valid = (u32)lds;
  lds += ((size_t)(cp.max_reads + 31) / 32 + 2) * 4;
  cp.off_tbl = (u32)lds;
  lds += (size_t)cp.C * 3 * 4;
  return lds;
}

static const char *check_limits(u32 max_rows, u32 max_values, u32 concurrency) {
  if (max_rows >= 0xFFFF || max_values > 2048 || concurrency > 128 || concurrency == 0) return "device checker: max_rows must be < 65535, max_values <= 2048, concurrency 1..128";
  return nullptr;
}

// `kernel` (check_kernel over cp; set_explain_kernel over cp and x, whose header and element slabs the caller has cleared) with `lds`
// bytes of check_layout, one wavefront per history over n slabs; the caller owns the buffers and the stream
template <class K, class... A> static hipError_t check_dispatch(K kernel, size_t lds, u32 n, hipStream_t st, const A &...args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(n), dim3(64), lds, st, args...);
  return hipGetLastError();
}

// the parameters of a check over n slabs as a configuration lays them out (the slabs themselves, out and recs: the caller's)
static CParams check_params(u32 workload, u32 concurrency, u32 max_rows, u32 max_pay, u32 max_values) {
  CParams cp;
  std::memset(&cp, 0, sizeof cp);
  cp.max_rows = max_rows; cp.max_pay = max_pay; cp.max_values = max_values; cp.C = concurrency; cp.workload = workload;
  return cp;
}
static CParams check_params(const msim_ctx *ctx) {
  const msim_config &c = ctx->cfg;
  CParams cp = check_params(c.workload, c.concurrency, c.max_rows, c.max_payload_words, c.max_values);
  cp.rows = ctx->d_rows; cp.payload = ctx->d_payload; cp.meta = ctx->d_meta; cp.out = ctx->d_check;
  return cp;
}
typedef ExplainSlabs<msim_set_explain, msim_set_element> SetSlabs;   // a header, max_elements element records per history
static SetExplainOut set_explain_out(const SetSlabs &xs) {
  SetExplainOut x;
  std::memset(&x, 0, sizeof x);
  x.hdr = xs.hdr(); x.elements = xs.rec(); x.max_elements = xs.max_k;
  return x;
}

// d_check_scratch for n histories: the read records of every instance.  Frees and allocates when it has to grow — a hipFree waits for
// the whole device —, so run_impl calls it in front of the simulation whose check it is about to queue, never between the two.
int msim_check_reserve(msim_ctx *ctx, uint32_t n) {
  const size_t rec_bytes = (size_t)n * (ctx->cfg.max_rows / 2 + 1) * 3 * sizeof(u32);
  if (ctx->cap_check_scratch < rec_bytes) {
    if (ctx->d_check_scratch) (void)msim_dev_free(ctx->d_check_scratch);
    ctx->d_check_scratch = nullptr; ctx->cap_check_scratch = 0;
    MSIM_HIP_TRY(ctx, msim_dev_malloc(&ctx->d_check_scratch, rec_bytes));
    ctx->cap_check_scratch = rec_bytes;
  }
  return MSIM_OK;
}

// Queues the checker over the slabs of the last run on `stream`, between ev2 and ev3, and returns: it never waits.  Behind the
// simulation kernel on the same stream (run_impl) it reads what that kernel wrote; it writes d_check and d_check_scratch only.
int msim_check_enqueue(msim_ctx *ctx, hipStream_t stream) {
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const msim_config &c = ctx->cfg;
  CParams cp = check_params(ctx);
  if (const char *why = check_limits(c.max_rows, c.max_values, c.concurrency)) { ctx->err = why; return MSIM_E_UNSUPPORTED; }
  const int rc = msim_check_reserve(ctx, ctx->n_inst);   // (run_impl has sized it already where the check follows its simulation)
  if (rc != MSIM_OK) return rc;
  cp.recs = static_cast<u32 *>(ctx->d_check_scratch);
  const size_t lds = check_layout(cp);
  MSIM_HIP_TRY(ctx, hipEventRecord(ctx->ev2, stream));
  MSIM_HIP_TRY(ctx, check_dispatch(check_kernel, lds, ctx->n_inst, stream, cp));
  MSIM_HIP_TRY(ctx, hipEventRecord(ctx->ev3, stream));
  return MSIM_OK;
}

// The other half: waits for the queued checker and makes its records visible (msim_check_results refuses until then).
int msim_check_wait(msim_ctx *ctx) {
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MSIM_HIP_TRY(ctx, hipEventSynchronize(ctx->ev3));
  MSIM_HIP_TRY(ctx, hipEventElapsedTime(&ctx->check_ms, ctx->ev2, ctx->ev3));
  ctx->checked = true; ctx->check_fetched = false;
  return MSIM_OK;
}

// What msim_check and msim_explain_set_full do first: the check run_impl queued behind the simulation is taken and waited for (1: its
// records are in d_check; < 0: the wait failed); with nothing queued (0) a launch on the context's own stream arms the context, so that
// its next launches queue theirs.
int msim_check_take_or_arm(msim_ctx *ctx) {
  const uint32_t flags = msim_dev_flags(ctx);
  if (ctx->check_queued) {
    ctx->check_queued = false;
    if (flags & 0x1000u) std::fprintf(stderr, "[check] taken %u\n", ctx->n_inst);
    const int rc = msim_check_wait(ctx);
    return rc != MSIM_OK ? rc : 1;
  }
  if (ctx->ran_own_stream && !(flags & 0x40000u)) ctx->check_armed = true;
  return 0;
}

int msim_check_launch(msim_ctx *ctx) {
  const int rc = msim_check_enqueue(ctx, ctx->stream);
  return rc != MSIM_OK ? rc : msim_check_wait(ctx);
}

// ---- echo: the explanation of a verdict (msim_explain_echo*; include/maelsim_small_explain.h) ----------------------------------------
// check_kernel counts the invocations whose completion is not an :ok with the same value; echo_explain_kernel, a kernel of its own over
// the histories that have such an invocation (`list`), names them: one wavefront per history pairs the rows again by worker thread
// (process mod C: the table's index; a crashed process's successor, process + C, has the same entry) — in rounds, as check_kernel's
// pass 1: of a step's 64 rows the earliest pending row of every thread acts on the thread's entry, an invocation opens it, a completion
// takes it — and notes per invocation row, in LDS, how it ended; a second sweep writes the errors in row order (ballot, prefix count).
#define ECHO_FINE 0xFFFFu      /* per invocation row: no error (and every row that is no invocation) */
#define ECHO_NO_OK 0xFFFEu     /* an error without an :ok completion; any other value: the row of the :ok that carries another value */
struct EchoExplainOut { msim_echo_explain *hdr; msim_echo_error *errors; u32 max_errors; };

__global__ void __launch_bounds__(64) echo_explain_kernel(const msim_op *rows_all, const msim_inst_meta *meta, const u32 *list, u32 max_rows, u32 C, const EchoExplainOut x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char csmem[];
  u32 *const open = reinterpret_cast<u32 *>(csmem);                         // [C] the thread's open invocation row
  u32 *const first = open + C;                                              // [C] ds_min target: (round, lane) of the thread's earliest pending row
  unsigned short *const how = reinterpret_cast<unsigned short *>(first + C);   // [max_rows]
  const u32 lane = threadIdx.x, hist = list[blockIdx.x];
  const uint4 *const r = reinterpret_cast<const uint4 *>(rows_all) + (size_t)hist * max_rows;
  const u32 n = min(meta[hist].n_rows, max_rows);
  const u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes below this one
  for (u32 i = lane; i < n; i += 64) how[i] = ECHO_FINE;
  for (u32 i = lane; i < C; i += 64) { open[i] = NONE32; first[i] = 0xFFFFFFFFu; }
  __syncthreads();
  u32 round_key = 0x3FFFFFFu;   // decreases with every round: a later round's ds_min beats whatever an earlier one left
  for (u32 base = 0; base < n; base += 64) {
    const u32 idx = base + lane;
    const uint4 row = idx < n ? r[idx] : make_uint4(0, 0, 0, 0);
    const u32 type = row.z & 3u, proc = row.z >> 12;
    bool pend = idx < n && proc != MSIM_PROCESS_NEMESIS && ((row.z >> 2) & 31u) == MSIM_F_ECHO;
    const u32 tt = pend ? proc % C : 0u;
    for (u64 pm = __ballot(pend); pm; pm = __ballot(pend)) {
      const u32 key = (round_key << 6) | lane;
      if (pend) atomicMin(&first[tt], key);
      wv_fence();
      if (pend && first[tt] == key) {
        pend = false;
        const u32 s = open[tt];
        if (type == MSIM_T_INVOKE) open[tt] = idx;
        else {
          open[tt] = NONE32;
          if (s != NONE32) { if (type != MSIM_T_OK) how[s] = ECHO_NO_OK; else if (r[s].w != row.w) how[s] = (unsigned short)idx; }
        }
      }
      round_key--;
      wv_fence();
    }
  }
  __syncthreads();
  for (u32 i = lane; i < C; i += 64) if (open[i] != NONE32) how[open[i]] = ECHO_NO_OK;   // invocations left without a completion
  __syncthreads();
  uint4 *const dst = reinterpret_cast<uint4 *>(x.errors + (size_t)hist * x.max_errors);
  u32 at = 0;
  for (u32 base = 0; base < n; base += 64) {
    const u32 idx = base + lane;
    const u32 h = idx < n ? how[idx] : ECHO_FINE;
    const u64 m = __ballot(h != ECHO_FINE);
    const u32 slot = at + (u32)__popcll(m & lt);
    if (h != ECHO_FINE && slot < x.max_errors)   // (the slab's bound)
      dst[slot] = make_uint4(idx, h == ECHO_NO_OK ? MSIM_NO_VALUE : h, r[idx].w, h == ECHO_NO_OK ? MSIM_NO_VALUE : r[h].w);
    at += (u32)__popcll(m);
  }
  if (lane == 0) { x.hdr[hist].n_errors = min(at, x.max_errors); x.hdr[hist].truncated = at > x.max_errors ? 1u : 0u; }
}

// the caller's arrays of an explaining echo run: a header per history, max_errors records per history
struct EchoExplainRun { msim_echo_explain *hdr; msim_echo_error *errors; u32 max_errors; };

// Behind check_kernel (whose records lie in d_out): the histories with an error go to echo_explain_kernel.  Without one nothing is
// launched and nothing allocated.  h_out: the records, fetched here.
static int echo_explain_run(msim_ctx *ctx, const msim_op *d_rows, const msim_inst_meta *d_meta, const msim_check_result *d_out, u32 max_rows, u32 C, u32 n,
                            msim_check_result *h_out, hipStream_t st, const EchoExplainRun &xr) {
  MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(msim_check_result), hipMemcpyDeviceToHost, st));
  MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
  std::memset(xr.hdr, 0, (size_t)n * sizeof(msim_echo_explain));
  if (xr.max_errors) std::memset(xr.errors, 0, (size_t)n * xr.max_errors * sizeof(msim_echo_error));
  std::vector<u32> list;
  for (u32 i = 0; i < n; i++) if (h_out[i].error_count) list.push_back(i);
  if (list.empty()) return MSIM_OK;
  ExplainSlabs<msim_echo_explain, msim_echo_error> xs;
  DevBuf d_list;
  if (int rc = xs.alloc(ctx, n, xr.max_errors, xr.hdr, xr.errors)) return rc;
  if (int rc = xs.clear(ctx, st)) return rc;
  MSIM_HIP_TRY(ctx, d_list.upload(list.data(), list.size() * 4));
  const size_t lds = ((size_t)C * 8 + (size_t)max_rows * 2 + 3) & ~(size_t)3;
  const EchoExplainOut x{xs.hdr(), xs.rec(), xr.max_errors};
  MSIM_HIP_TRY(ctx, check_dispatch(echo_explain_kernel, lds, (u32)list.size(), st, d_rows, d_meta, static_cast<const u32 *>(d_list.get<u32>()), max_rows, C, x));
  if (msim_dev_flags(ctx) & 0x1000u) std::fprintf(stderr, "[check] echo_explain_kernel over %zu of %u histories\n", list.size(), n);
  return xs.fetch(ctx, st);   // (waits: the buffers are freed with this frame)
}

// Checks `n_histories` broadcast / g-set (set-full) or echo histories given on the host with the device checker of msim_check:
// history i lies in the slabs rows + i * max_rows (n_rows[i] rows used) and payload + i * max_payload_words.
// (hdr: msim_explain_set_full_batch's arrays — set_explain_kernel in place of check_kernel, on the same upload)
static int set_full_batch(int device, uint32_t workload, uint32_t concurrency, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows,
                          const uint32_t *payload, uint32_t max_payload_words, uint32_t max_values, uint32_t n_histories, msim_check_result *out,
                          msim_set_explain *hdr = nullptr, msim_set_element *elements = nullptr, uint32_t max_elements = 0, const EchoExplainRun *echo = nullptr) {
  if (!rows || !n_rows || !out || n_histories == 0 || max_rows == 0 || (!payload && max_payload_words)) return MSIM_E_INVALID;
  if (workload != MSIM_WL_ECHO && workload != MSIM_WL_BROADCAST && workload != MSIM_WL_G_SET) return MSIM_E_INVALID;
  if (check_limits(max_rows, max_values, concurrency)) return MSIM_E_UNSUPPORTED;
  BatchFrame<SlabBatch> f(device); msim_ctx *ctx = &f.ctx;
  if (int rc = f.begin(n_histories, sizeof(msim_check_result), rows, n_rows, max_rows, n_histories)) return rc;
  if (int rc = f.b.upload_payload(ctx, payload, max_payload_words, n_histories)) return rc;
  SetSlabs xs;
  if (hdr) if (int rc = xs.alloc(ctx, n_histories, max_elements, hdr, elements)) return rc;
  DevBuf d_rec;
  MSIM_HIP_TRY(ctx, d_rec.alloc((size_t)n_histories * (max_rows / 2 + 1) * 3 * sizeof(u32)));
  CParams cp = check_params(workload, concurrency, max_rows, max_payload_words, max_values);
  cp.rows = f.b.rows.get<msim_op>(); cp.payload = f.b.pay.get<u32>(); cp.meta = f.b.meta.get<msim_inst_meta>(); cp.out = f.d_out.get<msim_check_result>(); cp.recs = d_rec.get<u32>();
  if (hdr) {
    SetExplainOut x = set_explain_out(xs);
    if (int rc = xs.clear(ctx, nullptr)) return rc;
    const size_t lds = check_layout(cp, &x.off_lat);
    MSIM_HIP_TRY(ctx, check_dispatch(set_explain_kernel, lds, n_histories, nullptr, cp, x));
    if (int rc = xs.fetch(ctx, nullptr)) return rc;
  } else MSIM_HIP_TRY(ctx, check_dispatch(check_kernel, check_layout(cp), n_histories, nullptr, cp));
  MSIM_HIP_TRY(ctx, hipDeviceSynchronize());
  if (echo) return echo_explain_run(ctx, cp.rows, cp.meta, cp.out, max_rows, concurrency, n_histories, out, nullptr, *echo);
  MSIM_HIP_TRY(ctx, hipMemcpy(out, cp.out, (size_t)n_histories * sizeof(msim_check_result), hipMemcpyDeviceToHost));
  return MSIM_OK;
}
extern "C" int msim_check_set_full_batch(int device, uint32_t workload, uint32_t concurrency, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows,
                                         const uint32_t *payload, uint32_t max_payload_words, uint32_t max_values, uint32_t n_histories, msim_check_result *out) {
  return set_full_batch(device, workload, concurrency, rows, n_rows, max_rows, payload, max_payload_words, max_values, n_histories, out);
}

// The explaining set-full check (include/maelsim.h msim_set_explain) of a caller's histories: msim_check_set_full_batch's upload and
// records, with set_explain_kernel's header and element records per history.
extern "C" int msim_explain_set_full_batch(int device, uint32_t workload, uint32_t concurrency, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows,
                                           const uint32_t *payload, uint32_t max_payload_words, uint32_t max_values, uint32_t n_histories,
                                           msim_check_result *out, msim_set_explain *hdr, msim_set_element *elements, uint32_t max_elements) {
  if (!hdr || (!elements && max_elements) || n_histories == 0) return MSIM_E_INVALID;
  if (workload != MSIM_WL_BROADCAST && workload != MSIM_WL_G_SET) return MSIM_E_UNSUPPORTED;
  return set_full_batch(device, workload, concurrency, rows, n_rows, max_rows, payload, max_payload_words, max_values, n_histories, out, hdr, elements, max_elements);
}

// ... and of the last run where it lies in HBM.  Towards the context this is msim_check (engine.hip): a check queued behind the
// simulation is taken and waited for, a launch on the context's own stream arms the context; then the explaining kernel runs over the
// same slabs on the context's stream and leaves in d_check the records check_kernel writes.
extern "C" int msim_explain_set_full(msim_ctx *ctx, msim_set_explain *hdr, msim_set_element *elements, uint32_t max_elements, uint32_t n_out) {
  if (!ctx || !hdr || (!elements && max_elements)) return MSIM_E_INVALID;
  const msim_config &c = ctx->cfg;
  if (int rc = explain_refusal(ctx, "msim_explain_set_full", c.workload == MSIM_WL_BROADCAST || c.workload == MSIM_WL_G_SET, "a broadcast or g-set", n_out)) return rc;
  if (const char *why = check_limits(c.max_rows, c.max_values, c.concurrency)) { ctx->err = why; return MSIM_E_UNSUPPORTED; }
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = msim_check_take_or_arm(ctx);
  if (rc < 0) return rc;
  if (msim_dev_flags(ctx) & 0x1000u) std::fprintf(stderr, "[check] explain %u\n", ctx->n_inst);
  SetSlabs xs;
  if ((rc = xs.alloc(ctx, ctx->n_inst, max_elements, hdr, elements)) != MSIM_OK) return rc;
  if ((rc = msim_check_reserve(ctx, ctx->n_inst)) != MSIM_OK) return rc;
  CParams cp = check_params(ctx);
  cp.recs = static_cast<u32 *>(ctx->d_check_scratch);
  SetExplainOut x = set_explain_out(xs);
  if ((rc = xs.clear(ctx, ctx->stream)) != MSIM_OK) return rc;
  const size_t lds = check_layout(cp, &x.off_lat);
  MSIM_HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  MSIM_HIP_TRY(ctx, check_dispatch(set_explain_kernel, lds, ctx->n_inst, ctx->stream, cp, x));
  MSIM_HIP_TRY(ctx, hipEventRecord(ctx->ev3, ctx->stream));
  if ((rc = xs.fetch(ctx, ctx->stream)) != MSIM_OK) return rc;
  return msim_check_wait(ctx);
}

// The explaining echo check of a caller's histories: msim_check_set_full_batch's upload, kernel and records for MSIM_WL_ECHO (rows only:
// an echo history has no payload words), then echo_explain_kernel over the histories with an error.  *n_host (may be null): always 0.
extern "C" int msim_explain_echo_batch(int device, uint32_t concurrency, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories,
                                       msim_check_result *out, msim_echo_explain *hdr, msim_echo_error *errors, uint32_t max_errors, uint32_t *n_host) {
  if (!hdr || (!errors && max_errors) || n_histories == 0) return MSIM_E_INVALID;
  if (n_host) *n_host = 0;
  const EchoExplainRun xr{hdr, errors, max_errors};
  return set_full_batch(device, MSIM_WL_ECHO, concurrency, rows, n_rows, max_rows, nullptr, 0, 32, n_histories, out, nullptr, nullptr, 0, &xr);
}

// ... and of the last run where it lies in HBM: msim_check (queued, taken or launched as it would be), then the explanation.
extern "C" int msim_explain_echo(msim_ctx *ctx, msim_echo_explain *hdr, msim_echo_error *errors, uint32_t max_errors, uint32_t n_out) {
  if (!ctx || !hdr || (!errors && max_errors)) return MSIM_E_INVALID;
  const msim_config &c = ctx->cfg;
  if (int rc = explain_refusal(ctx, "msim_explain_echo", c.workload == MSIM_WL_ECHO, "an echo", n_out)) return rc;
  if (int rc = msim_check(ctx)) return rc;
  std::vector<msim_check_result> h_out(ctx->n_inst);
  return echo_explain_run(ctx, ctx->d_rows, ctx->d_meta, ctx->d_check, c.max_rows, c.concurrency, ctx->n_inst, h_out.data(), ctx->stream, EchoExplainRun{hdr, errors, max_errors});
}

// ---- maelstrom.checker/availability-checker (checker.clj:6-39) ---------------------------------------------------------
// :ok-fraction = (float (/ ok-count invoke-count)) over (h/oks history) and (h/invokes history) — every :ok and every :invoke row
// (nemesis ops are :info) — 1 for an empty history; :valid? by --availability (core.clj:149): nil -> true, :total -> the
// fraction == 1, a number a -> a <= fraction.  One wavefront per history counts the two row types from HBM; the verdicts are
// formed on the host (n x 2 counters cross PCIe).
__global__ void __launch_bounds__(64) availability_kernel(const msim_op *rows, const msim_inst_meta *meta, u32 max_rows, uint2 *out) {
  const u32 lane = threadIdx.x, inst = blockIdx.x;
  const u32 n = meta[inst].n_rows;
  const uint4 *r = reinterpret_cast<const uint4 *>(rows + (size_t)inst * max_rows);
  u32 ok = 0, inv = 0;
  for (u32 i = lane; i < n; i += 64) { const u32 t = r[i].z & 3u; ok += t == MSIM_T_OK; inv += t == MSIM_T_INVOKE; }
  ok = c_wave_sum(ok); inv = c_wave_sum(inv);
  if (lane == 0) out[inst] = make_uint2(ok, inv);
}

static void availability_verdict(uint32_t ok, uint32_t inv, uint32_t mode, double a, msim_availability *o) {
  o->ok_count = ok; o->invoke_count = inv;
  o->ok_fraction = inv == 0 ? 1.0f : (float)((double)ok / (double)inv);   // (float (/ ok-count invoke-count)): a ratio rounded once
  o->valid = mode == MSIM_AVAIL_NIL ? 1u : mode == MSIM_AVAIL_TOTAL ? (o->ok_fraction == 1.0f ? 1u : 0u) : (a <= (double)o->ok_fraction ? 1u : 0u);
}

extern "C" int msim_check_availability_rows(const msim_op *rows, uint32_t n_rows, uint32_t mode, double availability, msim_availability *out) {
  if ((!rows && n_rows) || !out || mode > MSIM_AVAIL_FRACTION || (mode == MSIM_AVAIL_FRACTION && !(availability >= 0.0 && availability <= 1.0))) return MSIM_E_INVALID;
  uint32_t ok = 0, inv = 0;
  for (uint32_t i = 0; i < n_rows; i++) { const uint32_t t = MSIM_OP_TYPE(rows[i]); ok += t == MSIM_T_OK; inv += t == MSIM_T_INVOKE; }
  availability_verdict(ok, inv, mode, availability, out);
  return MSIM_OK;
}

extern "C" int msim_check_availability(msim_ctx *ctx, uint32_t mode, double availability, msim_availability *out, uint32_t n_out) {
  if (!ctx || !out) return MSIM_E_INVALID;
  if (!ctx->ran) { ctx->err = "msim_check_availability before msim_run"; return MSIM_E_RANGE; }
  if (mode > MSIM_AVAIL_FRACTION || (mode == MSIM_AVAIL_FRACTION && !(availability >= 0.0 && availability <= 1.0))) {
    ctx->err = "--availability is nil, total, or a number from 0 to 1 (core.clj:149, checker.clj:36-39)"; return MSIM_E_INVALID; }
  if (n_out < ctx->n_inst) { ctx->err = "msim_check_availability: output array shorter than the run"; return MSIM_E_RANGE; }
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)ctx->n_inst * sizeof(uint2);
  uint2 *d = nullptr;
  MSIM_HIP_TRY(ctx, msim_dev_malloc(reinterpret_cast<void **>(&d), bytes));
  hipLaunchKernelGGL(availability_kernel, dim3(ctx->n_inst), dim3(64), 0, ctx->stream, ctx->d_rows, ctx->d_meta, ctx->cfg.max_rows, d);
  std::vector<uint2> h(ctx->n_inst);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)msim_dev_free(d);
  if (e != hipSuccess) { ctx->err = std::string("msim_check_availability: ") + hipGetErrorString(e); return MSIM_E_HIP; }
  for (uint32_t i = 0; i < ctx->n_inst; i++) availability_verdict(h[i].x, h[i].y, mode, availability, &out[i]);
  return MSIM_OK;
}
