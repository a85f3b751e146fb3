// pn_check_dev.hip — the pn-counter / g-counter checker (workload/pn_counter.clj:84-123) on the device, one wavefront per history.
//
// "Every final read is the sum of all known-completed adds plus any number of possibly-completed adds": the acceptable values are
// {sum of :ok adds} + every subset sum of the :info adds' deltas.  pn_check.cpp keeps that set as sorted integer ranges (the
// reference: a Guava TreeRangeSet) on the host after a fetch.  Here it is a BITMAP over [sum + negative deltas, sum + positive
// deltas] — bit b <=> value base + b — one 64-bit word per lane, 4096 values wide: an :info add of delta d is B |= B shifted by d
// (two `ds_bpermute`s per half word), the number of ranges is the number of 0 -> 1 transitions, a final read is one bit test.
// A history whose window is wider than 4096 values or that has more than 1024 indeterminate adds goes to the host checker
// (pn_check.cpp) — same result either way.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "check_run.h"
#include "check_dev.h"

namespace {

constexpr u32 NEEDS_HOST = 3u;
constexpr u32 MAX_INFO = 1024u;

typedef long long s64;

__device__ __forceinline__ s64 p_sum64(s64 v) {
  for (int o = 32; o; o >>= 1) { const u32 lo = (u32)__shfl_xor((int)(u32)v, o), hi = (u32)__shfl_xor((int)(u32)((u64)v >> 32), o); v += (s64)(((u64)hi << 32) | lo); }
  return v;
}
__device__ __forceinline__ u64 p_get64(u64 v, int src_lane) {   // v of lane src_lane (0 outside the wavefront)
  const bool in = src_lane >= 0 && src_lane < 64;
  const int a = (in ? src_lane : 0) << 2;
  const u32 lo = (u32)__builtin_amdgcn_ds_bpermute(a, (int)(u32)v), hi = (u32)__builtin_amdgcn_ds_bpermute(a, (int)(u32)(v >> 32));
  return in ? (((u64)hi << 32) | lo) : 0ull;
}

// what pn_explain_kernel writes beside `out` (msim_explain_pn*; include/maelsim_small_explain.h): pn_check_kernel has an empty one
struct PnExplainOut {
  msim_pn_explain *hdr;   // one per history
  uint4 *records;         // per history: max_records records of 16 bytes, zeroed by the host
  u32 max_records;
};

__global__ void __launch_bounds__(64) pn_check_kernel(const msim_op *rows_all, const msim_inst_meta *meta, msim_check_result *out, u32 max_rows) {
  constexpr bool EXPLAIN = false;
  const PnExplainOut x = PnExplainOut();
#include "pn_body.inc"
}
// The same check with its explanation: the final reads, then the acceptable ranges read off the bitmap without a walk over its 4096 bits.
__global__ void __launch_bounds__(64) pn_explain_kernel(const msim_op *rows_all, const msim_inst_meta *meta, msim_check_result *out, u32 max_rows, const PnExplainOut x) {
  constexpr bool EXPLAIN = true;
#include "pn_body.inc"
}

}  // namespace

// the caller's arrays of an explaining run: a header per history, max_records records of 16 bytes per history
struct PnExplainRun { msim_pn_explain *hdr; void *records; u32 max_records; };
typedef ExplainSlabs<msim_pn_explain, uint4> PnSlabs;

// runs the kernel over n histories in slabs of max_rows rows and lets the host checker finish what the bitmap does not cover
// (xr: pn_explain_kernel in place of pn_check_kernel — every history has an explanation, so it is one launch either way; what the
// bitmap does not cover is explained by the host walk)
static int pn_dev_run(msim_ctx *ctx, const msim_op *d_rows, const msim_inst_meta *d_meta, msim_check_result *d_out, u32 max_rows, u32 n,
                      msim_check_result *h_out, hipStream_t st, u32 *n_host, const PnExplainRun *xr = nullptr) {
  PnSlabs xs;
  if (xr) {
    if (int rc = xs.alloc(ctx, n, xr->max_records, xr->hdr, static_cast<uint4 *>(xr->records))) return rc;
    if (int rc = xs.clear(ctx, st)) return rc;
    const PnExplainOut x{xs.hdr(), xs.rec(), xr->max_records};
    hipLaunchKernelGGL(pn_explain_kernel, dim3(n), dim3(64), 0, st, d_rows, d_meta, d_out, max_rows, x);
  } else hipLaunchKernelGGL(pn_check_kernel, dim3(n), dim3(64), 0, st, d_rows, d_meta, d_out, max_rows);
  MSIM_HIP_TRY(ctx, hipGetLastError());
  MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(msim_check_result), hipMemcpyDeviceToHost, st));
  MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
  if (xr) if (int rc = xs.fetch(ctx, st)) return rc;
  const std::vector<u32> todo = needs(h_out, n, [](u32 valid) { return valid == NEEDS_HOST; });
  if (xr && (msim_dev_flags(ctx) & 0x1000u)) std::fprintf(stderr, "[pn-check] pn_explain_kernel over %u histories, %zu of them for the host\n", n, todo.size());
  if (!todo.empty()) {   // wider than the bitmap: the host checker
    std::vector<msim_inst_meta> hm(n);
    MSIM_HIP_TRY(ctx, hipMemcpy(hm.data(), d_meta, (size_t)n * sizeof(msim_inst_meta), hipMemcpyDeviceToHost));
    const int rc = hand_off(ctx, HistorySource{d_rows, nullptr, &hm, max_rows, 0, nullptr, nullptr}, n, todo, h_out, d_out,
                            [&](const msim_op *rows, u32 nr, const u32 *, u32, u32 flags, u32 i) {
                              if (xr) msim_pn_explain_instance_host(rows, nr, flags, &h_out[i], &xr->hdr[i], static_cast<char *>(xr->records) + (size_t)i * xr->max_records * 16, xr->max_records);
                              else msim_pn_check_instance_host(rows, nr, flags, &h_out[i]);
                            });
    if (rc != MSIM_OK) return rc;
  }
  if (n_host) *n_host = (u32)todo.size();
  return MSIM_OK;
}

// msim_check for pn-counter / g-counter: the histories of the last run, where they lie in HBM (xr: msim_explain_pn's arrays).
static int pn_device(msim_ctx *ctx, const PnExplainRun *xr) {
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::chrono::steady_clock::time_point t0;
  if (int rc = begin_check(ctx, &t0, nullptr)) return rc;   // (no meta here: pn_dev_run fetches it behind the kernel, for the host checker only)
  u32 redone = 0;
  int rc = pn_dev_run(ctx, ctx->d_rows, ctx->d_meta, ctx->d_check, ctx->cfg.max_rows, ctx->n_inst, ctx->h_check, ctx->stream, &redone, xr);
  if (rc != MSIM_OK) return rc;
  finish_check(ctx, t0, redone);
  return MSIM_OK;
}
int msim_check_pn_device(msim_ctx *ctx) { return pn_device(ctx, nullptr); }

// msim_check that also explains.  Towards the context it is msim_check; under developer flag 0x800 the host walk explains.
extern "C" int msim_explain_pn(msim_ctx *ctx, msim_pn_explain *hdr, void *records, uint32_t max_records, uint32_t n_out) {
  if (!ctx || !hdr || (!records && max_records)) return MSIM_E_INVALID;
  const uint32_t wl = ctx->cfg.workload;
  if (int rc = explain_refusal(ctx, "msim_explain_pn", wl == MSIM_WL_PN_COUNTER || wl == MSIM_WL_G_COUNTER, "a pn-counter or g-counter", n_out)) return rc;
  if (msim_dev_flags(ctx) & 0x800u) return msim_explain_pn_host(ctx, hdr, records, max_records);
  const PnExplainRun xr{hdr, records, max_records};
  return pn_device(ctx, &xr);
}

// Checks `n_histories` pn-counter / g-counter histories given on the host, each in a slab of `max_rows` rows (history i at
// rows + i * max_rows, n_rows[i] of them used), with the device checker of msim_check; out[i] as msim_check_pn_rows would fill it.
static int pn_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out, uint32_t *n_host,
                    const PnExplainRun *xr) {
  if (!rows || !n_rows || !out || n_histories == 0 || max_rows == 0) return MSIM_E_INVALID;
  BatchFrame<SlabBatch> f(device);
  if (int rc = f.begin(n_histories, sizeof(msim_check_result), rows, n_rows, max_rows, n_histories)) return rc;
  return pn_dev_run(&f.ctx, f.b.rows.get<msim_op>(), f.b.meta.get<msim_inst_meta>(), f.d_out.get<msim_check_result>(), max_rows, n_histories, out, nullptr, n_host, xr);
}
extern "C" int msim_check_pn_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out) {
  return pn_batch(device, rows, n_rows, max_rows, n_histories, out, nullptr, nullptr);
}
// As msim_check_pn_batch, with pn_explain_kernel's header and records per history (include/maelsim_small_explain.h).
extern "C" int msim_explain_pn_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out,
                                     msim_pn_explain *hdr, void *records, uint32_t max_records, uint32_t *n_host) {
  if (!hdr || (!records && max_records)) return MSIM_E_INVALID;
  const PnExplainRun xr{hdr, records, max_records};
  return pn_batch(device, rows, n_rows, max_rows, n_histories, out, n_host, &xr);
}
