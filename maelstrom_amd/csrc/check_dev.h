// check_dev.h — the device side the device checkers share (txn / rw / kafka / pn / unique / perf _check_dev.hip, cycle_classify.inc),
// the twin of check_run.h: where a history lies, the record of a history not decided yet, the wavefront helpers.  Seen by kernels only.
// The transactional steps stated once are txn_pairing.inc, txn_realtime.inc and txn_kahn.inc; docs/KERNELS.md, "the device side of
// the device checkers".
#ifndef MSIM_CHECK_DEV_H
#define MSIM_CHECK_DEV_H

#include "engine_internal.h"

// The two below are text, not functions: as a function template returning a small struct (and a record returned by value) they
// compiled txn_check_kernel, txn_check_lds_kernel, the classify kernels and pn_check_kernel to other code than they had (the callee is
// simplified on its own before it is inlined: another block order, other registers), text is the same code by construction.

// One history of a launch: declares its rows `r` (16 bytes each) and payload words `pay`, how many of each (n_rows, n_words) and the
// run's `flags`.  p_ is any *Params that names rows / payload / meta / row_off / pay_off / max_rows / max_pay as check_run.h's
// source_of expects them: histories of a run (meta) lie at i * max_rows / i * max_pay, a caller's batch at row_off[i] / pay_off[i].
#define HIST_VIEW(p_, hist_) \
  const uint4 *const r = reinterpret_cast<const uint4 *>((p_).rows) + ((p_).row_off ? (p_).row_off[hist_] : (u64)(hist_) * (p_).max_rows); \
  const u32 *const pay = (p_).payload + ((p_).pay_off ? (p_).pay_off[hist_] : (u64)(hist_) * (p_).max_pay); \
  const u32 n_rows = (p_).meta ? (p_).meta[hist_].n_rows : (u32)((p_).row_off[(hist_) + 1] - (p_).row_off[hist_]); \
  const u32 n_words = (p_).meta ? (p_).meta[hist_].n_payload_words : (u32)((p_).pay_off[(hist_) + 1] - (p_).pay_off[hist_]); \
  [[maybe_unused]] const u32 flags = (p_).meta ? (p_).meta[hist_].flags : 0u

// declares the record res_ with nothing counted yet and `valid` as given (a checker's NEEDS_HOST: what it writes for a history it leaves)
#define BLANK_RESULT(res_, valid_) \
  msim_check_result res_; \
  res_.valid = (valid_); res_.attempt_count = 0; res_.stable_count = 0; res_.lost_count = 0; res_.never_read_count = 0; res_.stale_count = 0; \
  res_.duplicated_count = 0; res_.error_count = 0; \
  for (int i = 0; i < 5; i++) res_.stable_latency_ms[i] = 0; \
  res_.op_count = 0; res_.ok_count = 0; res_.fail_count = 0; res_.info_count = 0

// ---- one wavefront's lanes together (64 lanes; every lane calls) -------------------------------------------------------------------------
__device__ __forceinline__ u32 wv_rl(u32 v, u32 l) { return (u32)__builtin_amdgcn_readlane((int)v, (int)l); }   // v of lane l (l uniform)
__device__ __forceinline__ u32 wv_sum(u32 v) { for (int o = 32; o; o >>= 1) v += (u32)__shfl_xor((int)v, o); return v; }
__device__ __forceinline__ u32 wv_min(u32 v) { for (int o = 32; o; o >>= 1) v = min(v, (u32)__shfl_xor((int)v, o)); return v; }
__device__ __forceinline__ u32 wv_max(u32 v) { for (int o = 32; o; o >>= 1) v = max(v, (u32)__shfl_xor((int)v, o)); return v; }
__device__ __forceinline__ u32 wv_or(u32 v) { for (int o = 32; o; o >>= 1) v |= (u32)__shfl_xor((int)v, o); return v; }
__device__ __forceinline__ u32 wv_excl_scan(u32 v, u32 lane) {   // exclusive prefix sum over the wavefront
  u32 x = v;
  for (int o = 1; o < 64; o <<= 1) { const u32 y = (u32)__shfl_up((int)x, o); if (lane >= (u32)o) x += y; }
  return x - v;
}
// orders the LDS / workspace traffic of ONE wavefront across its lanes (no s_barrier: its memory operations execute in order, the
// compiler must not move them)
__device__ __forceinline__ void wv_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#endif
