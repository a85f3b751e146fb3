// latency_sampler.h — the exponential latency sampler of the device code (the sampler of engine.hip / the oracle), for every kernel but
// duo.hip (which keeps its table in LDS).  The Q24 log2 table has one copy per translation unit; the unit's launcher uploads it before its
// first launch on a device: MSIM_UPLOAD_ONCE(d_log2_q24, msim_log2_q24, sizeof(msim_log2_q24)).
#ifndef MSIM_LATENCY_SAMPLER_H
#define MSIM_LATENCY_SAMPLER_H
#include <hip/hip_runtime.h>

#include "wave_common.h"
#include "log2_table.h"

static __constant__ u32 d_log2_q24[257];

// -ln(u), u = (r+1)/2^32, Q16, integer only
__device__ __forceinline__ u32 neg_ln_q16(u32 r) {
  if (r == 0xFFFFFFFFu) return 0;
  const u32 v = r + 1;
  const u32 e = 31 - __clz(v);
  const u32 m = v << (31 - e);
  const u32 idx = (m >> 23) & 0xFF;
  const u32 f = (m >> 7) & 0xFFFF;
  const u32 l0 = d_log2_q24[idx], l1 = d_log2_q24[idx + 1];
  const u32 lg = (e << 24) + l0 + (u32)(((u64)(l1 - l0) * f) >> 16);
  const u32 d = (32u << 24) - lg;
  return (u32)(((u64)d * 2977044472ull) >> 40);
}

#endif
