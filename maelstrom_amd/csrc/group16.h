// group16.h — device helpers shared by the four-clusters-per-wavefront kernels (raft4.hip, svc4.hip, txng4.hip, dtg4.hip), whose clusters
// are the 16-lane DPP rows of the wavefront: the latency sampler (latency_sampler.h), the minimum and the prefix sum over a row.  The round
// machinery they share is in the body fragments group16_*.inc (and group8_nemesis.inc).
#ifndef MSIM_GROUP16_H
#define MSIM_GROUP16_H
#include "wave_common.h"
#include "latency_sampler.h"

namespace {

// min over the 16 lanes of the caller's DPP row (= its group), in every lane of the row
__device__ __forceinline__ u32 row_min(u32 v) {
  v = min(v, dpp_mov<0xB1, 0xF, 0xF, false>(v, v));   // quad_perm [1,0,3,2]
  v = min(v, dpp_mov<0x4E, 0xF, 0xF, false>(v, v));   // quad_perm [2,3,0,1]
  v = min(v, dpp_mov<0x141, 0xF, 0xF, false>(v, v));  // row_half_mirror
  v = min(v, dpp_mov<0x140, 0xF, 0xF, false>(v, v));  // row_mirror
  return v;
}
// inclusive prefix sum over the 16 lanes of the row
__device__ __forceinline__ u32 row_scan(u32 v) {
  v += dpp_mov<0x111, 0xF, 0xF, true>(0, v);   // row_shr:1
  v += dpp_mov<0x112, 0xF, 0xF, true>(0, v);   // row_shr:2
  v += dpp_mov<0x114, 0xF, 0xF, true>(0, v);   // row_shr:4
  v += dpp_mov<0x118, 0xF, 0xF, true>(0, v);   // row_shr:8
  return v;
}

}  // namespace
#endif
