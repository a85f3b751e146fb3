// group8.h — device helpers shared by the eight-clusters-per-wavefront kernels (hat8.hip, uid8.hip, crdt8.hip, bcast8.hip, kafka8.hip,
// txn8.hip, mk8.hip, dt8.hip): the latency sampler (latency_sampler.h), the minimum over the lanes of a group.  The round machinery they
// share is in the body fragments group8_*.inc (docs/KERNELS.md §4.10 lists which kernel takes which).
#ifndef MSIM_GROUP8_H
#define MSIM_GROUP8_H
#include "wave_common.h"
#include "latency_sampler.h"

namespace {

// min over the GS (4 or 8) lanes of the caller's group, in every lane of it
template <int GS>
__device__ __forceinline__ u32 g8_min(u32 v) {
  v = min(v, dpp_mov<0xB1, 0xF, 0xF, false>(v, v));   // quad_perm [1,0,3,2]
  v = min(v, dpp_mov<0x4E, 0xF, 0xF, false>(v, v));   // quad_perm [2,3,0,1]
  if (GS == 8) v = min(v, dpp_mov<0x141, 0xF, 0xF, false>(v, v));  // row_half_mirror
  return v;
}

}  // namespace
#endif
