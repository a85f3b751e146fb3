// k_general_d.hip - instantiates sim_kernel<> (general layout) for batched gossip (demo/python/broadcast.py).
// The colocated kernel has no arm for it: every concurrency runs the general layout.
#include "sim_kernels.h"

template <bool NEM, bool NET_RANDOM>
static hipError_t launch_batch(const KParams &kp, uint32_t n, size_t lds, hipStream_t st) {
  const void *fn = reinterpret_cast<const void *>(&sim_kernel<MSIM_NODE_BCAST_BATCH, NEM, NET_RANDOM>);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((sim_kernel<MSIM_NODE_BCAST_BATCH, NEM, NET_RANDOM>), dim3(n), dim3(64), lds, st, kp);
  return hipGetLastError();
}

hipError_t msim_launch_general_d(const KParams &kp, uint32_t n, size_t lds, hipStream_t st) {
  hipError_t e = msim_upload_tables();
  if (e != hipSuccess) return e;
  if (kp.cfg.node_program != MSIM_NODE_BCAST_BATCH) return MSIM_LAYOUT_DOES_NOT_FIT;
  const bool rnd = kp.cfg.latency_dist != MSIM_LAT_CONSTANT || kp.cfg.p_loss_q32 != 0;
  if (kp.cfg.nemesis_mask) return rnd ? launch_batch<true, true>(kp, n, lds, st) : launch_batch<true, false>(kp, n, lds, st);
  return rnd ? launch_batch<false, true>(kp, n, lds, st) : launch_batch<false, false>(kp, n, lds, st);
}
