// unique_check_dev.hip — [upstream] jepsen.checker/unique-ids (workload/unique_ids.clj:67) on the device, one wavefront per history:
// :attempted-count = :invoke :generate ops, :acknowledged-count = :ok ones, :duplicated = values acknowledged more than once,
// :range = [min max]; valid iff nothing is duplicated.  pn_check.cpp sorts the acknowledged ids on the host after a fetch; here the
// rows are streamed once (1 KiB per load), every :ok id goes into an open-addressing table in HBM workspace (compare-and-swap on
// the key word, an atomic count beside it), and the duplicated values are the table slots counted twice or more.  Complete: no
// host pass behind it.  Histories whose ids fit a table in LDS (up to 19660 acknowledged ids: every bench shape) take
// unique_check_lds_kernel instead — a workgroup of 1024 threads (round 6; 256 before) per history, 32768 id slots and a "seen again" bitmap in 132 KiB of LDS:
// the HBM tables cost 256 KiB of initialisation and scattered compare-and-swaps per history (25 ms per 16384 histories of the demo shape).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "check_run.h"
#include "check_dev.h"

namespace {

constexpr u32 EMPTY = 0xFFFFFFFFu;

struct UParams {
  const msim_op *rows; const msim_inst_meta *meta; msim_check_result *out;
  uint2 *ws;             // table_slots {id, count} per history of the launch
  u32 max_rows, table_slots /* power of two >= 2 x the ids of a history */, first;
};

__global__ void __launch_bounds__(64) unique_check_kernel(const UParams p) {
  const u32 lane = threadIdx.x, hist = p.first + blockIdx.x;
  const uint4 *const r = reinterpret_cast<const uint4 *>(p.rows) + (u64)hist * p.max_rows;
  const u32 n = p.meta[hist].n_rows, flags = p.meta[hist].flags;
  uint2 *const tab = p.ws + (u64)blockIdx.x * p.table_slots;
  const u32 mask = p.table_slots - 1u;
  for (u32 i = lane; i < p.table_slots; i += 64) tab[i] = make_uint2(EMPTY, 0u);
  __syncthreads();

  u32 c_inv = 0, c_ok = 0, c_fail = 0, c_info = 0, c_att = 0, lo = EMPTY, hi = 0, n_empty_id = 0, n_ids = 0;
  for (u32 base = 0; base < n; base += 64) {
    const u32 idx = base + lane;
    if (idx >= n) continue;
    const uint4 row = r[idx];
    const u32 type = row.z & 3u, f = (row.z >> 2) & 31u, proc = row.z >> 12;
    if (proc == MSIM_PROCESS_NEMESIS) continue;
    c_inv += type == MSIM_T_INVOKE; c_ok += type == MSIM_T_OK; c_fail += type == MSIM_T_FAIL; c_info += type == MSIM_T_INFO;
    if (f != MSIM_F_GENERATE) continue;
    c_att += type == MSIM_T_INVOKE;
    if (type != MSIM_T_OK) continue;
    const u32 id = row.w;
    lo = min(lo, id); hi = max(hi, id); n_ids++;
    if (id == EMPTY) { n_empty_id++; continue; }   // (the one value the table cannot hold is counted apart)
    u32 h = (id * 0x9E3779B1u) >> 7;
    for (;;) {
      h &= mask;
      const u32 old = atomicCAS(&tab[h].x, EMPTY, id);
      if (old == EMPTY || old == id) { atomicAdd(&tab[h].y, 1u); break; }
      h++;
    }
  }
  __syncthreads();
  u32 dups = 0;
  for (u32 i = lane; i < p.table_slots; i += 64) dups += tab[i].y >= 2u ? 1u : 0u;
  dups = wv_sum(dups); n_empty_id = wv_sum(n_empty_id); n_ids = wv_sum(n_ids);
  if (n_empty_id >= 2) dups++;
  c_inv = wv_sum(c_inv); c_ok = wv_sum(c_ok); c_fail = wv_sum(c_fail); c_info = wv_sum(c_info); c_att = wv_sum(c_att);
  lo = wv_min(lo); hi = wv_max(hi);
  if (lane == 0) {
    msim_check_result o;
    o.valid = flags ? 0u : (dups == 0 ? 1u : 0u);
    o.attempt_count = c_att; o.stable_count = 0; o.lost_count = 0; o.never_read_count = 0; o.stale_count = 0; o.duplicated_count = dups; o.error_count = 0;
    for (int i = 0; i < 5; i++) o.stable_latency_ms[i] = 0;
    if (n_ids) { o.stable_latency_ms[0] = lo; o.stable_latency_ms[1] = hi; }   // :range
    o.op_count = c_inv; o.ok_count = c_ok; o.fail_count = c_fail; o.info_count = c_info;
    p.out[hist] = o;
  }
}

#ifndef UNIQ_WG   // threads per history: the table's 132 KiB leave a CU one workgroup, so the workgroup is what hides the rows' way from HBM (round 6: 256 -> 1024, four wavefronts per SIMD)
#define UNIQ_WG 1024
#endif
constexpr u32 LDS_SLOTS = 32768u;   // ids a workgroup's table holds (power of two); + LDS_SLOTS / 32 words of "seen again" bits

// the same check with the table in LDS: one workgroup per history
__global__ void __launch_bounds__(UNIQ_WG) unique_check_lds_kernel(const UParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32 *const tab = reinterpret_cast<u32 *>(smem);            // [LDS_SLOTS] id (EMPTY: free)
  u32 *const again = tab + LDS_SLOTS;                        // [LDS_SLOTS / 32] the slot's id was acknowledged more than once
  u32 *const hdr = again + LDS_SLOTS / 32;                   // [16] counters
  const u32 tid = threadIdx.x, hist = p.first + blockIdx.x;
  const uint4 *const r = reinterpret_cast<const uint4 *>(p.rows) + (u64)hist * p.max_rows;
  const u32 n = p.meta[hist].n_rows, flags = p.meta[hist].flags;
  for (u32 i = tid; i < LDS_SLOTS; i += UNIQ_WG) tab[i] = EMPTY;
  for (u32 i = tid; i < LDS_SLOTS / 32 + 16; i += UNIQ_WG) again[i] = 0;
  __syncthreads();
  if (tid == 0) hdr[8] = EMPTY;   // (the minimum; the loop above zeroed the counters)
  __syncthreads();

  u32 c_inv = 0, c_ok = 0, c_fail = 0, c_info = 0, c_att = 0, lo = EMPTY, hi = 0, n_empty_id = 0, n_ids = 0;
  for (u32 idx = tid; idx < n; idx += UNIQ_WG) {
    const uint4 row = r[idx];
    const u32 type = row.z & 3u, f = (row.z >> 2) & 31u, proc = row.z >> 12;
    if (proc == MSIM_PROCESS_NEMESIS) continue;
    c_inv += type == MSIM_T_INVOKE; c_ok += type == MSIM_T_OK; c_fail += type == MSIM_T_FAIL; c_info += type == MSIM_T_INFO;
    if (f != MSIM_F_GENERATE) continue;
    c_att += type == MSIM_T_INVOKE;
    if (type != MSIM_T_OK) continue;
    const u32 id = row.w;
    lo = min(lo, id); hi = max(hi, id); n_ids++;
    if (id == EMPTY) { n_empty_id++; continue; }   // (the one value the table cannot hold is counted apart)
    u32 h = (id * 0x9E3779B1u) >> 7;
    // (the host only takes this kernel when every row of the history could be an acknowledged id and the table still stays below a
    //  load factor of 0.6; the probe count is bounded all the same: a full table must end in a verdict, not in a hung GPU)
    u32 probes = 0;
    for (; probes < LDS_SLOTS; probes++) {
      h &= LDS_SLOTS - 1u;
      const u32 old = atomicCAS(&tab[h], EMPTY, id);
      if (old == EMPTY) break;
      if (old == id) { atomicOr(&again[h >> 5], 1u << (h & 31u)); break; }
      h++;
    }
    if (probes == LDS_SLOTS) atomicOr(&hdr[10], 1u);   // table full
  }
  atomicAdd(&hdr[0], c_inv); atomicAdd(&hdr[1], c_ok); atomicAdd(&hdr[2], c_fail); atomicAdd(&hdr[3], c_info); atomicAdd(&hdr[4], c_att);
  atomicAdd(&hdr[5], n_empty_id); atomicAdd(&hdr[6], n_ids); atomicMin(&hdr[8], lo); atomicMax(&hdr[9], hi);
  __syncthreads();
  u32 dups = 0;
  for (u32 i = tid; i < LDS_SLOTS / 32; i += UNIQ_WG) dups += (u32)__popc(again[i]);
  atomicAdd(&hdr[7], dups);
  __syncthreads();
  if (tid == 0) {
    u32 d = hdr[7];
    if (hdr[5] >= 2) d++;
    msim_check_result o;
    o.valid = (flags || hdr[10]) ? 0u : (d == 0 ? 1u : 0u);
    o.attempt_count = hdr[4]; o.stable_count = 0; o.lost_count = 0; o.never_read_count = 0; o.stale_count = 0; o.duplicated_count = d; o.error_count = hdr[10];
    for (int i = 0; i < 5; i++) o.stable_latency_ms[i] = 0;
    if (hdr[6]) { o.stable_latency_ms[0] = hdr[8]; o.stable_latency_ms[1] = hdr[9]; }   // :range
    o.op_count = hdr[0]; o.ok_count = hdr[1]; o.fail_count = hdr[2]; o.info_count = hdr[3];
    p.out[hist] = o;
  }
}

// ---- the explanation (msim_explain_unique*; include/maelsim_small_explain.h): the duplicated ids, how often, the first two rows ----
// One workgroup per history that has a duplicate (`list`), the id table in LDS or — the histories unique_check_kernel takes — in HBM
// workspace.  The table is filled as above; the slots seen again are gathered into a list in LDS (any order) and sorted by id, so that
// a second sweep over the rows finds an acknowledgement's entry by bisection: it counts, and keeps the smallest row (atomicMin).  A
// third sweep keeps the smallest row that is not the first — two ordered passes, nothing depends on which lane came first.  Then the
// list is sorted by (count descending, id descending) and written as far as the caller's slab goes.
constexpr u32 XD_MAX = MSIM_UNIQUE_EXPLAIN_MAX_DUPS;   // duplicated ids the list in LDS holds: a history with more is the host walk's

struct UXOut {
  msim_unique_explain *hdr; msim_unique_dup *dups; u32 max_dups;
  u32 *ws;   // HBM route: table_slots id words + table_slots / 32 words of "seen again" bits per history of the launch
};

template <bool BY_ID> __device__ __forceinline__ bool dup_before(const uint4 a, const uint4 b) {
  if (BY_ID) return a.x != b.x ? a.x < b.x : a.y < b.y;   // (a padding entry {EMPTY, EMPTY, ..} behind the id EMPTY itself, whose count is still 0)
  return a.y != b.y ? a.y > b.y : a.x > b.x;
}
// bitonic network over n2 (a power of two) entries of `dl`, by the whole workgroup
template <bool BY_ID> __device__ __forceinline__ void dup_sort(uint4 *dl, u32 n2, u32 tid) {
  for (u32 k = 2; k <= n2; k <<= 1)
    for (u32 j = k >> 1; j; j >>= 1) {
      for (u32 i = tid; i < n2; i += UNIQ_WG) {
        const u32 l = i ^ j;
        if (l > i) {
          const uint4 a = dl[i], b = dl[l];
          if (dup_before<BY_ID>(b, a) == ((i & k) == 0)) { dl[i] = b; dl[l] = a; }
        }
      }
      __syncthreads();
    }
}
// the entry of `id` among the n_d entries sorted by id (n_d: none)
__device__ __forceinline__ u32 dup_find(const uint4 *dl, u32 n_d, u32 id) {
  u32 lo = 0, hi = n_d;
  while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (dl[mid].x < id) lo = mid + 1; else hi = mid; }
  return lo < n_d && dl[lo].x == id ? lo : n_d;
}

template <bool LDS_TABLE> __device__ __forceinline__ void unique_explain_body(const UParams &p, const u32 *list, const UXOut &x, unsigned char *smem) {
  uint4 *const dl = reinterpret_cast<uint4 *>(smem);   // [XD_MAX] {id, count, first row, second row}
  u32 *const dw = reinterpret_cast<u32 *>(smem);
  u32 *const hd = dw + 4u * XD_MAX;                    // [4] entries listed, acknowledgements of the id EMPTY
  const u32 slots = LDS_TABLE ? LDS_SLOTS : p.table_slots;
  u32 *const tab = LDS_TABLE ? hd + 4 : x.ws + (u64)blockIdx.x * (p.table_slots + p.table_slots / 32u);
  u32 *const again = tab + slots;
  const u32 tid = threadIdx.x, hist = list[p.first + blockIdx.x];
  const uint4 *const r = reinterpret_cast<const uint4 *>(p.rows) + (u64)hist * p.max_rows;
  const u32 n = p.meta[hist].n_rows;
  for (u32 i = tid; i < slots; i += UNIQ_WG) tab[i] = EMPTY;
  for (u32 i = tid; i < slots / 32u; i += UNIQ_WG) again[i] = 0;
  if (tid < 4) hd[tid] = 0;
  __syncthreads();
  // the acknowledged id of row idx (false: the row acknowledges none)
  auto ack = [&](u32 idx, u32 *id) {
    const uint4 row = r[idx];
    *id = row.w;
    return (row.z >> 12) != MSIM_PROCESS_NEMESIS && ((row.z >> 2) & 31u) == MSIM_F_GENERATE && (row.z & 3u) == MSIM_T_OK;
  };
  for (u32 idx = tid; idx < n; idx += UNIQ_WG) {
    u32 id;
    if (!ack(idx, &id)) continue;
    if (id == EMPTY) { atomicAdd(&hd[1], 1u); continue; }   // (the one value the table cannot hold is counted apart)
    u32 h = (id * 0x9E3779B1u) >> 7;
    for (u32 probes = 0; probes < slots; probes++, h++) {   // (the host sizes the table for a load factor of 0.6 at most; bounded all the same)
      h &= slots - 1u;
      const u32 old = atomicCAS(&tab[h], EMPTY, id);
      if (old == EMPTY) break;
      if (old == id) { atomicOr(&again[h >> 5], 1u << (h & 31u)); break; }
    }
  }
  __syncthreads();
  for (u32 i = tid; i < slots / 32u; i += UNIQ_WG)
    for (u32 w = again[i]; w; w &= w - 1u) {
      const u32 k = atomicAdd(&hd[0], 1u);
      if (k < XD_MAX) dl[k] = make_uint4(tab[i * 32u + (u32)__builtin_ctz(w)], 0u, EMPTY, EMPTY);
    }
  __syncthreads();
  if (tid == 0 && hd[1] >= 2u) { const u32 k = hd[0]; if (k < XD_MAX) dl[k] = make_uint4(EMPTY, 0u, EMPTY, EMPTY); hd[0] = k + 1u; }
  __syncthreads();
  const u32 n_d = hd[0];
  // n_d is what the check's kernels wrote as duplicated_count (the same table, the id EMPTY counted apart alike), and the host hands a
  // history with more than XD_MAX of them to its walk without listing it here.  Should the two ever disagree, the header says so: no
  // record, `truncated` set — never a zero header that reads as "no duplicate".
  if (n_d > XD_MAX) { if (tid == 0) { x.hdr[hist].n_dups = 0; x.hdr[hist].truncated = 1u; } return; }
  u32 n2 = 1;
  while (n2 < n_d) n2 <<= 1;
  for (u32 i = n_d + tid; i < n2; i += UNIQ_WG) dl[i] = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
  __syncthreads();
  dup_sort<true>(dl, n2, tid);
  for (u32 idx = tid; idx < n; idx += UNIQ_WG) {
    u32 id;
    if (!ack(idx, &id)) continue;
    const u32 d = dup_find(dl, n_d, id);
    if (d < n_d) { atomicAdd(&dw[4u * d + 1u], 1u); atomicMin(&dw[4u * d + 2u], idx); }
  }
  __syncthreads();
  for (u32 idx = tid; idx < n; idx += UNIQ_WG) {
    u32 id;
    if (!ack(idx, &id)) continue;
    const u32 d = dup_find(dl, n_d, id);
    if (d < n_d && idx != dw[4u * d + 2u]) atomicMin(&dw[4u * d + 3u], idx);
  }
  __syncthreads();
  for (u32 i = n_d + tid; i < n2; i += UNIQ_WG) dl[i] = make_uint4(0u, 0u, 0u, 0u);   // (count 0: behind every entry in the order of the output)
  __syncthreads();
  dup_sort<false>(dl, n2, tid);
  const u32 n_out = min(n_d, x.max_dups);
  uint4 *const dst = reinterpret_cast<uint4 *>(x.dups + (size_t)hist * x.max_dups);
  for (u32 i = tid; i < n_out; i += UNIQ_WG) dst[i] = dl[i];
  if (tid == 0) { x.hdr[hist].n_dups = n_out; x.hdr[hist].truncated = n_d > x.max_dups ? 1u : 0u; }
}

__global__ void __launch_bounds__(UNIQ_WG) unique_explain_lds_kernel(const UParams p, const u32 *list, const UXOut x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unique_explain_body<true>(p, list, x, smem);
}
__global__ void __launch_bounds__(UNIQ_WG) unique_explain_kernel(const UParams p, const u32 *list, const UXOut x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unique_explain_body<false>(p, list, x, smem);
}

}  // namespace

// `paired`: the histories are the engine's own — every :ok row follows its :invoke row, so at most max_rows / 2 ids are acknowledged;
// rows handed in by a caller (msim_check_unique_batch) may be ALL acknowledgements (a history filtered to its completions).
static int unique_dev_run(msim_ctx *ctx, UParams up, u32 n, void **ws, size_t *ws_cap, hipStream_t st, bool paired) {
  // a load factor of 0.6 keeps the LDS table's probe sequences short (and the table can never fill up)
  const uint64_t max_ids = paired ? up.max_rows / 2 : up.max_rows;
  if (max_ids * 10 <= (uint64_t)LDS_SLOTS * 6 && !(msim_dev_flags(ctx) & 0x2000u)) {   // (MSIM_DEV_FLAGS bit 13: the HBM tables)
    const size_t lds = ((size_t)LDS_SLOTS + LDS_SLOTS / 32 + 16) * 4;
    MSIM_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&unique_check_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    up.first = 0;
    hipLaunchKernelGGL(unique_check_lds_kernel, dim3(n), dim3(UNIQ_WG), lds, st, up);
    MSIM_HIP_TRY(ctx, hipGetLastError());
    return MSIM_OK;
  }
  u32 slots = 64; while (slots < (paired ? up.max_rows : 2 * up.max_rows)) slots <<= 1;   // >= 2 x the ids a history can acknowledge
  up.table_slots = slots;
  const u32 chunk = chunk_for(n, (uint64_t)slots * 8, 4ull << 30, msim_dev_flags(ctx));
  if (int rc = grow_ws(ctx, ws, ws_cap, (size_t)chunk * slots * 8)) return rc;
  up.ws = static_cast<uint2 *>(*ws);
  hipError_t e;
  const u32 launches = for_chunks(n, chunk, &e, [&](u32 first, u32 count) {
    up.first = first;
    hipLaunchKernelGGL(unique_check_kernel, dim3(count), dim3(64), 0, st, up);
  });
  MSIM_HIP_TRY(ctx, e);
  if (msim_dev_flags(ctx) & 0x1000u) std::fprintf(stderr, "[unique-check] HBM tables (%u slots) over %u histories (%u launches)\n", slots, n, launches);   // developer trace bit
  return MSIM_OK;
}

// the caller's arrays of an explaining run: a header per history, max_dups records per history
struct UniqueExplainRun { msim_unique_explain *hdr; msim_unique_dup *dups; u32 max_dups; };

// Behind unique_dev_run (whose records lie in up.out): the histories with a duplicate are explained by unique_explain_*_kernel, those
// with more than XD_MAX duplicated ids by the host walk (*n_host).  Without such a history nothing is launched and nothing allocated.
static int unique_explain_run(msim_ctx *ctx, UParams up, u32 n, void **ws, size_t *ws_cap, hipStream_t st, bool paired, msim_check_result *h_out,
                              const UniqueExplainRun &xr, u32 *n_host) {
  MSIM_HIP_TRY(ctx, hipMemcpyAsync(h_out, up.out, (size_t)n * sizeof(msim_check_result), hipMemcpyDeviceToHost, st));
  MSIM_HIP_TRY(ctx, hipStreamSynchronize(st));
  std::memset(xr.hdr, 0, (size_t)n * sizeof(msim_unique_explain));
  if (xr.max_dups) std::memset(xr.dups, 0, (size_t)n * xr.max_dups * sizeof(msim_unique_dup));
  std::vector<u32> list, todo;
  for (u32 i = 0; i < n; i++) if (h_out[i].duplicated_count) (h_out[i].duplicated_count > XD_MAX ? todo : list).push_back(i);
  if (n_host) *n_host = (u32)todo.size();
  if (!list.empty()) {
    const u32 m = (u32)list.size();
    ExplainSlabs<msim_unique_explain, msim_unique_dup> xs;   // (on the device only now that some history has a duplicate)
    DevBuf d_list;
    if (int rc = xs.alloc(ctx, n, xr.max_dups, xr.hdr, xr.dups)) return rc;
    if (int rc = xs.clear(ctx, st)) return rc;
    MSIM_HIP_TRY(ctx, d_list.upload(list.data(), (size_t)m * 4));
    const u32 *const dl = d_list.get<u32>();
    UXOut x{xs.hdr(), xs.rec(), xr.max_dups, nullptr};
    const uint64_t max_ids = paired ? up.max_rows / 2 : up.max_rows;
    const bool lds_route = max_ids * 10 <= (uint64_t)LDS_SLOTS * 6 && !(msim_dev_flags(ctx) & 0x2000u);   // (as unique_dev_run chooses)
    const size_t list_lds = (size_t)XD_MAX * 16 + 16;
    if (lds_route) {
      const size_t lds = list_lds + ((size_t)LDS_SLOTS + LDS_SLOTS / 32) * 4;
      MSIM_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&unique_explain_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      up.first = 0;
      hipLaunchKernelGGL(unique_explain_lds_kernel, dim3(m), dim3(UNIQ_WG), lds, st, up, dl, x);
      MSIM_HIP_TRY(ctx, hipGetLastError());
    } else {
      u32 slots = 64; while (slots < (paired ? up.max_rows : 2 * up.max_rows)) slots <<= 1;
      up.table_slots = slots;
      const uint64_t per = (uint64_t)slots * 4 + slots / 8;
      const u32 chunk = chunk_for(m, per, 4ull << 30, msim_dev_flags(ctx));
      if (int rc = grow_ws(ctx, ws, ws_cap, (size_t)chunk * per)) return rc;
      x.ws = static_cast<u32 *>(*ws);
      hipError_t e;
      for_chunks(m, chunk, &e, [&](u32 first, u32 count) {   // (one workspace: the chunks follow one another on the stream)
        up.first = first;
        hipLaunchKernelGGL(unique_explain_kernel, dim3(count), dim3(UNIQ_WG), list_lds, st, up, dl, x);
      });
      MSIM_HIP_TRY(ctx, e);
    }
    if (msim_dev_flags(ctx) & 0x1000u) std::fprintf(stderr, "[unique-check] unique_explain_kernel (%s table) over %u of %u histories\n", lds_route ? "LDS" : "HBM", m, n);
    if (int rc = xs.fetch(ctx, st)) return rc;   // (waits: the buffers are freed with this block)
  }
  if (!todo.empty()) {
    std::vector<msim_inst_meta> hm(n);
    MSIM_HIP_TRY(ctx, hipMemcpy(hm.data(), up.meta, (size_t)n * sizeof(msim_inst_meta), hipMemcpyDeviceToHost));
    const int rc = hand_off(ctx, HistorySource{up.rows, nullptr, &hm, up.max_rows, 0, nullptr, nullptr}, n, todo, h_out, up.out,
                            [&](const msim_op *rows, u32 nr, const u32 *, u32, u32 flags, u32 i) {
                              msim_unique_explain_instance_host(rows, nr, flags, &h_out[i], &xr.hdr[i], xr.dups + (size_t)i * xr.max_dups, xr.max_dups);
                            });
    if (rc != MSIM_OK) return rc;
  }
  return MSIM_OK;
}

// msim_check that also explains.  Towards the context it is msim_check (msim_check_host_rechecks: the histories of more than
// MSIM_UNIQUE_EXPLAIN_MAX_DUPS duplicated ids, whose records the host walk wrote again); under developer flag 0x800 the host walk explains.
extern "C" int msim_explain_unique(msim_ctx *ctx, msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups, uint32_t n_out) {
  if (!ctx || !hdr || (!dups && max_dups)) return MSIM_E_INVALID;
  if (int rc = explain_refusal(ctx, "msim_explain_unique", ctx->cfg.workload == MSIM_WL_UNIQUE_IDS, "a unique-ids", n_out)) return rc;
  if (msim_dev_flags(ctx) & 0x800u) return msim_explain_unique_host(ctx, hdr, dups, max_dups);
  // msim_check's own route for this workload (engine.hip workload_check): it leaves check_fetched false, so msim_check_results reads
  // d_check — which hand_off refreshes below — and no pinned copy of the records goes stale
  if (int rc = msim_check_unique_device(ctx)) return rc;
  UParams up;
  std::memset(&up, 0, sizeof up);
  up.rows = ctx->d_rows; up.meta = ctx->d_meta; up.out = ctx->d_check; up.max_rows = ctx->cfg.max_rows;
  std::vector<msim_check_result> h_out(ctx->n_inst);
  u32 redone = 0;
  if (int rc = unique_explain_run(ctx, up, ctx->n_inst, &ctx->d_check_scratch, &ctx->cap_check_scratch, ctx->stream, true, h_out.data(), UniqueExplainRun{hdr, dups, max_dups}, &redone)) return rc;
  ctx->lin_host_rechecks = redone;
  return MSIM_OK;
}

// msim_check for unique-ids: the histories of the last run, where they lie in HBM.
int msim_check_unique_device(msim_ctx *ctx) {
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  UParams up;
  std::memset(&up, 0, sizeof up);
  up.rows = ctx->d_rows; up.meta = ctx->d_meta; up.out = ctx->d_check; up.max_rows = ctx->cfg.max_rows;
  MSIM_HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  int rc = unique_dev_run(ctx, up, ctx->n_inst, &ctx->d_check_scratch, &ctx->cap_check_scratch, ctx->stream, true);
  if (rc != MSIM_OK) return rc;
  MSIM_HIP_TRY(ctx, hipEventRecord(ctx->ev3, ctx->stream));
  MSIM_HIP_TRY(ctx, hipEventSynchronize(ctx->ev3));
  MSIM_HIP_TRY(ctx, hipEventElapsedTime(&ctx->check_ms, ctx->ev2, ctx->ev3));
  ctx->checked = true; ctx->check_fetched = false;
  return MSIM_OK;
}

// Checks `n_histories` unique-ids histories given on the host, each in a slab of `max_rows` rows (history i at rows + i * max_rows,
// n_rows[i] of them used), with the device checker of msim_check; out[i] as msim_check_unique_rows would fill it.
// (xr: msim_explain_unique_batch's arrays)
static int unique_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out, const UniqueExplainRun *xr,
                        uint32_t *n_host) {
  if (!rows || !n_rows || !out || n_histories == 0 || max_rows == 0) return MSIM_E_INVALID;
  BatchFrame<SlabBatch> f(device); msim_ctx *ctx = &f.ctx;
  if (int rc = f.begin(n_histories, sizeof(msim_check_result), rows, n_rows, max_rows, n_histories)) return rc;
  DevBuf ws; size_t ws_cap = 0;
  UParams up;
  std::memset(&up, 0, sizeof up);
  up.rows = f.b.rows.get<msim_op>(); up.meta = f.b.meta.get<msim_inst_meta>(); up.out = f.d_out.get<msim_check_result>(); up.max_rows = max_rows;
  if (int rc = unique_dev_run(ctx, up, n_histories, ws.addr(), &ws_cap, nullptr, false)) return rc;
  if (xr) return unique_explain_run(ctx, up, n_histories, ws.addr(), &ws_cap, nullptr, false, out, *xr, n_host);
  MSIM_HIP_TRY(ctx, hipMemcpy(out, up.out, (size_t)n_histories * sizeof(msim_check_result), hipMemcpyDeviceToHost));
  return MSIM_OK;
}
extern "C" int msim_check_unique_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out) {
  return unique_batch(device, rows, n_rows, max_rows, n_histories, out, nullptr, nullptr);
}
// As msim_check_unique_batch, with the duplicated ids of every history that has one (include/maelsim_small_explain.h).
extern "C" int msim_explain_unique_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out,
                                         msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups, uint32_t *n_host) {
  if (!hdr || (!dups && max_dups)) return MSIM_E_INVALID;
  const UniqueExplainRun xr{hdr, dups, max_dups};
  return unique_batch(device, rows, n_rows, max_rows, n_histories, out, &xr, n_host);
}
