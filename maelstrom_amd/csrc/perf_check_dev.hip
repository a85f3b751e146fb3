// perf_check_dev.hip — [upstream] jepsen.checker/stats with its :by-f map (as jepsen.kafka/stats-checker wraps it, core.clj:96-97) and the
// numbers behind jepsen.checker/perf's latency plots (core.clj:92) on the device: per history and per (:f, completion type) the counts and
// the latency quantiles, over the whole history and per time window.  The contract is the comment above msim_check_perf in
// include/maelsim.h (upstream jepsen.checker is not vendored: parity with its plots is unpinned).
//
// One WAVEFRONT per history (perf_check_kernel).  A completion pairs with the previous row of its worker thread, so the rows have to be
// taken in order; inside a wavefront 64 rows are taken at once — the lanes of a chunk find their predecessors through a lane mask per
// worker thread in LDS, the last row of every thread stays behind in a table for the chunks that follow — and no barrier is ever waited
// for, which a workgroup of several wavefronts would need after every chunk.  The histories users run are a few thousand rows; the
// ensemble (thousands of histories per launch) is what fills the machine, as for check_kernel and availability_kernel.
//   pass 1  the rows once from HBM, 16 bytes per lane and 1 KiB per load, the next chunk in flight; the payload is never touched.  Every
//           completion counts in cnt[f][type] (LDS atomics); a paired one leaves {latency_us, group} at its rank in an HBM record area
//           (8 B per op against the 32 B of its two rows) and counts in the group histogram.  group = (f * 3 + type - 1) * W + window.
//   sort    exclusive prefix sums over the histogram, then the records are scattered by group into LDS: 4 B per paired op, at most
//           32767 ops (max_rows < 65535) = 128 KiB, which with the tables stays inside the CU's 160 KiB for every history the device
//           checkers accept — there is no second path and no host fallback.  The windows of one (f, type) are neighbours, so the
//           whole-history group is one contiguous span of the same array.
//   select  per record the span's minimum, maximum and sum, and the quantiles .5 .95 .99 by bisection on the value between them
//           (the rule of check_kernel's stable latencies).  Spans of more than SERIAL_MAX latencies are taken by the whole wavefront one
//           after the other, the many short ones (the windows) one per lane at the same time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "check_run.h"
#include "check_dev.h"

namespace {

constexpr u32 NF = 32;            // the :f field has five bits
constexpr u32 NT = 3;             // completion types: ok, fail, info
constexpr u32 SERIAL_MAX = 128;   // spans up to this length are selected by one lane
constexpr u32 SLOTS = MSIM_PERF_MAX_F * NT;   // latency records per history (and per window)

struct PParams {
  const msim_op *rows; const msim_inst_meta *meta;
  msim_perf_result *out; msim_latency_dist *win;   // win: null when W == 0
  uint2 *recs;                                       // per history: cap records {latency_us, group}
  u64 window_ns;
  u32 max_rows, C, W /* 0 = no windows */, cap /* paired ops a history can have: max_rows / 2 */;
  u32 off_hist, off_end, off_cnt, off_unp, off_lm, off_tbl;   // LDS offsets in words; the sorted latencies lie at 0
};

__device__ __forceinline__ u32 p_kth_bit(u32 mask, u32 k) { for (; k; k--) mask &= mask - 1; return (u32)__ffs((int)mask) - 1u; }

// count, sum and the five quantiles of the latencies s[a .. b): by the 64 lanes together (WAVE: every lane calls, lane 0 writes) or by the
// calling lane alone
template <bool WAVE>
__device__ __forceinline__ void p_select(const u32 *s, u32 a, u32 b, u32 lane, msim_latency_dist *dst) {
  const u32 n = b - a, first = WAVE ? a + lane : a, step = WAVE ? 64u : 1u;
  u32 mn = 0xFFFFFFFFu, mx = 0; u64 sum = 0;
  for (u32 e = first; e < b; e += step) { const u32 v = s[e]; mn = min(mn, v); mx = max(mx, v); sum += v; }
  if (WAVE) {
    mn = wv_min(mn); mx = wv_max(mx);
    const u32 lo = wv_sum((u32)sum & 0xFFFFu), mid = wv_sum(((u32)sum >> 16) & 0xFFFFu);   // (64 x 16 bits fit a word)
    const u32 hi = wv_sum((u32)(sum >> 32) & 0xFFFFu), top = wv_sum((u32)(sum >> 48));
    sum = (u64)lo + ((u64)mid << 16) + ((u64)hi << 32) + ((u64)top << 48);
  }
  msim_latency_dist o;
  o.count = n; o.sum_us = n ? sum : 0;
  o.q_us[0] = n ? mn : 0; o.q_us[4] = mx;
  auto quantile = [&](double pt) -> u32 {   // the element at min(n - 1, floor(n * q)): the smallest v with count(x <= v) > that index
    if (n == 0) return 0u;
    const u32 want = min(n - 1, (u32)floor((double)n * pt));
    u32 lo = mn, hi = mx;
    while (lo < hi) {
      const u32 mid = lo + (hi - lo) / 2;
      u32 c = 0;
      for (u32 e = first; e < b; e += step) c += s[e] <= mid ? 1u : 0u;
      if (WAVE) c = wv_sum(c);
      if (c > want) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  o.q_us[1] = quantile(0.5); o.q_us[2] = quantile(0.95); o.q_us[3] = quantile(0.99);
  if (!WAVE || lane == 0) *dst = o;
}

__global__ void __launch_bounds__(64) perf_check_kernel(const PParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32 *const L = reinterpret_cast<u32 *>(smem);
  u32 *const sorted = L;               // [cap] the latencies by group
  u32 *const hist = L + p.off_hist;    // [G] paired ops per group
  u32 *const end = L + p.off_end;      // [G] the group's span in `sorted`: first its start (the scatter's cursor), then its end
  u32 *const cnt = L + p.off_cnt;      // [NF x NT] completions per (f, type)
  u32 *const unp = L + p.off_unp;      // [NF] completions without an invocation
  u32 *const lm = L + p.off_lm;        // [C x 2] the lanes of the current chunk that hold a row of the worker thread
  u32 *const tbl = L + p.off_tbl;      // [C x 3] the worker thread's last row of the chunks before: time lo, time hi, packed

  const u32 lane = threadIdx.x, inst = blockIdx.x;
  const u32 Wd = p.W ? p.W : 1u, G = NF * NT * Wd, C = p.C;
  const u32 n = min(p.meta[inst].n_rows, p.max_rows);
  const uint4 *const rows = reinterpret_cast<const uint4 *>(p.rows + (size_t)inst * p.max_rows);
  uint2 *const recs = p.recs + (size_t)inst * p.cap;
  const u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes below this one

  for (u32 i = lane; i < G; i += 64) hist[i] = 0;
  for (u32 i = lane; i < NF * NT; i += 64) cnt[i] = 0;
  for (u32 i = lane; i < NF; i += 64) unp[i] = 0;
  for (u32 i = lane; i < C; i += 64) { lm[2 * i] = 0; lm[2 * i + 1] = 0; tbl[3 * i] = 0; tbl[3 * i + 1] = 0; tbl[3 * i + 2] = MSIM_T_OK; /* no invocation pending */ }
  __syncthreads();

  // ---- pass 1 ----
  u32 n_inv = 0, n_paired = 0;
  auto ldrow = [&](u32 b) -> uint4 { return rows[min(b + lane, n ? n - 1 : 0u)]; };   // (past the end: the last row again, never used)
  uint4 nxt = n ? ldrow(0) : make_uint4(0, 0, 0, 0);
  for (u32 base = 0; base < n; base += 64) {
    const uint4 r = nxt;
    if (base + 64 < n) nxt = ldrow(base + 64);
    const u32 type = r.z & 3u, f = (r.z >> 2) & 31u, proc = r.z >> 12;
    const bool live = base + lane < n && proc != MSIM_PROCESS_NEMESIS;
    const bool comp = live && type != MSIM_T_INVOKE;
    const u32 slot = live ? proc % C : 0u;   // the worker thread ([upstream] jepsen's interpreter)
    n_inv += live && type == MSIM_T_INVOKE ? 1u : 0u;
    if (comp) atomicAdd(&cnt[f * NT + type - 1], 1u);
    if (live) atomicOr(&lm[2 * slot + (lane >> 5)], 1u << (lane & 31u));
    wv_fence();
    // the previous row of the worker thread: the nearest lane below with the same thread, else what the chunks before left in the table
    const u64 m = live ? ((u64)lm[2 * slot] | ((u64)lm[2 * slot + 1] << 32)) : 0ull;
    const u64 below = m & lt;
    u32 px = 0, py = 0, pz = MSIM_T_OK;
    if (comp && !below) { px = tbl[3 * slot]; py = tbl[3 * slot + 1]; pz = tbl[3 * slot + 2]; }
    const u32 pl = below ? 63u - (u32)__clzll((long long)below) : lane;
    const u32 sx = (u32)__shfl((int)r.x, (int)pl), sy = (u32)__shfl((int)r.y, (int)pl), sz = (u32)__shfl((int)r.z, (int)pl);
    if (comp && below) { px = sx; py = sy; pz = sz; }
    wv_fence();
    if (live && !((m >> lane) >> 1)) {   // the thread's last row of this chunk stays behind; its lane mask is cleared for the next chunk
      tbl[3 * slot] = r.x; tbl[3 * slot + 1] = r.y; tbl[3 * slot + 2] = r.z;
      lm[2 * slot] = 0; lm[2 * slot + 1] = 0;
    }
    const bool paired = comp && (pz & 3u) == MSIM_T_INVOKE && (pz >> 12) == proc;
    if (comp && !paired) atomicAdd(&unp[f], 1u);
    const u64 pm = __ballot(paired);   // (every lane has passed the table update above when this returns)
    if (paired) {
      const u64 t = ((u64)(r.y & 0xFFFFu) << 32) | r.x, tp = ((u64)(py & 0xFFFFu) << 32) | px;   // 64-bit ns: a 5 s timeout is beyond 2^32 ns
      const u64 d = t > tp ? (t - tp) / 1000ull : 0ull;
      const u32 lat = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)d;
      u32 w = 0;
      if (p.W) { const u64 wq = tp / p.window_ns; w = wq < (u64)(p.W - 1) ? (u32)wq : p.W - 1; }
      const u32 key = (f * NT + type - 1) * Wd + w;
      const u32 rank = n_paired + (u32)__popcll(pm & lt);
      if (rank < p.cap) { recs[rank] = make_uint2(lat, key); atomicAdd(&hist[key], 1u); }   // (a pair takes two rows: rank < max_rows / 2 always)
    }
    n_paired += (u32)__popcll(pm);
  }
  n_paired = min(n_paired, p.cap);
  __threadfence_block();
  __syncthreads();

  // ---- sort by group: exclusive prefix sums, every lane a contiguous block of groups; then the scatter ----
  {
    const u32 B = (G + 63) / 64;
    u32 s = 0;
    for (u32 k = 0; k < B; k++) { const u32 g = lane * B + k; if (g < G) s += hist[g]; }
    u32 incl = s;
    for (u32 o = 1; o < 64; o <<= 1) { const u32 v = (u32)__shfl_up((int)incl, o); if (lane >= o) incl += v; }
    u32 run = incl - s;
    for (u32 k = 0; k < B; k++) { const u32 g = lane * B + k; if (g < G) { end[g] = run; run += hist[g]; } }
  }
  __syncthreads();
  for (u32 i = lane; i < n_paired; i += 64) {
    const uint2 rc = recs[i];
    const u32 pos = atomicAdd(&end[rc.y], 1u);
    if (pos < p.cap) sorted[pos] = rc.x;
  }
  __syncthreads();

  // ---- :stats ----
  u32 c_ok = 0, c_fail = 0, c_info = 0;
  if (lane < NF) { c_ok = cnt[lane * NT]; c_fail = cnt[lane * NT + 1]; c_info = cnt[lane * NT + 2]; }
  const bool has = c_ok + c_fail + c_info > 0;
  const u32 fmask = (u32)__ballot(has);
  const u32 invalid = (u32)__ballot(has && c_ok == 0 && lane != MSIM_F_CRASH);
  const u32 t_ok = wv_sum(c_ok), t_fail = wv_sum(c_fail), t_info = wv_sum(c_info), t_inv = wv_sum(n_inv);
  const u32 n_dist = (u32)__popc(fmask), n_f = min(n_dist, (u32)MSIM_PERF_MAX_F);
  msim_perf_result *const o = p.out + inst;
  if (lane == 0) {
    o->valid = invalid ? 0u : 1u; o->n_f = n_f; o->count = t_ok + t_fail + t_info; o->ok_count = t_ok; o->fail_count = t_fail; o->info_count = t_info;
    o->open_count = t_inv - n_paired; o->flags = n_dist > MSIM_PERF_MAX_F ? 1u : 0u;
  }
  {
    const u32 k = has ? (u32)__popc(fmask & ((1u << lane) - 1u)) : lane - 32u;   // lanes 32..35 write the slots no :f uses
    const bool used = has && k < MSIM_PERF_MAX_F, unused = lane >= 32u && k >= n_f && k < MSIM_PERF_MAX_F;
    if (used || unused) {
      msim_f_stats *const fs = &o->by_f[k];
      fs->f = used ? lane : 0xFFFFFFFFu; fs->valid = used && c_ok > 0 ? 1u : 0u; fs->count = c_ok + c_fail + c_info;
      fs->ok_count = c_ok; fs->fail_count = c_fail; fs->info_count = c_info; fs->unpaired = used ? unp[lane] : 0u; fs->reserved = 0;
    }
  }

  // ---- the latency records: SLOTS over the whole history, then SLOTS per window ----
  const u32 R = SLOTS * (1u + p.W);
  auto span = [&](u32 rid, u32 &a, u32 &b) -> msim_latency_dist * {
    const u32 q = rid % SLOTS, k = q / NT, t = q % NT;
    msim_latency_dist *dst;
    u32 g0, g1;
    const u32 fk = k < n_f ? p_kth_bit(fmask, k) : 0u;
    if (rid < SLOTS) { dst = &o->by_f[k].latency[t]; g0 = (fk * NT + t) * Wd; g1 = g0 + Wd - 1; }
    else { const u32 w = rid / SLOTS - 1; dst = p.win + ((size_t)inst * p.W + w) * SLOTS + q; g0 = g1 = (fk * NT + t) * Wd + w; }
    if (k < n_f) { a = end[g0] - hist[g0]; b = end[g1]; } else { a = 0; b = 0; }
    return dst;
  };
  for (u32 rid = 0; rid < R; rid++) {   // the long spans, the wavefront on one at a time (a span's length is the same for every lane)
    u32 a, b;
    msim_latency_dist *const dst = span(rid, a, b);
    if (b - a > SERIAL_MAX) p_select<true>(sorted, a, b, lane, dst);
  }
  for (u32 rid = lane; rid < R; rid += 64) {   // the short and the empty ones, a lane each
    u32 a, b;
    msim_latency_dist *const dst = span(rid, a, b);
    if (b - a <= SERIAL_MAX) p_select<false>(sorted, a, b, lane, dst);
  }
}

const char *perf_args(uint32_t window_ms, uint32_t n_windows, const void *windows) {
  if (n_windows > MSIM_PERF_MAX_WINDOWS) return "at most MSIM_PERF_MAX_WINDOWS (16) windows";
  if (n_windows && windows && window_ms == 0) return "window_ms must not be 0 when windows are requested";
  return nullptr;
}

// one wavefront per history over n slabs; the caller owns the buffers and the stream
hipError_t perf_dispatch(PParams &pp, u32 n, hipStream_t st) {
  pp.cap = std::max(1u, pp.max_rows / 2);
  const u32 G = NF * NT * (pp.W ? pp.W : 1u);
  u32 off = pp.cap;
  pp.off_hist = off; off += G;
  pp.off_end = off; off += G;
  pp.off_cnt = off; off += NF * NT;
  pp.off_unp = off; off += NF;
  pp.off_lm = off; off += 2 * pp.C;
  pp.off_tbl = off; off += 3 * pp.C;
  const size_t lds = (size_t)off * 4;   // <= 131068 + 12288 + 512 + 2560 bytes: inside the 160 KiB of a CU for every accepted shape
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&perf_check_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(perf_check_kernel, dim3(n), dim3(64), lds, st, pp);
  return hipGetLastError();
}

const char *perf_limits(u32 max_rows, u32 concurrency) {
  if (max_rows >= 0xFFFF || concurrency > 128 || concurrency == 0) return "device checker: max_rows must be < 65535, concurrency 1..128";
  return nullptr;
}

size_t perf_align(size_t v) { return (v + 255) & ~(size_t)255; }

msim_latency_dist dist_of(std::vector<u32> &v) {
  msim_latency_dist d;
  std::memset(&d, 0, sizeof d);
  if (v.empty()) return d;
  std::sort(v.begin(), v.end());
  const double pts[5] = {0.0, 0.5, 0.95, 0.99, 1.0};
  const size_t n = v.size();
  d.count = (u32)n;
  for (int i = 0; i < 5; i++) d.q_us[i] = v[std::min(n - 1, (size_t)std::floor((double)n * pts[i]))];
  for (u32 x : v) d.sum_us += x;
  return d;
}

}  // namespace

// One history on the host: the statement of the contract in plain C++ (the device kernel is compared with it field by field).
extern "C" int msim_check_perf_rows(const msim_op *rows, uint32_t n_rows, uint32_t concurrency, uint32_t window_ms, uint32_t n_windows,
                                    msim_perf_result *out, msim_latency_dist *windows) {
  if ((!rows && n_rows) || !out || concurrency == 0 || perf_args(window_ms, n_windows, windows)) return MSIM_E_INVALID;
  const u32 W = windows ? n_windows : 0;
  const u64 window_ns = (u64)window_ms * 1000000ull;
  struct Last { bool invoke = false; u32 process = 0; u64 t = 0; };
  std::vector<Last> last(concurrency);
  std::vector<std::vector<u32>> whole(NF * NT), win((size_t)NF * NT * W);
  u32 cnt[NF][NT] = {}, unp[NF] = {}, n_inv = 0, n_paired = 0;
  for (u32 i = 0; i < n_rows; i++) {
    const msim_op &r = rows[i];
    const u32 proc = MSIM_OP_PROCESS(r), type = MSIM_OP_TYPE(r), f = MSIM_OP_F(r);
    if (proc == MSIM_PROCESS_NEMESIS) continue;
    Last &l = last[proc % concurrency];
    const u64 t = MSIM_OP_TIME_NS(r);
    if (type != MSIM_T_INVOKE) {
      cnt[f][type - 1]++;
      if (l.invoke && l.process == proc) {
        const u64 d = t > l.t ? (t - l.t) / 1000ull : 0ull;
        const u32 lat = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)d;
        whole[f * NT + type - 1].push_back(lat);
        if (W) win[(size_t)std::min<u64>(l.t / window_ns, W - 1) * NF * NT + f * NT + type - 1].push_back(lat);
        n_paired++;
      } else unp[f]++;
    } else n_inv++;
    l.invoke = type == MSIM_T_INVOKE; l.process = proc; l.t = t;
  }
  std::memset(out, 0, sizeof *out);
  if (W) std::memset(windows, 0, (size_t)W * SLOTS * sizeof(msim_latency_dist));
  out->valid = 1; out->open_count = n_inv - n_paired;
  u32 n_dist = 0;
  for (u32 f = 0; f < NF; f++) {
    const u32 c = cnt[f][0] + cnt[f][1] + cnt[f][2];
    if (!c) continue;
    out->count += c; out->ok_count += cnt[f][0]; out->fail_count += cnt[f][1]; out->info_count += cnt[f][2];
    if (cnt[f][0] == 0 && f != MSIM_F_CRASH) out->valid = 0;
    const u32 k = n_dist++;
    if (k >= MSIM_PERF_MAX_F) continue;
    msim_f_stats &fs = out->by_f[k];
    fs.f = f; fs.valid = cnt[f][0] > 0; fs.count = c; fs.ok_count = cnt[f][0]; fs.fail_count = cnt[f][1]; fs.info_count = cnt[f][2]; fs.unpaired = unp[f];
    for (u32 t = 0; t < NT; t++) {
      fs.latency[t] = dist_of(whole[f * NT + t]);
      for (u32 w = 0; w < W; w++) windows[((size_t)w * MSIM_PERF_MAX_F + k) * NT + t] = dist_of(win[(size_t)w * NF * NT + f * NT + t]);
    }
  }
  out->n_f = std::min(n_dist, (u32)MSIM_PERF_MAX_F);
  out->flags = n_dist > MSIM_PERF_MAX_F ? 1u : 0u;
  for (u32 k = out->n_f; k < MSIM_PERF_MAX_F; k++) out->by_f[k].f = 0xFFFFFFFFu;
  return MSIM_OK;
}

// Every history of the last run, where the rows lie in HBM, on the context's stream.
extern "C" int msim_check_perf(msim_ctx *ctx, uint32_t window_ms, uint32_t n_windows, msim_perf_result *out, uint32_t n_out, msim_latency_dist *windows) {
  if (!ctx || !out) return MSIM_E_INVALID;
  if (!ctx->ran) { ctx->err = "msim_check_perf before msim_run"; return MSIM_E_RANGE; }
  if (const char *why = perf_args(window_ms, n_windows, windows)) { ctx->err = std::string("msim_check_perf: ") + why; return MSIM_E_INVALID; }
  if (n_out < ctx->n_inst) { ctx->err = "msim_check_perf: output array shorter than the run"; return MSIM_E_RANGE; }
  if (const char *why = perf_limits(ctx->cfg.max_rows, ctx->cfg.concurrency)) { ctx->err = why; return MSIM_E_UNSUPPORTED; }
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const u32 n = ctx->n_inst, W = windows ? n_windows : 0;
  PParams pp;
  std::memset(&pp, 0, sizeof pp);
  pp.max_rows = ctx->cfg.max_rows; pp.C = ctx->cfg.concurrency; pp.W = W; pp.window_ns = (u64)window_ms * 1000000ull;
  // one cached block: the records of pass 1, the results, the window records
  const size_t rec_bytes = perf_align((size_t)n * std::max(1u, pp.max_rows / 2) * sizeof(uint2)), out_bytes = perf_align((size_t)n * sizeof(msim_perf_result));
  const size_t win_bytes = (size_t)n * W * SLOTS * sizeof(msim_latency_dist), need = rec_bytes + out_bytes + win_bytes;
  if (int rc = grow_ws(ctx, &ctx->d_perf_scratch, &ctx->cap_perf_scratch, need)) return rc;
  unsigned char *const base = static_cast<unsigned char *>(ctx->d_perf_scratch);
  pp.rows = ctx->d_rows; pp.meta = ctx->d_meta; pp.recs = reinterpret_cast<uint2 *>(base);
  pp.out = reinterpret_cast<msim_perf_result *>(base + rec_bytes);
  pp.win = W ? reinterpret_cast<msim_latency_dist *>(base + rec_bytes + out_bytes) : nullptr;
  const bool timed = (msim_dev_flags(ctx) & 0x1000u) != 0;   // developer trace bit: the kernel's own time on stderr (tools/perf_check_timing.py)
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (timed) { MSIM_HIP_TRY(ctx, hipEventCreate(&t0)); MSIM_HIP_TRY(ctx, hipEventCreate(&t1)); MSIM_HIP_TRY(ctx, hipEventRecord(t0, ctx->stream)); }
  MSIM_HIP_TRY(ctx, perf_dispatch(pp, n, ctx->stream));
  if (timed) MSIM_HIP_TRY(ctx, hipEventRecord(t1, ctx->stream));
  MSIM_HIP_TRY(ctx, hipMemcpyAsync(out, pp.out, (size_t)n * sizeof(msim_perf_result), hipMemcpyDeviceToHost, ctx->stream));
  if (W) MSIM_HIP_TRY(ctx, hipMemcpyAsync(windows, pp.win, win_bytes, hipMemcpyDeviceToHost, ctx->stream));
  MSIM_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (timed) {
    float ms = 0.f;
    MSIM_HIP_TRY(ctx, hipEventElapsedTime(&ms, t0, t1));
    std::fprintf(stderr, "[perf-check] kernel %.4f ms over %u histories, %u windows\n", ms, n, W);
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
  }
  return MSIM_OK;
}

// Histories given on the host in slabs of `max_rows` rows (history i at rows + i * max_rows, n_rows[i] of them used) through the kernel.
extern "C" int msim_check_perf_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, uint32_t concurrency,
                                     uint32_t window_ms, uint32_t n_windows, msim_perf_result *out, msim_latency_dist *windows) {
  if (!rows || !n_rows || !out || n_histories == 0 || max_rows == 0 || perf_args(window_ms, n_windows, windows)) return MSIM_E_INVALID;
  if (perf_limits(max_rows, concurrency)) return MSIM_E_UNSUPPORTED;
  BatchFrame<SlabBatch> f(device); msim_ctx *ctx = &f.ctx;
  if (int rc = f.begin(n_histories, sizeof(msim_perf_result), rows, n_rows, max_rows, n_histories)) return rc;
  const u32 W = windows ? n_windows : 0;
  PParams pp;
  std::memset(&pp, 0, sizeof pp);
  pp.max_rows = max_rows; pp.C = concurrency; pp.W = W; pp.window_ns = (u64)window_ms * 1000000ull;
  const size_t win_bytes = (size_t)n_histories * W * SLOTS * sizeof(msim_latency_dist);
  DevBuf d_win, d_rec;
  if (W) MSIM_HIP_TRY(ctx, d_win.alloc(win_bytes));
  MSIM_HIP_TRY(ctx, d_rec.alloc((size_t)n_histories * std::max(1u, max_rows / 2) * sizeof(uint2)));
  pp.rows = f.b.rows.get<msim_op>(); pp.meta = f.b.meta.get<msim_inst_meta>();
  pp.out = f.d_out.get<msim_perf_result>(); pp.win = d_win.get<msim_latency_dist>(); pp.recs = d_rec.get<uint2>();
  MSIM_HIP_TRY(ctx, perf_dispatch(pp, n_histories, nullptr));
  MSIM_HIP_TRY(ctx, hipDeviceSynchronize());
  MSIM_HIP_TRY(ctx, hipMemcpy(out, pp.out, (size_t)n_histories * sizeof(msim_perf_result), hipMemcpyDeviceToHost));
  if (W) MSIM_HIP_TRY(ctx, hipMemcpy(windows, pp.win, win_bytes, hipMemcpyDeviceToHost));
  return MSIM_OK;
}
