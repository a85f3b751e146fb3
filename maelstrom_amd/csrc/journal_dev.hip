// journal_dev.hip — the net journal's messages on the device (include/maelsim_journal.h: the contract; journal.cpp: the host walk):
// every :send joined to its :recv (the reference's net/viz.clj:27-56 `messages`), the counts of net/checker.clj:28-41, the undelivered
// messages and the delivery latencies per class, where the journals lie in HBM.  journal_messages_kernel, one workgroup per journal,
// keeps four words per message id in the grow-only workspace — the send's position and class, its record's index, the recv that claimed
// it, the latency — and sweeps the events twice: the sends number their records and enter the table, the recvs look their send up
// and claim it.  What the walk's map would notice — an id sent twice, a recv without an earlier send, a second recv — the table
// notices too, and such a journal (and one with an id beyond its events) is not analysed here: its summary says NEEDS_HOST and the host
// walk redoes it whole.  A well-formed journal never leaves the device.  docs/KERNELS.md, "journal_messages_kernel".
#include <hip/hip_runtime.h>

#include <cstdio>

#include "check_run.h"
#include "check_dev.h"

namespace {

constexpr u32 NEEDS_HOST = 3u;   // msim_journal_summary.valid of a journal the device leaves to the host walk
constexpr u32 JWG = 256;         // threads per journal: the width of a block of events
constexpr u32 JWAVES = JWG / 64;
constexpr u32 WS_WORDS = 4;      // workspace words per event of a journal: tab, rec, rcv, lat (each indexed by message id)

struct JParams {
  const uint4 *events;            // 16 bytes each
  const u64 *ev_off;              // a caller's batch: journal i at ev_off[i] .. ev_off[i + 1]; null: a run's slab
  const msim_inst_meta *meta;     // a run's slab: journal i at i * capacity, min(n_events, capacity) events
  msim_journal_summary *sum; uint4 *msgs /* two per record */;
  u32 *ws;                        // WS_WORDS * stride words per journal of the launch
  u32 capacity, stride, max_msgs, n_nodes, client_slots, first;
};

// LDS words of a workgroup
enum { S_BAD, S_SEND_C, S_SEND_S, S_RECV_C, S_RECV_S, S_DELIV_C, S_DELIV_S, S_CROSS_C, S_CROSS_S, S_MIN_C, S_MIN_S, S_MAX_C, S_MAX_S, S_BITMAP, S_WTOT = S_BITMAP + 8,
       S_RED = S_WTOT + 2 * JWAVES, S_WORDS = S_RED + 2 * JWAVES };

// the workgroup's sum of v (every thread calls; `par` alternates the slots, so one barrier a call is enough)
__device__ __forceinline__ u32 wg_sum(u32 *s, u32 v, u32 &par, u32 tid) {
  v = wv_sum(v);
  if ((tid & 63u) == 0) s[S_RED + par * JWAVES + (tid >> 6)] = v;
  __syncthreads();
  u32 t = 0;
  for (u32 w = 0; w < JWAVES; w++) t += s[S_RED + par * JWAVES + w];
  par ^= 1u;
  return t;
}

__global__ void __launch_bounds__(JWG) journal_messages_kernel(const JParams p) {
  __shared__ u32 s[S_WORDS];
  __shared__ u64 s_sum[2];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, j = p.first + blockIdx.x;
  const uint4 *const ev = p.events + (p.ev_off ? p.ev_off[j] : (u64)j * p.capacity);
  const u32 n = p.ev_off ? (u32)(p.ev_off[j + 1] - p.ev_off[j]) : min(p.meta[j].n_events, p.capacity);
  u32 *const tab = p.ws + (u64)blockIdx.x * WS_WORDS * p.stride;   // [id] the send's position + 1, bit 31: a servers message; 0: not sent
  u32 *const rec = tab + p.stride;                                  // [id] the send's record index
  u32 *const rcv = rec + p.stride;                                  // [id] the recv that claimed the send; MSIM_NO_VALUE: none
  u32 *const lat = rcv + p.stride;                                  // [id] its latency
  uint4 *const out = p.msgs + (u64)j * p.max_msgs * 2u;
  for (u32 i = tid; i < n; i += JWG) { tab[i] = 0u; rcv[i] = MSIM_NO_VALUE; }
  for (u32 i = tid; i < S_WORDS; i += JWG) s[i] = (i == S_MIN_C || i == S_MIN_S) ? MSIM_NO_VALUE : 0u;
  if (tid < 2) s_sum[tid] = 0;
  __syncthreads();

  // ---- sweep 1: the counts, the endpoints, every send's record and table entry ----------------------------------------------------
  u32 send_c = 0, send_s = 0, recv_c = 0, recv_s = 0, carry = 0, bad = 0;
  for (u32 base = 0, it = 0; base < n; base += JWG, it++) {
    const u32 idx = base + tid;
    const bool live = idx < n;
    const uint4 e = live ? ev[idx] : make_uint4(0u, 0x80u, 0u, 0u);   // {time_us, msg, a, route}
    const u32 id = e.y >> 8, src = e.w & 0xFFu, dest = (e.w >> 8) & 0xFFu;
    const bool send = live && !(e.y & 0x80u), client = src - p.n_nodes < p.client_slots || dest - p.n_nodes < p.client_slots;
    if (live) {
      send_c += send && client; send_s += send && !client; recv_c += !send && client; recv_s += !send && !client;
      if (!(s[S_BITMAP + (src >> 5)] >> (src & 31u) & 1u)) atomicOr(&s[S_BITMAP + (src >> 5)], 1u << (src & 31u));
      if (!(s[S_BITMAP + (dest >> 5)] >> (dest & 31u) & 1u)) atomicOr(&s[S_BITMAP + (dest >> 5)], 1u << (dest & 31u));
      if (id >= n) bad = 1u;
    }
    // the record index: the sends before this one in the block (a ballot per wavefront, the wavefronts' totals through LDS) + the carry
    const u64 m = __ballot(send);
    const u32 before = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
    u32 *const wtot = s + S_WTOT + (it & 1u) * JWAVES;   // (alternating: one barrier a block)
    if (lane == 0) wtot[wave] = (u32)__popcll(m);
    __syncthreads();
    u32 k = carry + before;
    for (u32 w = 0; w < JWAVES; w++) { const u32 t = wtot[w]; if (w < wave) k += t; carry += t; }
    if (send) {
      if (k < p.max_msgs) {   // a wavefront's sends are neighbours: 16 bytes a lane, twice
        out[2u * k] = make_uint4(id, idx, MSIM_NO_VALUE, e.x);
        out[2u * k + 1u] = make_uint4(MSIM_NO_VALUE, (e.y & 0x7Fu) | (client ? 0x80u : 0u), e.w, e.z);
      }
      if (id < n) {
        if (atomicCAS(&tab[id], 0u, (idx + 1u) | (client ? 0u : 0x80000000u)) != 0u) bad = 1u;   // sent before
        else rec[id] = k;
      }
    }
  }
  if (bad) s[S_BAD] = 1u;
  // the barrier orders the table and the records, written through HBM by every wavefront, in front of the recvs that read them
  __syncthreads();
  if (s[S_BAD]) {
    if (tid == 0) p.sum[j].valid = NEEDS_HOST;
    return;
  }

  // ---- sweep 2: every recv finds its send and claims it ---------------------------------------------------------------------------
  u32 deliv_c = 0, deliv_s = 0, cross_c = 0, cross_s = 0, min_c = MSIM_NO_VALUE, min_s = MSIM_NO_VALUE, max_c = 0, max_s = 0;
  u64 sum_c = 0, sum_s = 0;
  for (u32 idx = tid; idx < n; idx += JWG) {
    const uint4 e = ev[idx];
    if (!(e.y & 0x80u)) continue;
    const u32 id = e.y >> 8, src = e.w & 0xFFu, dest = (e.w >> 8) & 0xFFu;   // (id < n: sweep 1 looked)
    const bool client = src - p.n_nodes < p.client_slots || dest - p.n_nodes < p.client_slots;
    const u32 t = tab[id], pos = (t & 0x7FFFFFFFu) - 1u;
    if (t == 0u || pos > idx) { bad = 1u; continue; }                         // no send, or none so far
    if (atomicCAS(&rcv[id], MSIM_NO_VALUE, idx) != MSIM_NO_VALUE) { bad = 1u; continue; }   // a second recv
    const u32 sent = ev[pos].x, l = e.x > sent ? e.x - sent : 0u, k = rec[id];
    const bool to_client = !(t >> 31);
    lat[id] = l;
    if (k < p.max_msgs) { u32 *const w = reinterpret_cast<u32 *>(out + 2u * k); w[2] = idx; w[4] = l; }
    if (to_client) { deliv_c++; sum_c += l; min_c = min(min_c, l); max_c = max(max_c, l); }
    else { deliv_s++; sum_s += l; min_s = min(min_s, l); max_s = max(max_s, l); }
    if (client != to_client) { cross_c += client; cross_s += !client; }     // the id occurs in the recv's class too (msg_count)
  }
  if (bad) s[S_BAD] = 1u;
  atomicAdd(&s[S_SEND_C], send_c); atomicAdd(&s[S_SEND_S], send_s); atomicAdd(&s[S_RECV_C], recv_c); atomicAdd(&s[S_RECV_S], recv_s);
  atomicAdd(&s[S_DELIV_C], deliv_c); atomicAdd(&s[S_DELIV_S], deliv_s); atomicAdd(&s[S_CROSS_C], cross_c); atomicAdd(&s[S_CROSS_S], cross_s);
  atomicMin(&s[S_MIN_C], min_c); atomicMin(&s[S_MIN_S], min_s); atomicMax(&s[S_MAX_C], max_c); atomicMax(&s[S_MAX_S], max_s);
  atomicAdd(&s_sum[0], sum_c); atomicAdd(&s_sum[1], sum_s);
  __syncthreads();
  if (s[S_BAD]) {
    if (tid == 0) p.sum[j].valid = NEEDS_HOST;
    return;
  }

  // ---- the quantiles of a class: the want-th smallest latency by bisection on the value, counted over the table ------------------
  u32 par = 0, q_c1 = 0, q_c2 = 0, q_c3 = 0, q_s1 = 0, q_s2 = 0, q_s3 = 0;
  for (u32 c = 0; c < 2; c++) {
    const u32 cnt = s[S_DELIV_C + c];
    if (!cnt) continue;
    for (u32 qi = 1; qi < 4; qi++) {   // (quantile 0 is the minimum, quantile 1 the maximum)
      const double q = qi == 1 ? 0.5 : qi == 2 ? 0.95 : 0.99;
      const u32 want = min(cnt - 1u, (u32)floor((double)cnt * q));
      u32 lo = s[S_MIN_C + c], hi = s[S_MAX_C + c];   // the smallest v with count(latency <= v) > want
      while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2u;
        u32 below = 0;
        for (u32 id = tid; id < n; id += JWG) {
          const u32 t = tab[id];
          below += (t != 0u && (t >> 31) == c && rcv[id] != MSIM_NO_VALUE && lat[id] <= mid) ? 1u : 0u;
        }
        if (wg_sum(s, below, par, tid) > want) hi = mid; else lo = mid + 1u;
      }
      if (c == 0) { if (qi == 1) q_c1 = lo; else if (qi == 2) q_c2 = lo; else q_c3 = lo; }
      else { if (qi == 1) q_s1 = lo; else if (qi == 2) q_s2 = lo; else q_s3 = lo; }
    }
  }

  if (tid == 0) {
    msim_journal_summary o;
    const u32 sc = s[S_SEND_C], ss = s[S_SEND_S], rc = s[S_RECV_C], rs = s[S_RECV_S], dc = s[S_DELIV_C], ds = s[S_DELIV_S];
    o.valid = 1u; o.n_events = n;
    o.flags = (sc + ss > p.max_msgs ? MSIM_JOURNAL_TABLE_TRUNCATED : 0u) | (p.meta && (p.meta[j].flags & MSIM_FLAG_JOURNAL_OVERFLOW) ? MSIM_JOURNAL_TRUNCATED : 0u);
    o.n_msgs = sc + ss;
    o.send_count[0] = sc + ss; o.send_count[1] = sc; o.send_count[2] = ss;
    o.recv_count[0] = rc + rs; o.recv_count[1] = rc; o.recv_count[2] = rs;
    o.msg_count[0] = sc + ss; o.msg_count[1] = sc + s[S_CROSS_C]; o.msg_count[2] = ss + s[S_CROSS_S];   // (well-formed: one send an id)
    o.undelivered[0] = sc + ss - dc - ds; o.undelivered[1] = sc - dc; o.undelivered[2] = ss - ds;
    o.dup_sends = 0; o.orphan_recvs = 0; o.extra_recvs = 0;
    o.n_nodes = p.n_nodes; o.client_slots = p.client_slots;
    o.reserved[0] = 0; o.reserved[1] = 0; o.reserved[2] = 0;
    for (int i = 0; i < 8; i++) o.endpoints[i] = s[S_BITMAP + i];
    o.latency[0].count = dc; o.latency[0].sum_us = s_sum[0];
    o.latency[0].q_us[0] = dc ? s[S_MIN_C] : 0u; o.latency[0].q_us[1] = q_c1; o.latency[0].q_us[2] = q_c2; o.latency[0].q_us[3] = q_c3; o.latency[0].q_us[4] = s[S_MAX_C];
    o.latency[1].count = ds; o.latency[1].sum_us = s_sum[1];
    o.latency[1].q_us[0] = ds ? s[S_MIN_S] : 0u; o.latency[1].q_us[1] = q_s1; o.latency[1].q_us[2] = q_s2; o.latency[1].q_us[3] = q_s3; o.latency[1].q_us[4] = s[S_MAX_S];
    p.sum[j] = o;
  }
}

// The launches over n journals of at most `longest` events, in chunks of the grow-only workspace *ws; the summaries and the record
// slabs to the caller's arrays; the journals that are not well-formed to the host walk (*n_host).
int journal_dev_run(msim_ctx *ctx, JParams p, u32 n, u32 longest, void **ws, size_t *ws_cap, hipStream_t st, msim_journal_summary *summaries, msim_journal_msg *msgs,
                    u32 *n_host) {
  ExplainSlabs<msim_journal_summary, msim_journal_msg> xs;
  if (int rc = xs.alloc(ctx, n, p.max_msgs, summaries, msgs)) return rc;
  if (int rc = xs.clear(ctx, st)) return rc;
  p.sum = xs.hdr(); p.msgs = reinterpret_cast<uint4 *>(xs.rec());
  p.stride = std::max(longest, 1u);
  const int launches = chunked_pass(ctx, n, (uint64_t)p.stride * WS_WORDS * 4, 4ull << 30, nullptr, ws, ws_cap, [&](const u32 *, void *w, u32 first, u32 count) {
    p.ws = static_cast<u32 *>(w); p.first = first;
    hipLaunchKernelGGL(journal_messages_kernel, dim3(count), dim3(JWG), 0, st, p);
  }, xs.hdr(), summaries, n, st);
  if (launches < 0) return launches;
  if (int rc = xs.fetch(ctx, st)) return rc;
  std::vector<u32> todo;
  for (u32 i = 0; i < n; i++) if (summaries[i].valid == NEEDS_HOST) todo.push_back(i);
  if (msim_dev_flags(ctx) & 0x1000u) std::fprintf(stderr, "[journal] journal_messages_kernel over %u journals (%d launches), %zu to the host walk\n", n, launches, todo.size());   // developer trace bit
  if (n_host) *n_host = (u32)todo.size();
  if (todo.empty()) return MSIM_OK;
  // a run's meta records on the host, for hand_off: n_rows the events analysed (behind the launches: xs.fetch has waited for the stream)
  std::vector<msim_inst_meta> hm;
  if (p.meta) {
    hm.resize(n);
    MSIM_HIP_TRY(ctx, hipMemcpy(hm.data(), p.meta, (size_t)n * sizeof(msim_inst_meta), hipMemcpyDeviceToHost));
    for (auto &m : hm) m.n_rows = std::min(m.n_events, p.capacity);
  }
  // (the events go as hand_off's 16-byte rows; the truncation flag of a run's journal is the device's to add: the walk knows no run)
  const HistorySource hs{reinterpret_cast<const msim_op *>(p.events), nullptr, p.meta ? &hm : nullptr, p.capacity, 0, p.ev_off, nullptr};
  return hand_off(ctx, hs, n, todo, summaries, xs.hdr(), [&](const msim_op *rows, u32 nr, const u32 *, u32, u32 flags, u32 i) {
    (void)msim_journal_messages_rows(reinterpret_cast<const msim_event *>(rows), nr, p.n_nodes, p.client_slots, &summaries[i], msgs + (size_t)i * p.max_msgs, p.max_msgs);
    if (flags & MSIM_FLAG_JOURNAL_OVERFLOW) summaries[i].flags |= MSIM_JOURNAL_TRUNCATED;
  });
}

}  // namespace

extern "C" int msim_journal_messages_batch(int device, const msim_event *events, const uint64_t *event_offsets, uint32_t n_journals, uint32_t n_nodes, uint32_t client_slots,
                                           msim_journal_summary *summaries, msim_journal_msg *msgs, uint32_t max_msgs, uint32_t *n_host) {
  if (!event_offsets || !summaries || n_journals == 0 || (!events && event_offsets[n_journals]) || (!msgs && max_msgs)) return MSIM_E_INVALID;
  BatchFrame<OffsetsBatch> f(device); msim_ctx *ctx = &f.ctx;
  if (int rc = f.begin(n_journals, 16, reinterpret_cast<const msim_op *>(events), event_offsets, nullptr, nullptr, n_journals, 0x7FFFFFFFull)) return rc;
  DevBuf ws; size_t ws_cap = 0;
  JParams p;
  std::memset(&p, 0, sizeof p);
  p.events = f.b.rows.get<uint4>(); p.ev_off = f.b.row_off.get<u64>(); p.max_msgs = max_msgs; p.n_nodes = n_nodes; p.client_slots = client_slots;
  return journal_dev_run(ctx, p, n_journals, f.b.longest, ws.addr(), &ws_cap, nullptr, summaries, msgs, n_host);
}

// The workspace is the context's d_perf_scratch: msim_check_perf and this entry both wait for their kernels before they return, so
// neither finds the other's launch still reading it — d_check_scratch may belong to a check queued behind the run.
extern "C" int msim_journal_messages(msim_ctx *ctx, msim_journal_summary *summaries, msim_journal_msg *msgs, uint32_t max_msgs, uint32_t n_out) {
  if (!ctx || !summaries || (!msgs && max_msgs)) return MSIM_E_INVALID;
  if (!ctx->cfg.journal_capacity) { ctx->err = "msim_journal_messages: journal_capacity is 0 (journal off)"; return MSIM_E_UNSUPPORTED; }
  if (int rc = explain_refusal(ctx, "msim_journal_messages", true, "", n_out)) return rc;
  MSIM_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const msim_config &c = ctx->cfg;
  const u32 n = ctx->n_inst;
  JParams p;
  std::memset(&p, 0, sizeof p);
  p.events = reinterpret_cast<const uint4 *>(ctx->d_journal); p.meta = ctx->d_meta; p.capacity = c.journal_capacity; p.max_msgs = max_msgs;
  p.n_nodes = c.n_nodes; p.client_slots = std::max(c.concurrency, c.n_nodes);
  return journal_dev_run(ctx, p, n, c.journal_capacity, &ctx->d_perf_scratch, &ctx->cap_perf_scratch, ctx->stream, summaries, msgs, nullptr);
}
