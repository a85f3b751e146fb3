// cycle_classify.inc — the classification of one history's dependency cycles, shared by the two transactional checkers on the
// device: rw_classify_kernel (rw_check_dev.hip, txn-rw-register) and txn_classify_kernel (txn_check_dev.hip, txn-list-append).  Included
// inside the including unit's unnamed namespace, after its `NONE` and check_dev.h (the wv_* helpers); one wavefront per history (blockDim.x == 64).  The front end builds
// the tagged edges (to | kind << 28) as a CSR and its reverse in its workspace; what this file reads beside them is CycleParams.
struct CycleParams {
  msim_check_result *out;
  u32 cm, proscribed;            // the consistency model and what it proscribes (msim_proscribed_anomalies)
  u32 ccap;                      // transactions of one strongly connected component the reachability matrix holds (<= CCAP)
  u32 big;                       // a larger component is searched in the workspace (0: it is the host's, MSIM_DEV_FLAGS bit 13)
};
// EXPLAIN (txn_explain_kernel / rw_explain_kernel): where the witness cycle of include/maelsim.h goes, and the rows of a transaction
struct CycleWitness {
  msim_cycle_result *cycles; msim_cycle_step *steps; u32 max_steps;   // history i's steps at steps + i * max_steps
  const u32 *t_inv, *t_cmp;                                           // a transaction's :invoke row and completion row (NONE: never completed)
};
__device__ __forceinline__ u64 cw_min64(u64 v) {
  for (int o = 32; o; o >>= 1) { const u32 lo = (u32)__shfl_xor((int)(u32)v, o), hi = (u32)__shfl_xor((int)(u32)(v >> 32), o); v = min(v, ((u64)hi << 32) | lo); }
  return v;
}
constexpr u32 CCAP = 256u;       // 256 x 256 bits of LDS: 8 KB per history
constexpr u32 E_WW = 1u, E_WR = 2u, E_RW = 4u, E_RT = 8u, E_TO = 0x0FFFFFFFu;   // the full graph's edges: to | kind << 28

// ---- the classification of one history's cycles (lane = transaction unless said otherwise) ---------------------------------------------
// What finish() and classify() of txn_check.cpp do with Tarjan's algorithm, restated for one wavefront over the tagged edges (off / adj)
// and their reverse (roff / radj):
//   * "is there a cycle over these edge kinds" is Kahn's algorithm over the masked edges (peel);
//   * the transactions in strongly connected components of more than one transaction: peel forwards and backwards until every
//     transaction left has a predecessor and a successor left; any chain of predecessors then ends in a cycle, so pointer doubling over
//     one predecessor each finds a transaction ON a cycle; its component is what a search along the edges and one against them both
//     reach; count it, take it out, peel again.  Every search is a queue, O(edges): the realtime edges form chains as long as the
//     history, which a sweep to a fixpoint would walk once per link;
//   * G-single: in a component, some rw edge u -> v whose v reaches u over ww + wr (+ realtime).  Such a path lies inside the component,
//     so reachability is closed (Warshall, rows of bits in LDS) over the component's transactions alone — ccap of them at the most.
//     A larger component (they grow with the history: a mean of 520 transactions at five nodes and 3000 transactions) would need a matrix
//     in HBM and s^3 / 64 word operations; the question only needs what the HEADS v of the component's rw edges reach, so those are
//     searched 64 at a time: a 64-bit word per transaction (reach, in the workspace), bit b = "head b of this batch reaches it", pushed
//     along the other edges inside the component from a worklist until nothing changes, then every rw edge into the batch is looked up.
//
// EXPLAIN: after the class is decided, the witness cycle (include/maelsim.h) in the arrays that are free by then.  Its start is the
// smallest transaction on a cycle over the class's mask — the minimum over the members of every component (G2: of the classification's
// own components, G0 / G1c: of one more pass over the narrower mask) — or, for G-single, the smallest head v of a rw edge u -> v whose
// v reaches u over the other kinds: read off the matrix, or the smallest hit of the first batch with one in the search, whose heads
// are numbered by transaction index for this; every component is asked, not only the first with a hit.  Then a BFS from it, one
// level at a time (a transaction's distance is set once, by compare-and-swap, while its level is expanded), the closing transaction by a
// minimum over the start's reversed edges, and the walk back: per step a minimum over one transaction's reversed edges.
template <bool EXPLAIN = false>
__device__ __forceinline__ void cycle_classify(const CycleParams &p, const u32 hist, msim_check_result &res, const u32 anomalies, const u32 n, const u32 n_edges,
                                            const u32 flags, const u32 c_ok, u32 *const deg, const u32 *const off, const u32 *const adj,
                                            const u32 *const roff, const u32 *const radj, u32 *const st, u32 *const jump, u32 *const queue, u64 *const reach,
                                            const CycleWitness *const cw = nullptr) {
  __shared__ u64 mat[CCAP * CCAP / 64];
  constexpr u32 GONE = 1u, FWD = 2u, BWD = 4u, QUEUED = 8u;
  const u32 lane = threadIdx.x;
  const u64 lt = (1ull << lane) - 1ull;
  auto reset = [&]() { for (u32 t = lane; t < n; t += 64) st[t] = 0; __syncthreads(); };
  // takes out (GONE), among the transactions left, those that no edge of `mask` enters from a transaction left, until there is none;
  // o / a: the edges followed, ro / ra: the same edges reversed.  Returns how many it took.
  auto peel = [&](const u32 *o, const u32 *a, const u32 *ro, const u32 *ra, const u32 mask) -> u32 {
    u32 tail = 0;
    for (u32 base = 0; base < n; base += 64) {
      const u32 t = base + lane;
      bool z = false;
      if (t < n && !(st[t] & GONE)) {
        u32 d = 0;
        for (u32 e = ro[t]; e < ro[t + 1]; e++) { const u32 x = ra[e]; d += ((x >> 28) & mask) && !(st[x & E_TO] & GONE); }
        deg[t] = d; z = d == 0;
      }
      const u64 zm = __ballot(z);
      if (z) queue[tail + (u32)__popcll(zm & lt)] = t;
      tail += (u32)__popcll(zm);
    }
    __syncthreads();
    u32 head = 0;
    while (head < tail) {
      const u32 cnt = min(64u, tail - head);
      const bool on = lane < cnt;
      const u32 v = on ? queue[head + lane] : 0u;
      const u32 a0 = on ? o[v] : 0u, a1 = on ? o[v + 1] : 0u;
      for (u32 k = 0; __ballot(a0 + k < a1); k++) {
        bool push = false; u32 wv = 0;
        if (a0 + k < a1) {
          const u32 x = a[a0 + k]; wv = x & E_TO;
          if (((x >> 28) & mask) && !(st[wv] & GONE)) push = atomicSub(&deg[wv], 1u) == 1u;   // (one taken in this call has no counted edge left)
        }
        const u64 pm = __ballot(push);
        if (push) queue[tail + (u32)__popcll(pm & lt)] = wv;
        tail += (u32)__popcll(pm);
      }
      head += cnt;
      __syncthreads();
    }
    for (u32 i = lane; i < tail; i += 64) st[queue[i]] |= GONE;
    __syncthreads();
    return tail;
  };
  // marks `bit` on what `src` reaches over `mask` among the transactions left that carry `need`; the queue then lists them; returns how many
  auto search = [&](const u32 *o, const u32 *a, const u32 mask, const u32 src, const u32 need, const u32 bit) -> u32 {
    if (lane == 0) { queue[0] = src; st[src] |= bit; }
    __syncthreads();
    u32 head = 0, tail = 1;
    while (head < tail) {
      const u32 cnt = min(64u, tail - head);
      const bool on = lane < cnt;
      const u32 v = on ? queue[head + lane] : 0u;
      const u32 a0 = on ? o[v] : 0u, a1 = on ? o[v + 1] : 0u;
      for (u32 k = 0; __ballot(a0 + k < a1); k++) {
        bool push = false; u32 wv = 0;
        if (a0 + k < a1) {
          const u32 x = a[a0 + k]; wv = x & E_TO;
          if ((x >> 28) & mask) { const u32 s = st[wv]; if (!(s & (GONE | bit)) && (s & need) == need) push = !(atomicOr(&st[wv], bit) & bit); }
        }
        const u64 pm = __ballot(push);
        if (push) queue[tail + (u32)__popcll(pm & lt)] = wv;
        tail += (u32)__popcll(pm);
      }
      head += cnt;
      __syncthreads();
    }
    return tail;
  };
  // A component beyond the matrix, listed in queue[0 .. s) and marked BWD: is there a rw edge u -> v in it whose v reaches u over the other
  // kinds of `mask`?  The worklist is a ring of s slots in `deg` (free between two peels): QUEUED keeps a transaction from being in it
  // twice, so it never holds more than the component.  A transaction is taken (mark cleared, word read) before anything is pushed in
  // that step, so bits that reach it afterwards queue it again.  Cost: typically about (heads / 64) x the component's edges; a transaction
  // is taken once per time its word gained bits, at most 64 times per batch, so the bound is 64 x the edges per batch = heads x edges.
  // Returns NONE if there is none; EXPLAIN: else the smallest such v (the heads are then numbered by transaction index, so the first batch
  // with a hit holds it).
  auto single_by_search = [&](const u32 mask, const u32 s) -> u32 {
    u32 *const wl = deg;
    u32 heads = 0;   // the heads, numbered along the list: jump[v] = its number (NONE: no rw edge of the component enters v)
    if constexpr (EXPLAIN) {
      for (u32 base = 0; base < n; base += 64) {
        const u32 v = base + lane;
        const bool mem = v < n && (st[v] & BWD);
        bool h = false;
        if (mem) for (u32 e = roff[v]; e < roff[v + 1] && !h; e++) { const u32 x = radj[e], u = x & E_TO; h = ((x >> 28) & E_RW) && u != v && (st[u] & BWD); }
        const u64 hm = __ballot(h);
        if (mem) jump[v] = h ? heads + (u32)__popcll(hm & lt) : NONE;
        heads += (u32)__popcll(hm);
      }
    } else
    for (u32 base = 0; base < s; base += 64) {
      const u32 i = base + lane;
      bool h = false; u32 v = 0;
      if (i < s) {
        v = queue[i];
        for (u32 e = roff[v]; e < roff[v + 1] && !h; e++) { const u32 x = radj[e], u = x & E_TO; h = ((x >> 28) & E_RW) && u != v && (st[u] & BWD); }
      }
      const u64 hm = __ballot(h);
      if (i < s) jump[v] = h ? heads + (u32)__popcll(hm & lt) : NONE;
      heads += (u32)__popcll(hm);
    }
    __syncthreads();
    for (u32 b = 0; b * 64u < heads; b++) {
      u32 hd = 0, cnt = 0;   // the ring: first slot taken, slots taken
      for (u32 base = 0; base < s; base += 64) {   // the words cleared, this batch's heads seeded and queued (64 of them at the most)
        const u32 i = base + lane;
        bool sd = false; u32 v = 0;
        if (i < s) {
          v = queue[i];
          const u32 o = jump[v];
          sd = (o >> 6) == b;
          reach[v] = sd ? 1ull << (o & 63u) : 0ull;
          if (sd) st[v] |= QUEUED;
        }
        const u64 sm = __ballot(sd);
        if (sd) wl[cnt + (u32)__popcll(sm & lt)] = v;
        cnt += (u32)__popcll(sm);
      }
      __syncthreads();
      while (cnt) {
        const u32 take = min(64u, cnt);
        const bool on = lane < take;
        u32 v = 0; u64 rv = 0;
        if (on) { u32 q = hd + lane; if (q >= s) q -= s; v = wl[q]; st[v] &= ~QUEUED; rv = reach[v]; }
        hd += take; if (hd >= s) hd -= s;
        cnt -= take;
        __syncthreads();
        const u32 a0 = on ? off[v] : 0u, a1 = on ? off[v + 1] : 0u;
        for (u32 k = 0; __ballot(a0 + k < a1); k++) {
          bool push = false; u32 wv = 0;
          if (a0 + k < a1) {
            const u32 x = adj[a0 + k]; wv = x & E_TO;
            if (((x >> 28) & mask & ~E_RW) && (st[wv] & BWD) && (rv & ~reach[wv]))
              if (rv & ~(u64)atomicOr(reinterpret_cast<unsigned long long *>(&reach[wv]), (unsigned long long)rv)) push = !(atomicOr(&st[wv], QUEUED) & QUEUED);
          }
          const u64 pm = __ballot(push);
          if (push) { u32 q = hd + cnt + (u32)__popcll(pm & lt); if (q >= s) q -= s; wl[q] = wv; }   // (cnt + pushes <= s: QUEUED)
          cnt += (u32)__popcll(pm);
        }
        __syncthreads();
      }
      bool hit = false; u32 hv = NONE;
      for (u32 i = lane; i < s; i += 64) {
        const u32 u = queue[i];
        const u64 ru = reach[u];
        for (u32 e = off[u]; e < off[u + 1]; e++) {
          const u32 x = adj[e], w = x & E_TO;
          if (((x >> 28) & E_RW) && w != u && (st[w] & BWD)) {
            const u32 o = jump[w];
            const bool r = (o >> 6) == b && ((ru >> (o & 63u)) & 1ull) != 0;
            hit |= r;
            if constexpr (EXPLAIN) { if (r) hv = min(hv, w); }
          }
        }
      }
      if (__ballot(hit)) { if constexpr (EXPLAIN) return wv_min(hv); else return 0u; }
      __syncthreads();
    }
    return NONE;
  };
  // the transactions in components of more than one transaction over `mask`; want_single: is there, in one of them, a rw edge u -> v
  // whose v reaches u without a rw edge (single)?  over: a component beyond the matrix that is left to the host
  bool single = false, over = false;
  u32 cmin = NONE, shead = NONE;   // EXPLAIN: the smallest member of a component so far; the smallest head of a closing rw edge so far
  auto components = [&](const u32 mask, const bool want_single) -> u32 {
    reset();
    u32 left = n - peel(off, adj, roff, radj, mask);
    if (left) left -= peel(roff, radj, off, adj, mask);
    u32 cyc = 0;
    while (left) {
      for (u32 t = lane; t < n; t += 64) {   // one predecessor each (there is one: the peel is done)
        if (st[t] & GONE) continue;
        u32 pr = t;
        for (u32 e = roff[t]; e < roff[t + 1]; e++) { const u32 x = radj[e]; if (((x >> 28) & mask) && !(st[x & E_TO] & GONE)) { pr = x & E_TO; break; } }
        jump[t] = pr;
      }
      __syncthreads();
      for (u32 r = 1; r < left; r <<= 1) {   // after these rounds jump[t] is at least `left` predecessors back: past every tail, on a cycle
        for (u32 t = lane; t < n; t += 64) if (!(st[t] & GONE)) jump[t] = jump[jump[t]];
        __syncthreads();
      }
      u32 pivot = NONE;
      for (u32 base = 0; base < n && pivot == NONE; base += 64) {
        const u32 t = base + lane;
        const u64 m = __ballot(t < n && !(st[t] & GONE));
        if (m) pivot = jump[base + (u32)__builtin_ctzll(m)];
      }
      if (pivot == NONE) break;
      (void)search(off, adj, mask, pivot, 0u, FWD);
      const u32 s = search(roff, radj, mask, pivot, FWD, BWD);   // the queue now lists the pivot's component
      cyc += s;
      if constexpr (EXPLAIN) { u32 m = NONE; for (u32 i = lane; i < s; i += 64) m = min(m, queue[i]); cmin = min(cmin, wv_min(m)); }
      if (want_single && (EXPLAIN || !single) && !over) {
        if (s > p.ccap) {
          if (p.big) { const u32 h = single_by_search(mask, s); if constexpr (EXPLAIN) { single |= h != NONE; shead = min(shead, h); } else single = h != NONE; }
          else over = true;
        }
        else {
          const u32 W = (s + 63u) >> 6;
          for (u32 i = lane; i < s; i += 64) jump[queue[i]] = i;
          for (u32 i = lane; i < s * W; i += 64) mat[i] = 0;
          __syncthreads();
          for (u32 i = lane; i < s; i += 64) {   // lane = a row
            const u32 u = queue[i];
            for (u32 e = off[u]; e < off[u + 1]; e++) {
              const u32 x = adj[e], w = x & E_TO;
              if (((x >> 28) & mask & ~E_RW) && (st[w] & BWD)) mat[i * W + (jump[w] >> 6)] |= 1ull << (jump[w] & 63u);
            }
          }
          __syncthreads();
          for (u32 k = 0; k < s; k++) {
            for (u32 i = lane; i < s; i += 64)
              if ((mat[i * W + (k >> 6)] >> (k & 63u)) & 1ull) for (u32 w = 0; w < W; w++) mat[i * W + w] |= mat[k * W + w];
            __syncthreads();
          }
          bool hit = false; u32 hv = NONE;
          for (u32 i = lane; i < s; i += 64) {
            const u32 u = queue[i];
            for (u32 e = off[u]; e < off[u + 1]; e++) {
              const u32 x = adj[e], w = x & E_TO;
              if (((x >> 28) & E_RW) && w != u && (st[w] & BWD)) {
                const bool r = ((mat[jump[w] * W + (i >> 6)] >> (i & 63u)) & 1ull) != 0;
                hit |= r;
                if constexpr (EXPLAIN) { if (r) hv = min(hv, w); }
              }
            }
          }
          if (__ballot(hit)) { single = true; if constexpr (EXPLAIN) shead = min(shead, wv_min(hv)); }
        }
      }
      for (u32 i = lane; i < s; i += 64) st[queue[i]] = GONE;
      __syncthreads();
      for (u32 t = lane; t < n; t += 64) st[t] &= GONE;
      __syncthreads();
      left -= s;
      if (left) left -= peel(off, adj, roff, radj, mask);
      if (left) left -= peel(roff, radj, off, adj, mask);
    }
    return cyc;
  };
  // EXPLAIN: the witness cycle of class `cls` (+ the realtime edges: x) into cw's record and steps; deg holds the BFS distances
  [[maybe_unused]] auto witness = [&](const u32 cls, const u32 x, const u32 all_bits) {
    const bool sg = cls == MSIM_ANOMALY_G_SINGLE;
    const u32 K = (cls == MSIM_ANOMALY_G0 ? E_WW : cls == MSIM_ANOMALY_G2 ? (E_WW | E_WR | E_RW) : (E_WW | E_WR)) | x;   // (G-single: the path's kinds)
    if (!sg && cls != MSIM_ANOMALY_G2) { cmin = NONE; (void)components(K, false); }
    const u32 start = sg ? shead : cmin;
    if (start == NONE) return;
    u32 *const d = deg;
    for (u32 t = lane; t < n; t += 64) d[t] = NONE;
    __syncthreads();
    if (lane == 0) { queue[0] = start; d[start] = 0; }
    __syncthreads();
    u32 lo = 0, hi = 1, tail = 1;
    for (u32 level = 0; lo < hi; level++) {   // queue[lo .. hi) is the level; what it reaches first is the next one
      for (u32 base = lo; base < hi; base += 64) {
        const bool on = base + lane < hi;
        const u32 v = on ? queue[base + lane] : 0u;
        const u32 a0 = on ? off[v] : 0u, a1 = on ? off[v + 1] : 0u;
        for (u32 k = 0; __ballot(a0 + k < a1); k++) {
          bool push = false; u32 wv = 0;
          if (a0 + k < a1) {
            const u32 e = adj[a0 + k]; wv = e & E_TO;
            if (((e >> 28) & K) && d[wv] == NONE) push = atomicCAS(&d[wv], NONE, level + 1u) == NONE;
          }
          const u64 pm = __ballot(push);
          if (push) queue[tail + (u32)__popcll(pm & lt)] = wv;
          tail += (u32)__popcll(pm);
        }
      }
      __syncthreads();
      lo = hi; hi = tail;
    }
    const u32 close = sg ? E_RW : K;
    u64 best = ~0ull;   // distance << 32 | transaction
    for (u32 e = roff[start] + lane; e < roff[start + 1]; e += 64) {
      const u32 xe = radj[e], u = xe & E_TO;
      if (((xe >> 28) & close) && d[u] != NONE) best = min(best, ((u64)d[u] << 32) | u);
    }
    best = cw_min64(best);
    if (best == ~0ull) return;
    const u32 L = (u32)(best >> 32);
    msim_cycle_step *const steps = cw->steps + (u64)hist * cw->max_steps;
    u32 src = (u32)best, cur = start;   // the step src -> cur is the cycle's step i
    for (u32 i = L;; i--) {
      u32 kk = 0;
      for (u32 e = roff[cur] + lane; e < roff[cur + 1]; e += 64) { const u32 xe = radj[e]; if ((xe & E_TO) == src) kk |= xe >> 28; }
      kk = (sg && i == L) ? E_RW : (wv_or(kk) & K);
      if (lane == 0 && i < cw->max_steps) { msim_cycle_step sp; sp.txn = src; sp.inv_row = cw->t_inv[src]; sp.cmp_row = cw->t_cmp[src]; sp.kinds = kk; steps[i] = sp; }
      if (i == 0) break;
      u32 pw = NONE;   // the smallest predecessor one level up
      for (u32 e = roff[src] + lane; e < roff[src + 1]; e += 64) { const u32 xe = radj[e], f = xe & E_TO; if (((xe >> 28) & K) && d[f] == i - 1u) pw = min(pw, f); }
      pw = wv_min(pw);
      if (pw == NONE) return;   // (there is one: the distance came along such an edge)
      cur = src; src = pw;
    }
    if (lane == 0) {
      msim_cycle_result c; c.anomalies = all_bits; c.length = L + 1u; c.n_steps = min(L + 1u, cw->max_steps); c.reserved = 0;
      cw->cycles[hist] = c;
    }
  };

  u32 bits = 0, cyc = 0;
  reset();
  if (peel(off, adj, roff, radj, E_WW | E_WR | E_RW | E_RT) != n) {   // else acyclic over every edge kind (the common case elsewhere): nothing to classify
    for (u32 x = 0; x <= E_RT && !bits; x += E_RT) {   // the dependency edges alone first; with the realtime edges only if that finds nothing
      if (x == 0) { reset(); if (peel(off, adj, roff, radj, E_WW | E_WR | E_RW) == n) continue; }
      reset();
      u32 cls = 0;
      if (peel(off, adj, roff, radj, E_WW | x) != n) cls = MSIM_ANOMALY_G0;
      else { reset(); if (peel(off, adj, roff, radj, E_WW | E_WR | x) != n) cls = MSIM_ANOMALY_G1C; }
      cyc = components(E_WW | E_WR | E_RW | x, cls == 0);
      if (over) { if (lane == 0) p.out[hist] = res; return; }   // (res.valid is NEEDS_HOST)
      if (!cls) cls = single ? MSIM_ANOMALY_G_SINGLE : MSIM_ANOMALY_G2;
      bits = cls | (x ? MSIM_ANOMALY_REALTIME : 0u);
      if constexpr (EXPLAIN) witness(cls, x, bits);
    }
  }
  if (lane == 0) {
    const u32 all = anomalies | bits;
    const u32 cycles = MSIM_ANOMALY_G0 | MSIM_ANOMALY_G1C | MSIM_ANOMALY_G_SINGLE | MSIM_ANOMALY_G2;
    u32 judged = all;   // judge(): cycles that need a realtime edge count under strict-serializable only
    if ((judged & MSIM_ANOMALY_REALTIME) && p.cm != MSIM_CM_STRICT_SERIALIZABLE) judged &= ~(cycles | MSIM_ANOMALY_REALTIME);
    res.lost_count = n_edges; res.stale_count = cyc; res.error_count = all;
    res.valid = flags ? 0u : (judged & p.proscribed) ? 0u : (c_ok == 0 ? 2u : 1u);
    p.out[hist] = res;
  }
}
