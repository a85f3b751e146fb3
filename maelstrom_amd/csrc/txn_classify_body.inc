// txn_classify_body.inc — the body of txn_classify_kernel and txn_explain_kernel (txn_check_dev.hip, which describes the analysis above
// the two kernels), included once into each: `p` is the kernel's TParams, EXPLAIN a constant the including kernel defines.  EXPLAIN
// (txn_explain_kernel): the same record, and the witness cycle of its cycle class (cycle_classify.inc); the workspace then keeps every
// transaction's :invoke row as well (t_inv, behind the reversed edges).  A body included into the two kernels, not a function of its
// own: as a function it compiled txn_classify_kernel to other code than it had (61 for 63 vector registers, 65 more instructions).
// FINDINGS (txn_findings_kernel; a constant of the including kernel as EXPLAIN is): where passes D and E OR a non-cycle bit they also
// emit a record into the history's region behind t_inv (txn_findings.inc), sorted and written out before the cycles are classified.
  const u32 lane = threadIdx.x, hist = p.list[p.first + blockIdx.x];
  const u64 lt = (1ull << lane) - 1ull;
  HIST_VIEW(p, hist);
  const u32 NM = p.nmax;
  u32 *const ws = p.ws + (u64)blockIdx.x * p.ws_words;   // (ws_words is even and the workspace 256-byte aligned: the 64-bit tables come first)
  u64 *const long64 = reinterpret_cast<u64 *>(ws);            // [KMAX] (len + 1) << 40 | inverted transaction << 16 | inverted micro-op
  u64 *const reach = long64 + KMAX;                           // [NM] cycle_classify's search of a component beyond the matrix
  u32 *const t_cmp = reinterpret_cast<u32 *>(reach + NM), *const t_off = t_cmp + NM, *const t_lt = t_off + NM;   // t_lt: words | type << 16
  u32 *const t_first = t_lt + NM;            // transactions invoked before this one's completion row (= index of the first one after it)
  u32 *const sm = t_first + NM;              // [NM + 1] suffix minimum of the :ok completions ...
  u32 *const smf = sm + NM + 1;              // [NM + 1] ... and t_first of the transaction that attains it
  u32 *const deg = smf + NM + 1, *const off = deg + NM;   // off [NM + 1]: out-degrees, then CSR offsets
  u32 *const cur = off + NM + 1, *const queue = cur + NM;
  u32 *const roff = queue + NM, *const rcur = roff + NM + 1, *const st = rcur + NM, *const jump = st + NM;   // roff [NM + 1]: in-degrees, then offsets
  u32 *const longest = jump + NM;            // [KMAX] (len + 1) << 24 | first payload word of the list
  u32 *const writer = longest + KMAX;        // [WMAX]
  u32 *const adj = writer + WMAX, *const radj = adj + p.emax;   // [emax] each
  [[maybe_unused]] u32 *const t_inv = radj + p.emax;          // [NM] EXPLAIN and FINDINGS only
  [[maybe_unused]] const FRegion F(t_inv + NM);               // FINDINGS only

  BLANK_RESULT(res, NEEDS_HOST);
#define TO_HOST() do { if (lane == 0) p.out[hist] = res; return; } while (0)
  if (n_words >= (1u << 24) || NM > 0xFFFFFFu) TO_HOST();
  if constexpr (FINDINGS) { if (lane == 0) *F.cnt = 0; __syncthreads(); }

  // ---- A: transactions ---------------------------------------------------------------------------------------------------------
  u32 n = 0, c_ok = 0, c_fail = 0, c_info = 0;
  {
    bool o_used = false; u32 o_proc = 0, o_txn = 0, o_len = 0; bool bad = false;   // txn_pairing.inc's open calls
    for (u32 base = 0; base < n_rows; base += 64) {
      const u32 idx = base + lane;
      uint4 row = make_uint4(0, 0, 0, 0);
      if (idx < n_rows) row = r[idx];
      const u32 type = row.z & 3u, f = (row.z >> 2) & 31u, proc = row.z >> 12, len = row.y >> 16, woff = row.w;
      const bool is = idx < n_rows && proc != MSIM_PROCESS_NEMESIS && f == MSIM_F_TXN;
      if (__ballot(is && (u64)woff + len > n_words)) { bad = true; break; }
      const bool inv = is && type == MSIM_T_INVOKE;
      const u64 im = __ballot(inv);
      const u32 my_t = n + (u32)__popcll(im & lt);
      if (n + (u32)__popcll(im) > NM) { bad = true; break; }
      if (inv) { t_cmp[my_t] = NONE; t_off[my_t] = woff; t_lt[my_t] = len | (MSIM_T_INFO << 16); t_first[my_t] = 0; if constexpr (EXPLAIN || FINDINGS) t_inv[my_t] = idx; }   // never completed = indeterminate
#include "txn_pairing.inc"
      if (bad) break;
      n += (u32)__popcll(im);
    }
    if (bad) TO_HOST();
  }
  __syncthreads();
  res.op_count = n; res.attempt_count = n; res.ok_count = c_ok; res.stable_count = c_ok; res.fail_count = c_fail; res.info_count = c_info;
#define TYPE(t_) (t_lt[t_] >> 16)

  // ---- B: ranges, and the tables cleared ------------------------------------------------------------------------------------------
  u32 max_key = 0, max_val = 0, anomalies = 0; bool bad = false;
  for (u32 t = lane; t < n; t += 64) {
    const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
    for (u32 i = 0; i < wn;) { const Mop m = next_mop(w, wn, i); bad |= m.bad; max_key = max(max_key, m.key); if (m.f) max_val = max(max_val, m.val); }
  }
  max_key = wv_max(max_key); max_val = wv_max(max_val);
  const u32 stride = max_val + 1u;
  if (__ballot(bad) || max_key >= KMAX || (u64)(max_key + 1u) * stride > WMAX) TO_HOST();
  for (u32 k = lane; k <= max_key; k += 64) { longest[k] = 0; long64[k] = 0; }
  for (u32 k = lane; k < (max_key + 1u) * stride; k += 64) writer[k] = NONE;
  for (u32 t = lane; t <= n; t += 64) { off[t] = 0; roff[t] = 0; if (t < n) { cur[t] = 0; rcur[t] = 0; } }
  __syncthreads();

  // ---- C: writers (every transaction, whatever became of it) -------------------------------------------------------------------------
  for (u32 t = lane; t < n; t += 64) {
    const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
    for (u32 i = 0; i < wn;) { const Mop m = next_mop(w, wn, i); if (m.f && atomicCAS(&writer[m.key * stride + m.val], NONE, t) != NONE) bad = true; }
  }
  __syncthreads();
  if (__ballot(bad)) TO_HOST();   // a (key, element) appended twice: the host's table is last-writer-wins in row order
#define WRITER(k_, el_) ((el_) < stride ? writer[(k_) * stride + (el_)] : NONE)

  // ---- D: the reads of :ok transactions ------------------------------------------------------------------------------------------------
  for (u32 t = lane; t < n; t += 64) {
    if (TYPE(t) != MSIM_T_OK) continue;
    const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
    u32 k = 0;
    for (u32 i = 0; i < wn; k++) {
      const Mop m = next_mop(w, wn, i);
      if (m.f) continue;
      { u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0;   // duplicates
        [[maybe_unused]] bool dup_told = false;
        for (u32 e = 0; e < m.len; e++) {
          const u32 x = elem(m.list, e); const u64 b = 1ull << (x & 63u); const u32 q = x >> 6;
          const u64 s = q == 0 ? s0 : q == 1 ? s1 : q == 2 ? s2 : s3;
          if (s & b) anomalies |= MSIM_ANOMALY_DUPLICATE_ELEMENTS;
          if constexpr (FINDINGS) if ((s & b) && !dup_told) {   // the lowest position that repeats an earlier one, and the lowest it repeats
            dup_told = true;
            u32 a = 0;
            while (elem(m.list, a) != x) a++;
            f_emit(F, F_DUPLICATE, m.key, t, t_inv[t], t_cmp[t], k, NONE, NONE, NONE, x, e, a);
          }
          s0 |= q == 0 ? b : 0; s1 |= q == 1 ? b : 0; s2 |= q == 2 ? b : 0; s3 |= q == 3 ? b : 0;
        } }
      { int prev = -1; Mop pm = m; u32 e_i = 0, e_k = 0;   // internal consistency: what the transaction's own earlier micro-ops imply for this read
        for (e_i = 0, e_k = 0; e_k < k; e_k++) { const Mop q = next_mop(w, wn, e_i); if (!q.f && q.key == m.key) { prev = (int)e_k; pm = q; } }
        const u32 e0 = prev < 0 ? 0u : (u32)prev + 1u;
        u32 n_app = 0;
        for (e_i = 0, e_k = 0; e_k < k; e_k++) { const Mop q = next_mop(w, wn, e_i); if (e_k >= e0 && q.f && q.key == m.key) n_app++; }
        bool ok = true; u32 at = 0;
        if (prev >= 0) { ok = m.len == pm.len + n_app; if (ok) for (u32 e = 0; e < pm.len; e++) ok &= elem(m.list, e) == elem(pm.list, e); at = pm.len; }
        else { ok = m.len >= n_app; at = m.len - n_app; }
        if (ok) { u32 a = 0; for (e_i = 0, e_k = 0; e_k < k; e_k++) { const Mop q = next_mop(w, wn, e_i); if (e_k >= e0 && q.f && q.key == m.key) { if (elem(m.list, at + a) != q.val) ok = false; a++; } } }
        if (!ok) anomalies |= MSIM_ANOMALY_INTERNAL;
        if constexpr (FINDINGS) if (!ok) {
          const bool pr = prev >= 0;
          f_emit(F, F_INTERNAL, m.key, t, t_inv[t], t_cmp[t], k, pr ? t_inv[t] : NONE, pr ? t_cmp[t] : NONE, pr ? (u32)prev : NONE, m.len, pr ? pm.len : NONE, n_app);
        } }
      u32 ext = m.len;   // the externally visible part: without the transaction's own appends at the tail
      while (ext > 0 && WRITER(m.key, elem(m.list, ext - 1)) == t) ext--;
      for (u32 e = 0; e < ext; e++) {
        const u32 wr = WRITER(m.key, elem(m.list, e));
        if (wr == NONE || TYPE(wr) == MSIM_T_FAIL) {
          anomalies |= MSIM_ANOMALY_G1A;
          if constexpr (FINDINGS) f_emit(F, F_G1A, m.key, t, t_inv[t], t_cmp[t], k, wr == NONE ? NONE : t_inv[wr], wr == NONE ? NONE : t_cmp[wr], NONE, elem(m.list, e), NONE, e);
        }
      }
      if (ext > 0) {   // G1b: the last visible element must be its writer's last append to the key
        const u32 last = elem(m.list, ext - 1), wr = WRITER(m.key, last);
        if (wr != NONE && wr != t) {
          const u32 *w2 = pay + t_off[wr]; const u32 wn2 = t_lt[wr] & 0xFFFFu; u32 fin = NONE;
          for (u32 i2 = 0; i2 < wn2;) { const Mop q = next_mop(w2, wn2, i2); if (q.f && q.key == m.key) fin = q.val; }
          if (fin != last) anomalies |= MSIM_ANOMALY_G1B;
          if constexpr (FINDINGS) if (fin != last) {
            u32 fin_k = NONE, k2 = 0;   // the micro-op of that last append
            for (u32 i2 = 0; i2 < wn2; k2++) { const Mop q = next_mop(w2, wn2, i2); if (q.f && q.key == m.key) fin_k = k2; }
            f_emit(F, F_G1B, m.key, t, t_inv[t], t_cmp[t], k, t_inv[wr], t_cmp[wr], fin_k, last, fin, ext - 1u);
          }
        }
      }
      // the key's longest read; among equals the first in (transaction, micro-op) order
      atomicMax(reinterpret_cast<unsigned long long *>(&long64[m.key]),
                (unsigned long long)(((u64)(m.len + 1u) << 40) | ((u64)(0xFFFFFFu - t) << 16) | (u64)(0xFFFFu - (k & 0xFFFFu))));
    }
  }
  __syncthreads();
  for (u32 key = lane; key <= max_key; key += 64) {   // the winner's list (lane = key)
    const u64 L = long64[key];
    if (!L) continue;
    const u32 t = 0xFFFFFFu - (u32)((L >> 16) & 0xFFFFFFu), k = 0xFFFFu - (u32)(L & 0xFFFFu);
    const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
    u32 i = 0; Mop m = next_mop(w, wn, i);
    for (u32 e_k = 0; e_k < k && i < wn; e_k++) m = next_mop(w, wn, i);
    longest[key] = ((m.len + 1u) << 24) | (u32)(m.list - pay);
  }

#include "txn_realtime.inc"
  __syncthreads();

  // ---- E: edges: pass 0 counts degrees, pass 1 fills the CSR and its reverse ------------------------------------------------------------
  u32 n_edges = 0;
  for (int pass = 0; pass < 2; pass++) {
    u32 my_edges = 0;
#define ADD(a_, b_, kind_) do { const u32 ea = (a_), eb = (b_); if (ea != eb) { if (pass == 0) { atomicAdd(&off[ea], 1u); atomicAdd(&roff[eb], 1u); my_edges++; } \
      else { adj[off[ea] + atomicAdd(&cur[ea], 1u)] = eb | ((kind_) << 28); radj[roff[eb] + atomicAdd(&rcur[eb], 1u)] = ea | ((kind_) << 28); } } } while (0)
    for (u32 key = lane; key <= max_key; key += 64) {   // ww along each key's version order (lane = key)
      const u32 L = longest[key];
      if (L == 0) continue;
      const u32 len = (L >> 24) - 1u; const u32 *ord = pay + (L & 0xFFFFFFu);
      for (u32 i = 0; i + 1 < len; i++) {
        const u32 a = WRITER(key, elem(ord, i)), b = WRITER(key, elem(ord, i + 1));
        if (a == NONE || b == NONE) continue;
        const bool fa = TYPE(a) == MSIM_T_FAIL, fb = TYPE(b) == MSIM_T_FAIL;
        if (fa && !fb) anomalies |= MSIM_ANOMALY_DIRTY_UPDATE;
        if constexpr (FINDINGS) if (fa && !fb && pass == 0) f_emit(F, F_DIRTY, key, b, t_inv[b], t_cmp[b], NONE, t_inv[a], t_cmp[a], NONE, elem(ord, i + 1), elem(ord, i), i);
        if (!fa && !fb) ADD(a, b, E_WW);
      }
    }
    for (u32 t = lane; t < n; t += 64) {   // wr / rw per read of an :ok transaction; its realtime successors
      if (TYPE(t) != MSIM_T_OK) continue;
      const u32 *w = pay + t_off[t]; const u32 wn = t_lt[t] & 0xFFFFu;
      for ([[maybe_unused]] u32 i = 0, k = 0; i < wn; k++) {
        const Mop m = next_mop(w, wn, i);
        if (m.f) continue;
        const u32 L = longest[m.key];
        if (L == 0) continue;   // (an :ok read always left one)
        const u32 llen = (L >> 24) - 1u; const u32 *ord = pay + (L & 0xFFFFFFu);
        bool pre = m.len <= llen;
        if (pre) for (u32 e = 0; e < m.len; e++) pre &= elem(m.list, e) == elem(ord, e);
        if constexpr (FINDINGS) if (!pre && pass == 0) {   // against longest(k): where the two lists part
          const u64 L64 = long64[m.key];
          const u32 lt_ = 0xFFFFFFu - (u32)((L64 >> 16) & 0xFFFFFFu), lk = 0xFFFFu - (u32)(L64 & 0xFFFFu);
          u32 d = 0;
          while (d < m.len && d < llen && elem(m.list, d) == elem(ord, d)) d++;
          f_emit(F, F_ORDER, m.key, t, t_inv[t], t_cmp[t], k, t_inv[lt_], t_cmp[lt_], lk, elem(m.list, d), d < llen ? elem(ord, d) : NONE, d);
        }
        if (!pre) { anomalies |= MSIM_ANOMALY_INCOMPATIBLE_ORDER; continue; }
        u32 ext = m.len;
        while (ext > 0 && WRITER(m.key, elem(m.list, ext - 1)) == t) ext--;
        if (ext > 0) { const u32 wr = WRITER(m.key, elem(m.list, ext - 1)); if (wr != NONE && TYPE(wr) != MSIM_T_FAIL) ADD(wr, t, E_WR); }
        if (m.len < llen) { const u32 wr = WRITER(m.key, elem(ord, m.len)); if (wr != NONE && TYPE(wr) != MSIM_T_FAIL) ADD(t, wr, E_RW); }   // anti-dependency
      }
      const u32 first = t_first[t];                          // the transactions invoked after t completed start here ...
      const u32 last = sm[first] == NONE ? n : smf[first];   // ... and end where the first of them to complete :ok did
      for (u32 v = first; v < last; v++) if (TYPE(v) != MSIM_T_FAIL) ADD(t, v, E_RT);
    }
#undef ADD
    __syncthreads();
    if (pass == 0) {
      n_edges = wv_sum(my_edges);
      if (n_edges > p.emax) TO_HOST();
      for (int which = 0; which < 2; which++) {   // out-degrees / in-degrees -> offsets (exclusive prefix sums, 64 at a time)
        u32 *const o = which ? roff : off;
        u32 carry = 0;
        for (u32 base = 0; base <= n; base += 64) {
          const u32 t = base + lane;
          const u32 d = t < n ? o[t] : 0u;
          const u32 ex = wv_excl_scan(d, lane);
          if (t <= n) o[t] = carry + ex;
          carry += wv_sum(d);
        }
      }
      __syncthreads();
    }
  }
  anomalies = wv_or(anomalies);
  if constexpr (FINDINGS) { if (!f_finish(F, FOut{p.fhdr, p.frecs, p.max_findings}, hist)) TO_HOST(); }   // (more than the region holds: the host walk's)
  const CycleParams cp = {p.out, p.cm, p.proscribed, p.ccap, p.big};
  if constexpr (EXPLAIN) {
    const CycleWitness cw = {p.cycles, p.steps, p.max_steps, t_inv, t_cmp};
    cycle_classify<true>(cp, hist, res, anomalies, n, n_edges, flags, c_ok, deg, off, adj, roff, radj, st, jump, queue, reach, &cw);
  } else cycle_classify(cp, hist, res, anomalies, n, n_edges, flags, c_ok, deg, off, adj, roff, radj, st, jump, queue, reach);
#undef TO_HOST
#undef WRITER
#undef TYPE
