// pn_body.inc — the body of pn_check_kernel and pn_explain_kernel (pn_check_dev.hip, whose head describes the bitmap): included inside a
// kernel that has `rows_all`, `meta`, `out`, `max_rows`, `const PnExplainOut x` and `constexpr bool EXPLAIN`.  EXPLAIN adds the final
// reads and the ranges of msim_explain_pn* behind the verdict; without it nothing of `x` is read and the text is pn_check_kernel's.
  __shared__ int deltas[MAX_INFO];
  __shared__ u64 bits[64];
  __shared__ u32 n_info_s;
  const u32 lane = threadIdx.x, hist = blockIdx.x;
  const uint4 *const r = reinterpret_cast<const uint4 *>(rows_all) + (u64)hist * max_rows;
  const u32 n = meta[hist].n_rows, flags = meta[hist].flags;
  if (lane == 0) n_info_s = 0;
  __syncthreads();

  u32 c_inv = 0, c_ok = 0, c_fail = 0, c_info = 0;
  s64 definite = 0, neg = 0, pos = 0;
  for (u32 base = 0; base < n; base += 64) {
    const u32 idx = base + lane;
    if (idx >= n) continue;
    const uint4 row = r[idx];
    const u32 type = row.z & 3u, f = (row.z >> 2) & 31u, proc = row.z >> 12;
    if (proc == MSIM_PROCESS_NEMESIS) continue;
    c_inv += type == MSIM_T_INVOKE; c_ok += type == MSIM_T_OK; c_fail += type == MSIM_T_FAIL; c_info += type == MSIM_T_INFO;
    if (f != MSIM_F_ADD) continue;
    const int d = (int)row.w;
    if (type == MSIM_T_OK) definite += d;
    if (type == MSIM_T_INFO) {
      if (d < 0) neg += d; else pos += d;
      const u32 k = atomicAdd(&n_info_s, 1u);
      if (k < MAX_INFO) deltas[k] = d;
    }
  }
  __syncthreads();
  definite = p_sum64(definite); neg = p_sum64(neg); pos = p_sum64(pos);
  c_inv = wv_sum(c_inv); c_ok = wv_sum(c_ok); c_fail = wv_sum(c_fail); c_info = wv_sum(c_info);
  const u32 n_info = n_info_s;
  BLANK_RESULT(o, NEEDS_HOST);
  o.op_count = c_inv; o.ok_count = c_ok; o.fail_count = c_fail; o.info_count = c_info;
  if (n_info > MAX_INFO || pos - neg >= 4096) { if (lane == 0) out[hist] = o; return; }   // (EXPLAIN: the host walk writes this history's header and records)

  // the acceptable set: bit b of the 4096-bit map (word `lane`) <=> value lo_v + b
  const s64 lo_v = definite + neg;
  u64 B = 0;
  { const u32 b0 = (u32)(-neg); if ((b0 >> 6) == lane) B = 1ull << (b0 & 63u); }
  for (u32 k = 0; k < n_info; k++) {   // (any order: the set of subset sums does not depend on it)
    const int d = deltas[k];
    if (d == 0) continue;
    const u32 s = (u32)(d < 0 ? -d : d), q = s >> 6, rr = s & 63u;
    u64 sh;
    if (d > 0) {   // towards higher values: word w takes from words w - q and w - q - 1
      const u64 a = p_get64(B, (int)lane - (int)q), b = p_get64(B, (int)lane - (int)q - 1);
      sh = rr ? ((a << rr) | (b >> (64u - rr))) : a;
    } else {
      const u64 a = p_get64(B, (int)lane + (int)q), b = p_get64(B, (int)lane + (int)q + 1);
      sh = rr ? ((a >> rr) | (b << (64u - rr))) : a;
    }
    B |= sh;
  }
  bits[lane] = B;
  __syncthreads();
  // ranges = maximal runs of ones
  { const u64 prev_top = p_get64(B, (int)lane - 1) >> 63; o.stable_count = wv_sum((u32)__popcll(B & ~((B << 1) | prev_top))); }
  // final reads that completed :ok must lie in the set
  auto in_set = [&](const u32 value) {
    const s64 rel = (s64)(int)value - lo_v;
    return rel >= 0 && rel < 4096 && ((bits[(u32)rel >> 6] >> ((u32)rel & 63u)) & 1ull);
  };
  u32 attempts = 0, errors = 0;
  for (u32 base = 0; base < n; base += 64) {
    const u32 idx = base + lane;
    if (idx >= n) continue;
    const uint4 row = r[idx];
    if ((row.z >> 12) == MSIM_PROCESS_NEMESIS || !((row.z >> 11) & 1u) || (row.z & 3u) != MSIM_T_OK) continue;
    attempts++;
    errors += in_set(row.w) ? 0u : 1u;
  }
  attempts = wv_sum(attempts); errors = wv_sum(errors);
  if constexpr (EXPLAIN) {
    // the final reads compacted in row order, 64 rows per step: a ballot ranks a read among the step's, on top of the reads before
    const u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes below this one
    uint4 *const rec = x.records + (u64)hist * x.max_records;
    const u32 w_reads = min(attempts, x.max_records);
    u32 at = 0;
    for (u32 base = 0; base < n && at < w_reads; base += 64) {
      const u32 idx = base + lane;
      const uint4 row = idx < n ? r[idx] : make_uint4(0, 0, 0, 0);
      const bool fr = idx < n && (row.z >> 12) != MSIM_PROCESS_NEMESIS && ((row.z >> 11) & 1u) && (row.z & 3u) == MSIM_T_OK;
      const u64 m = __ballot(fr);
      const u32 slot = at + (u32)__popcll(m & lt);
      if (fr && slot < w_reads) rec[slot] = make_uint4(idx, row.w, row.z >> 12, in_set(row.w) ? 1u : 0u);   // (slot < max_records: the slab's bound)
      at += (u32)__popcll(m);
    }
    // the ranges behind them, in the room they left: a run starts at a one with a zero below it and ends at a one with a zero above it
    // (the bit below / above a word's edge comes from the neighbouring lane); the k-th start and the k-th end are one range, and a
    // prefix sum over the lanes' counts gives every lane the k of its first start and of its first end
    const u32 room = x.max_records - w_reads;
    const u64 prev_top = p_get64(B, (int)lane - 1) >> 63, next_bottom = p_get64(B, (int)lane + 1) & 1ull;
    u64 S = B & ~((B << 1) | prev_top), E = B & ~((B >> 1) | (next_bottom << 63));
    u32 ks = wv_excl_scan((u32)__popcll(S), lane), ke = wv_excl_scan((u32)__popcll(E), lane);
    s64 *const g = reinterpret_cast<s64 *>(rec + w_reads);
    for (; S; S &= S - 1, ks++) if (ks < room) g[2 * ks] = lo_v + (s64)(lane * 64u + (u32)__builtin_ctzll(S));
    for (; E; E &= E - 1, ke++) if (ke < room) g[2 * ke + 1] = lo_v + (s64)(lane * 64u + (u32)__builtin_ctzll(E));
    if (lane == 0) {
      msim_pn_explain h;
      h.n_reads = w_reads; h.n_ranges = min(o.stable_count, room);
      h.truncated = (w_reads < attempts || h.n_ranges < o.stable_count) ? 1u : 0u;
      h.reserved = 0; h.definite_sum = definite;
      x.hdr[hist] = h;
    }
  }
  if (lane == 0) {
    o.attempt_count = attempts; o.error_count = errors;
    o.valid = flags ? 0u : (errors == 0 ? 1u : 0u);
    out[hist] = o;
  }
