// set_full_body.inc — the body of check_kernel and set_explain_kernel (checker.hip, whose head describes the two passes): included
// inside a kernel that has `const CParams p`, `const SetExplainOut x` and `constexpr bool EXPLAIN`.  EXPLAIN adds the element records
// and the header of msim_explain_set_full* behind the outcomes; without it nothing of `x` is read and the text is check_kernel's.
  extern __shared__ __attribute__((aligned(16))) unsigned char csmem[];
  typedef unsigned short u16;
  u16 *const known = reinterpret_cast<u16 *>(csmem);
  u16 *const lp_idx = known + p.max_values;
  u16 *const la_idx = lp_idx + p.max_values;
  u32 *const lat = reinterpret_cast<u32 *>(EXPLAIN ? csmem + x.off_lat : csmem);  // reused after the walk: stable latency per element (needs 4 B each); EXPLAIN: a region of its own, the row indices are kept
  u32 *const llat = lat + p.max_values;  // EXPLAIN: the lost latency per element
  (void)llat;
  u32 *const valid = reinterpret_cast<u32 *>(csmem + p.off_valid);  // bitmap over invocation ranks: read completed :ok
  u32 *const slot = reinterpret_cast<u32 *>(csmem + p.off_tbl);     // [C] the worker thread's pending invocation: row | rank << 16 (echo: row)
  u32 *const first = slot + p.C;                                     // [C] ds_min target: (round, lane) of the thread's earliest pending row
  u32 *const slotv = first + p.C;                                    // [C] echo: the :value of the thread's last invocation

  const u32 lane = threadIdx.x, inst = blockIdx.x;
  const msim_inst_meta meta = p.meta[inst];
  const uint4 *const rows = reinterpret_cast<const uint4 *>(p.rows + (size_t)inst * p.max_rows);
  const u32 *const pay = p.payload + (size_t)inst * p.max_pay;
  u32 *const rec = p.recs + (size_t)inst * p.max_reads * 3;
  const u32 n_rows = meta.n_rows, C = p.C;
  const bool setfull = p.workload != MSIM_WL_ECHO;
  const u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes below this one

  for (u32 i = lane; i < p.max_values; i += 64) { known[i] = NONE; lp_idx[i] = NONE; la_idx[i] = NONE; }
  for (u32 i = lane; i < (p.max_reads + 31) / 32 + 2; i += 64) valid[i] = 0;
  for (u32 i = lane; i < C; i += 64) { slot[i] = NONE32; first[i] = 0xFFFFFFFFu; slotv[i] = 0; }
  __syncthreads();

  u32 v_cur = 0, n_ri = 0, errors = 0;
#ifdef CK_PROF   // developer build (tools/check_prof_report.py): cycles of pass 1 / pass 2 / the rest in stable_latency_ms[0..2], pairing rounds in [3], reads in [4]
  const u64 ck_t0 = __builtin_readcyclecounter(); u64 ck_t1 = 0, ck_t2 = 0; u32 ck_rounds = 0;
#endif
  u32 cnt_lo = 0, cnt_hi = 0;    // per lane: rows of type :invoke | :ok << 16, :fail | :info << 16 (summed over the wavefront at the end)
  u32 round_key = 0x3FFFFFFu;    // decreases with every pairing round: a later round's ds_min beats whatever an earlier one left

  // ---- pass 1 ----
  // Four chunks of rows (4 KiB) are in flight: with one, a chunk's 150 instructions waited out an HBM round trip each time (round 6: pass 1 took
  // 1.7e5 cycles per history, 2700 per chunk).  The buffers keep their registers — a rotation by moves would wait for the load just issued —
  // and the loads are unconditional (past the end: the last row again; every use of a row is behind `lane < cnt`).
  auto ldrow = [&](u32 b) -> uint4 { return rows[min(b + lane, n_rows ? n_rows - 1 : 0u)]; };
  auto rowchunk = [&](const u32 base, const uint4 r) {
    const u32 cnt = min(64u, n_rows - base);
    const u32 my_type = r.z & 3, my_f = (r.z >> 2) & 31, my_proc = r.z >> 12, idx = base + lane;
    const bool live = lane < cnt && my_proc != MSIM_PROCESS_NEMESIS;  // (r/filter (comp number? :process))
    const bool add_like = my_f == MSIM_F_ADD || my_f == MSIM_F_BROADCAST;
    if (live) { const u32 one = 1u << ((my_type & 1) * 16); if (my_type & 2) cnt_hi += one; else cnt_lo += one; }
    // add :ok -> known (first of add-ok / first containing read, by :index): order-free as a minimum; one add per element
    if (live && add_like && my_type == MSIM_T_OK && r.w < p.max_values && known[r.w] > idx) known[r.w] = (u16)idx;
    const u64 add_inv = __ballot(live && add_like && my_type == MSIM_T_INVOKE);  // elements come into existence
    const u32 v_here = v_cur + (u32)__popcll(add_inv & lt);                      // elements existing at this row
    v_cur += (u32)__popcll(add_inv);  // values are handed out 0,1,2,... in invoke order
    const bool is_r = live && my_f == (setfull ? MSIM_F_READ : MSIM_F_ECHO);
    const u64 ri = __ballot(is_r && my_type == MSIM_T_INVOKE);
    const u32 rank = n_ri + (u32)__popcll(ri & lt);                                // invocation order of the reads
    n_ri += (u32)__popcll(ri);
    // what a read :ok leaves behind: its record at the rank of its invocation `sv` = row | rank << 16
    auto record = [&](u32 sv) {
      const u32 rk = sv >> 16;
      if (rk < p.max_reads) {
        u32 *q = rec + (size_t)rk * 3;
        q[0] = r.w | ((r.y >> 16) << 24); q[1] = (sv & 0xFFFFu) | (v_here << 16); q[2] = idx;
        atomicOr(&valid[rk >> 5], 1u << (rk & 31));
      }
    };
    // A completion that directly follows its invocation (all but a few: the rows of one operation are only separated when another
    // worker thread's row falls between them) is settled from the lane below; the pair never touches the thread's table entry.
    // (Same PROCESS, which is the same worker thread for the two rows of one operation; the invocation's rank is this lane's count of the
    //  invocations below it, less one.  Rows reach the lane above by DPP: the packed word, and for echo the value.)
    const u32 below_z = c_dpp<0x138, 0xF, true>(r.z);   // wave_shr:1
    const u32 below_v = setfull ? 0u : c_dpp<0x138, 0xF, true>(r.w);
    const bool adj = is_r && my_type != MSIM_T_INVOKE && lane > 0 && (below_z & 3) == MSIM_T_INVOKE && ((below_z ^ r.z) & 0xFFFFF07Cu) == 0;
    const u64 adj_m = __ballot(adj);
    if (adj) {
      if (setfull) { if (my_type == MSIM_T_OK) record((idx - 1) | ((rank - 1) << 16)); }
      // echo.clj:44-63: every :invoke whose completion is not an :ok carrying the same :echo is an error — a :fail, an
      // :info (its :value is the request string, (:echo "...") = nil) and an invocation that never completes included
      else if (my_type != MSIM_T_OK || below_v != r.w) errors++;
    }
    bool pend = is_r && !adj && !((adj_m >> 1 >> lane) & 1);
    u64 pm = __ballot(pend);
    // worker thread = process mod C ([upstream] jepsen's interpreter): one float multiply and a correction instead of a division
    u32 tt = 0;
    if (pm && pend) {
      const u32 qd = (u32)((float)my_proc * p.rcp_C);
      int rem = (int)(my_proc - qd * C);
      if (rem < 0) rem += (int)C;
      if (rem >= (int)C) rem -= (int)C;
      tt = (u32)rem;
    }
    while (pm) {   // rounds: the earliest pending read row of every worker thread acts on the thread's table entry
      const u32 key = (round_key << 6) | lane;
      if (pend) atomicMin(&first[tt], key);
      c_lds_fence();   // (one wavefront: LDS is in order; __syncthreads would also wait for the rows in flight)
      if (pend && first[tt] == key) {
        pend = false;
        const u32 s = slot[tt];
        if (my_type == MSIM_T_INVOKE) {
          slot[tt] = setfull ? (idx | (rank << 16)) : idx;
          if (!setfull) slotv[tt] = r.w;
        } else {
          slot[tt] = NONE32;
          if (setfull) { if (my_type == MSIM_T_OK && s != NONE32) record(s); }
          else if (my_type != MSIM_T_OK || slotv[tt] != r.w) errors++;
        }
      }
      round_key--;
      c_lds_fence();   // (one wavefront: LDS is in order; __syncthreads would also wait for the rows in flight)
      pm = __ballot(pend);
#ifdef CK_PROF
      ck_rounds++;
#endif
    }
  };
  if (n_rows) {
    uint4 q0 = ldrow(0), q1 = ldrow(64), q2 = ldrow(128), q3 = ldrow(192);
    for (u32 base = 0; base < n_rows; base += 256) {
      rowchunk(base, q0); q0 = ldrow(base + 256);
      if (base + 64 >= n_rows) break;
      rowchunk(base + 64, q1); q1 = ldrow(base + 320);
      if (base + 128 >= n_rows) break;
      rowchunk(base + 128, q2); q2 = ldrow(base + 384);
      if (base + 192 >= n_rows) break;
      rowchunk(base + 192, q3); q3 = ldrow(base + 448);
    }
  }
  if (!setfull) { for (u32 i = lane; i < C; i += 64) errors += slot[i] != NONE32 ? 1u : 0u; }   // invocations left without a completion
  errors = c_wave_sum(errors);
  cnt_lo = c_wave_sum(cnt_lo & 0xFFFFu) | (c_wave_sum(cnt_lo >> 16) << 16);   // (at most 65534 rows: every count fits 16 bits)
  cnt_hi = c_wave_sum(cnt_hi & 0xFFFFu) | (c_wave_sum(cnt_hi >> 16) << 16);
  const u32 op_count = cnt_lo & 0xFFFFu, n_ok = cnt_lo >> 16, n_fail = cnt_hi & 0xFFFFu, n_info = cnt_hi >> 16;
  __threadfence_block();
  __syncthreads();
  if (n_ri > p.max_reads) n_ri = p.max_reads;
#ifdef CK_PROF
  ck_t1 = __builtin_readcyclecounter();
#endif

  // ---- pass 2: ONE sweep over the :ok reads in invocation order, 64 reads at a time, LANE r = READ r of the chunk ----------------------------
  // Per element three reductions over the reads (§ header): last-present = the LAST read that has it, last-absent = the LAST read that lacks
  // it while it exists, known = the smallest :ok index among the reads that have it.  Rounds 3-6 swept with lane w = word w of ONE read's
  // bitmap at a time: a read cost ~140 issued instructions whatever it changed (its rank, three readlanes, the load, the masks, three bit
  // loops), half the lanes idle (17 words on average).  Now a lane holds its OWN read's bitmap (16-byte loads at the read's own address, three
  // in flight) and the wavefront walks the words 0 .. max words of the chunk; for word w
  //   last-present: the highest lane with a bit decides ALL its bits at once (one 32-lane store, lane b = element 32w + b); what is left
  //     (bits some lower lane has and that one has not: only at the frontier of the elements still spreading) takes the next-highest lane with
  //     one of them, and so on.  Later chunks overwrite: the last chunk's last read wins.  last-absent likewise over ~word & existing
  //     (nothing to do for words whose elements every read of the chunk holds);
  //   known: the FIRST lane that has a not-yet-seen element gives its :ok index (lowest lane first, all its new bits at once) — right unless a
  //     read invoked later completed earlier; such a read has an :ok index below the maximum of the reads before it, so every lane of which
  //     that is true (`nm`: rare) takes the minimum over ALL its bits — which is always allowed, `known` being a minimum over containing reads.
  // Element 32w + b is always written by lane b: no cross-lane ordering in LDS.
  {
    const u32 sub = lane & 31u;
    uint4 tiny = make_uint4(0, 0, 0, 0);   // a payload slab of less than four words, whole
    if (p.max_pay < 4) { if (p.max_pay > 0) tiny.x = pay[0]; if (p.max_pay > 1) tiny.y = pay[1]; if (p.max_pay > 2) tiny.z = pay[2]; }
    u32 unkv = 0xFFFFFFFFu;          // lane j: the elements of word j no read has contained yet
    u64 unk_any = ~0ull;             // wave-uniform: the lanes of unkv that are not zero
    u32 pend = NONE;                 // lane j: word j was SETTLED in the last chunk that had it (below) — last-present of its 32 elements, not yet written
    u32 ok_carry = 0;                // the largest :ok index of the chunks before
    auto chunk_mask = [&](u32 cb) -> u64 {
      if (cb >= n_ri) return 0ull;
      const u32 cn = min(64u, n_ri - cb);
      return ((u64)valid[cb / 32 + 1] << 32 | valid[cb / 32]) & (cn >= 64 ? ~0ull : ((1ull << cn) - 1));
    };
    // the records of the next chunk are requested while this one is swept
    u32 nx = 0, ny = 0, nz = 0;
    u64 nmask = chunk_mask(0);
    if ((nmask >> lane) & 1) { const u32 *q = rec + (size_t)lane * 3; nx = q[0]; ny = q[1]; nz = q[2]; }
    for (u32 cb = 0; cb < n_ri; cb += 64) {
      const u64 vmask = nmask;
      const u32 rx = nx, ry = ny, rz = nz;   // {payload ref | words << 24, invoke index | elements existing at completion << 16, :ok index}; 0 for a rank without an :ok
      nmask = chunk_mask(cb + 64);
      nx = ny = nz = 0;
      if ((nmask >> lane) & 1) { const u32 *q = rec + (size_t)(cb + 64 + lane) * 3; nx = q[0]; ny = q[1]; nz = q[2]; }
      if (!vmask) continue;
      const u32 ref = rx & 0xFFFFFFu, nw = rx >> 24, inv = ry & 0xFFFFu, v_here = ry >> 16, ok = rz;
      // four words of this lane's bitmap from word 4g on: ONE unconditional 16-byte load (a lane with nothing there reads the slab's first
      // words and ignores them: no branch around the load, so the loads in flight stay countable).  A bitmap that ends in the slab's last
      // three words — one instance in thousands — reads the slab's last four words and shifts.  (A slab of less than four words holds no bitmap
      // worth the name: it is read once, before the sweep.)
      auto ld = [&](u32 g) -> uint4 {
        const u32 at = ref + 4 * g;
        const bool in = 4 * g < nw;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p.max_pay >= 4) {
          const u32 last4 = p.max_pay - 4;
          const ck_u32x4 q = *reinterpret_cast<const ck_u32x4 *>(pay + (in ? min(at, last4) : 0u));   // (16 bytes at a 4-byte boundary)
          v = in ? make_uint4(q.x, q.y, q.z, q.w) : make_uint4(0, 0, 0, 0);   // (a lane without a word in this group — a rank without a record among them — holds zeros)
          if (__ballot(in && at > last4)) {
            const u32 sh = in && at > last4 ? at - last4 : 0u;
            if (sh == 1) v = make_uint4(v.y, v.z, v.w, 0); else if (sh == 2) v = make_uint4(v.z, v.w, 0, 0); else if (sh >= 3) v = make_uint4(sh == 3 ? v.w : 0u, 0, 0, 0);
          }
        } else if (in) {   // (no load here: a load on this path would make the loads in flight uncountable for the path that matters)
          auto tw = [&](u32 i) { return i == 0 ? tiny.x : (i == 1 ? tiny.y : (i == 2 ? tiny.z : 0u)); };
          v = make_uint4(tw(at), tw(at + 1), tw(at + 2), 0);
        }
        return v;
      };
      uint4 b0 = ld(0), b1 = ld(1), b2 = ld(2), b3 = ld(3);
      const u32 maxw = min(64u, c_wave_max(max(nw, (v_here + 31) >> 5)));   // (a bitmap may be shorter than the elements that exist: they are absent)
      // lanes whose :ok index is below the largest of the reads before them: inclusive prefix maximum, then the lane below's
      const u32 pm = c_wave_incl_max(ok);
      u32 before = (u32)__shfl_up((int)pm, 1);
      before = max(lane ? before : 0u, ok_carry);
      const u64 nm_mask = __ballot(((vmask >> lane) & 1) && ok < before);
      ok_carry = max(ok_carry, c_rdlane(pm, 63));
      const u32 inv_top = c_rdlane(inv, 63u - (u32)__builtin_clzll(vmask));
      const u32 minw = ~c_wave_max(((vmask >> lane) & 1) ? ~nw : 0u);   // every read of the chunk has at least this many words
      // one word of the 64 bitmaps.  What the loops decide for element 32w + b collects in lane b's registers; LDS is touched once per word and kind
      auto word = [&](const u32 w, const u32 raw) {
        u32 W = raw;
        if (w >= minw) W = w < nw ? raw : 0u;   // (wave-uniform test: below minw every read of the chunk has the word, and a lane without a read holds zeros)
        u32 unk_w = (unk_any >> w) & 1 ? c_rdlane(unkv, w) : 0u;
        // A SETTLED word — every read of the chunk holds all 32 elements, all of them seen before, no overtaker among the reads: most words,
        // the elements behind the frontier — changes one thing: last-present = the chunk's last read, for all 32.  That is noted in `pend`
        // and written when a chunk finds the word unsettled, or at the end.
        if (__ballot(W == 0xFFFFFFFFu) == vmask && unk_w == 0 && nm_mask == 0) { if (lane == w) pend = inv_top; return; }
        const u32 e = 32 * w + sub;
        const bool e_ok = lane < 32 && e < p.max_values;
        const u32 pw = c_rdlane(pend, w);
        if (pw != NONE) { if (e_ok) lp_idx[e] = (u16)pw; if (lane == w) pend = NONE; }
        const int d = (int)v_here - (int)(32 * w);
        const u32 ex = d >= 32 ? 0xFFFFFFFFu : (d <= 0 ? 0u : ((1u << d) - 1));  // elements that exist at this read
        const u32 A = ~W & ex;
        u64 m = __ballot(W != 0);
        const u64 holders = m;
        if (m) {   // last-present
          u32 rem = 0xFFFFFFFFu, got = 0;
          do {
            const u32 L = 63u - (u32)__builtin_clzll(m);
            const u32 bits = c_rdlane(W, L) & rem, iv = c_rdlane(inv, L);
            got = ((bits >> sub) & 1) ? iv : got;
            rem &= ~bits;
            m = __ballot((W & rem) != 0);
          } while (m);
          if (e_ok && !((rem >> sub) & 1)) lp_idx[e] = (u16)got;
        }
        m = __ballot(A != 0);
        if (m) {   // last-absent
          u32 rem = 0xFFFFFFFFu, got = 0;
          do {
            const u32 L = 63u - (u32)__builtin_clzll(m);
            const u32 bits = c_rdlane(A, L) & rem, iv = c_rdlane(inv, L);
            got = ((bits >> sub) & 1) ? iv : got;
            rem &= ~bits;
            m = __ballot((A & rem) != 0);
          } while (m);
          if (e_ok && !((rem >> sub) & 1)) la_idx[e] = (u16)got;
        }
        if (unk_w) {   // known: the first read that holds a not-yet-seen element gives its :ok index.  Every lane takes the bits NO LOWER lane
          const u32 nw_bits = W & unk_w;   // holds (a prefix OR across the lanes) and writes them itself: as many turns as ONE read has new elements
          if (__ballot(nw_bits != 0)) {
            const u32 below = c_wave_excl_or(nw_bits);
            u32 mine = nw_bits & ~below;
            while (mine) {
              const u32 x = 32 * w + (u32)__builtin_ctz(mine); mine &= mine - 1;
              if (x < p.max_values && known[x] > ok) known[x] = (u16)ok;
            }
            c_lds_fence();   // (the elements of word w are lane b's again below)
            unk_w &= ~(c_rdlane(below, 63) | c_rdlane(nw_bits, 63));   // everything some lane holds
            if (lane == w) unkv = unk_w;
            unk_any = __ballot(unkv != 0);
          }
        }
        u32 kmin = NONE;
        bool any = false;   // wave-uniform
        m = nm_mask & holders;
        if (m) {   // ... and the reads that overtook an earlier one
          any = true;
          do {
            const u32 L = (u32)__builtin_ctzll(m); m &= m - 1;
            const u32 bits = c_rdlane(W, L), okl = c_rdlane(ok, L);
            kmin = ((bits >> sub) & 1) ? min(kmin, okl) : kmin;
          } while (m);
        }
        if (any && e_ok && known[e] > kmin) known[e] = (u16)kmin;
      };
      auto group = [&](const u32 g, const uint4 &c) {
        // four settled words at once (most groups: everything well behind the frontier)
        if (4 * g + 3 < minw && nm_mask == 0 && ((unk_any >> (4 * g)) & 0xFu) == 0 && __ballot((c.x & c.y & c.z & c.w) == 0xFFFFFFFFu) == vmask) {
          if ((lane >> 2) == g) pend = inv_top;
          return;
        }
        word(4 * g, c.x);
        if (4 * g + 1 < maxw) word(4 * g + 1, c.y);
        if (4 * g + 2 < maxw) word(4 * g + 2, c.z);
        if (4 * g + 3 < maxw) word(4 * g + 3, c.w);
      };
      // four 16-byte loads per lane in flight; the buffers keep their registers (a rotation by moves would wait for the load just issued)
      const u32 ng = (maxw + 3) >> 2;
      for (u32 g = 0; g < ng; g += 4) {
        group(g, b0); if (g + 1 >= ng) break; b0 = ld(g + 4);
        group(g + 1, b1); if (g + 2 >= ng) break; b1 = ld(g + 5);
        group(g + 2, b2); if (g + 3 >= ng) break; b2 = ld(g + 6);
        group(g + 3, b3); b3 = ld(g + 7);
      }
    }
    for (u64 m = __ballot(pend != NONE); m; m &= m - 1) {   // the words that were settled to the end
      const u32 w = (u32)__builtin_ctzll(m), pw = c_rdlane(pend, w), e = 32 * w + sub;
      if (lane < 32 && e < p.max_values) lp_idx[e] = (u16)pw;
    }
  }
  __syncthreads();

#ifdef CK_PROF
  ck_t2 = __builtin_readcyclecounter();
#endif
  // ---- per-element outcomes (each lane owns elements e = lane, lane+64, ...; at most 32 per lane) ----
  u32 c_stable = 0, c_lost = 0, c_never = 0, c_stale = 0;
  u32 my_lat[32];  // statically indexed (unrolled): stays in VGPRs
#pragma unroll
  for (u32 k = 0; k < 32; k++) {
    const u32 e = lane + 64 * k;
    u32 l = NOLAT;
    u32 ll = NOLAT;   // EXPLAIN: :lost-latency = long(nanos->ms(max(0, (time(last-present)+1 | 0) - time(known))))
    if (e < v_cur) {
      const u32 kn = known[e], lp = lp_idx[e], la = la_idx[e];
      const bool stable = lp != NONE && (la == NONE || la < lp);
      const bool lost = kn != NONE && la != NONE && (lp == NONE || lp < la) && kn < la;
      if (stable) {
        l = 0;
        if (la != NONE) {
          const uint4 ra = rows[la], rk = rows[kn];
          const u64 ta = (((u64)(ra.y & 0xFFFF) << 32) | ra.x) + 1, tk = ((u64)(rk.y & 0xFFFF) << 32) | rk.x;
          if (ta > tk) l = (u32)((ta - tk) / 1000000ull);
        }
        c_stable++; if (l > 0) c_stale++;
      } else if (lost) {
        c_lost++;
        if constexpr (EXPLAIN) {
          ll = 0;
          if (lp != NONE) {
            const uint4 rp = rows[lp], rk = rows[kn];
            const u64 tp = (((u64)(rp.y & 0xFFFF) << 32) | rp.x) + 1, tk = ((u64)(rk.y & 0xFFFF) << 32) | rk.x;
            if (tp > tk) ll = (u32)((tp - tk) / 1000000ull);
          }
        }
      } else c_never++;
    }
    if constexpr (EXPLAIN) { if (e < v_cur && e < p.max_values) { lat[e] = l; llat[e] = ll; } }   // (regions of their own: nobody's row indices are overwritten)
    else my_lat[k] = l;
  }
  if constexpr (!EXPLAIN) {
  __syncthreads();  // everyone has read the u16 arrays: the same LDS now holds the latencies
#pragma unroll
  for (u32 k = 0; k < 32; k++) { const u32 e = lane + 64 * k; if (e < v_cur) lat[e] = my_lat[k]; }
  }
  __syncthreads();
  const u32 n_stable = c_wave_sum(c_stable), n_lost = c_wave_sum(c_lost), n_never = c_wave_sum(c_never), n_stale = c_wave_sum(c_stale);

  // ---- quantiles of the stable latencies (set_full_quantiles.inc) ----
  const u32 v_lat = EXPLAIN ? min(v_cur, p.max_values) : v_cur;   // the elements that have a latency word
  u32 q[5] = {0, 0, 0, 0, 0};
#define QUANT_ARR lat
#define QUANT_N n_stable
#define QUANT_Q q
#include "set_full_quantiles.inc"

  if constexpr (EXPLAIN) {
    // ---- the explanation: the lost, never-read and stale elements compacted in element order, the eight stalest, the lost latencies ----
    // Lane l holds element base + l of a block of 64 consecutive elements: a ballot per class ranks a member among the block's, on top
    // of the class's count in the blocks before; a segment starts where the one before it ends (the counts WRITTEN: min(count, room left)).
    u32 lq[5] = {0, 0, 0, 0, 0};
#define QUANT_ARR llat
#define QUANT_N n_lost
#define QUANT_Q lq
#include "set_full_quantiles.inc"
    const u32 w_lost = min(n_lost, x.max_elements), w_never = min(n_never, x.max_elements - w_lost), w_stale = min(n_stale, x.max_elements - w_lost - w_never);
    msim_set_element *const el = x.elements + (size_t)inst * x.max_elements;
    auto element_record = [&](const u32 e) {
      const u32 kn = known[e], lp = lp_idx[e], la = la_idx[e], l = lat[e], ll = llat[e];
      msim_set_element r;
      r.element = e; r.outcome = l != NOLAT ? MSIM_SET_STABLE : (ll != NOLAT ? MSIM_SET_LOST : MSIM_SET_NEVER_READ);
      r.latency_ms = l != NOLAT ? l : ll;   // (never-read: NOLAT is MSIM_NO_VALUE)
      r.known_row = kn == NONE ? MSIM_NO_VALUE : kn; r.last_present_row = lp == NONE ? MSIM_NO_VALUE : lp; r.last_absent_row = la == NONE ? MSIM_NO_VALUE : la;
      return r;
    };
    u32 at_lost = 0, at_never = w_lost, at_stale = w_lost + w_never;   // where the next member of each class goes
    for (u32 base = 0; base < v_lat; base += 64) {
      const u32 e = base + lane;
      const bool in = e < v_lat;
      const u32 l = in ? lat[e] : NOLAT, ll = in ? llat[e] : NOLAT;
      const bool is_lost = in && ll != NOLAT, is_never = in && l == NOLAT && ll == NOLAT, is_stale = in && l != NOLAT && l > 0;
      const u64 m_lost = __ballot(is_lost), m_never = __ballot(is_never), m_stale = __ballot(is_stale);
      u32 pos = NOLAT;
      if (is_lost) { const u32 r = at_lost + (u32)__popcll(m_lost & lt); if (r < w_lost) pos = r; }
      else if (is_never) { const u32 r = at_never + (u32)__popcll(m_never & lt); if (r < w_lost + w_never) pos = r; }
      else if (is_stale) { const u32 r = at_stale + (u32)__popcll(m_stale & lt); if (r < w_lost + w_never + w_stale) pos = r; }
      if (pos != NOLAT) el[pos] = element_record(e);   // (pos < max_elements: the slab's bound)
      at_lost += (u32)__popcll(m_lost); at_never += (u32)__popcll(m_never); at_stale += (u32)__popcll(m_stale);
    }
    // :worst-stale — eight rounds of a maximum over (latency, element) below the round before's pick
    msim_set_explain *const hd = x.hdr + inst;
    u32 n_worst = 0, prev_l = NOLAT, prev_e = NOLAT;
    for (u32 r = 0; r < 8; r++) {
      u32 best_l = 0, best_e = 0;   // this lane's largest key below the last pick (stale: latency > 0, so 0 = none; a later element wins a tie)
      for (u32 e = lane; e < v_lat; e += 64) {
        const u32 l = lat[e];
        if (l != NOLAT && l > 0 && l >= best_l && (l < prev_l || (l == prev_l && e < prev_e))) { best_l = l; best_e = e; }
      }
      const u32 top_l = c_wave_max(best_l);
      if (top_l == 0) break;
      const u32 top_e = c_wave_max(best_l == top_l ? best_e + 1 : 0u) - 1;
      if (lane == 0) hd->worst_stale[r] = element_record(top_e);
      prev_l = top_l; prev_e = top_e; n_worst++;
    }
    if (lane == 0) {
      hd->n_lost = w_lost; hd->n_never_read = w_never; hd->n_stale = w_stale;
      hd->truncated = w_lost + w_never + w_stale < n_lost + n_never + n_stale ? 1u : 0u;
      hd->n_worst_stale = n_worst;
      for (int i = 0; i < 5; i++) hd->lost_latency_ms[i] = lq[i];
    }
  }

  if (lane == 0) {
    msim_check_result o;
    o.attempt_count = v_cur; o.stable_count = n_stable; o.lost_count = n_lost; o.never_read_count = n_never;
    o.stale_count = n_stale; o.duplicated_count = 0; o.error_count = errors;
    for (int i = 0; i < 5; i++) o.stable_latency_ms[i] = q[i];
#ifdef CK_PROF
    o.stable_latency_ms[0] = (u32)(ck_t1 - ck_t0); o.stable_latency_ms[1] = (u32)(ck_t2 - ck_t1); o.stable_latency_ms[2] = (u32)(__builtin_readcyclecounter() - ck_t2); o.stable_latency_ms[3] = ck_rounds; o.stable_latency_ms[4] = n_ri;
#endif
    o.op_count = op_count; o.ok_count = n_ok; o.fail_count = n_fail; o.info_count = n_info;
    if (meta.flags) o.valid = 0;
    else if (!setfull) o.valid = errors == 0 ? 1 : 0;
    else o.valid = n_lost ? 0u : (n_stable == 0 ? 2u : 1u);
    p.out[inst] = o;
  }
