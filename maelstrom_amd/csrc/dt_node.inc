// dt_node.inc — the Datomic-style transactor node (demo/ruby/datomic_list_append.rb, specification: oracle/dt_nodes.inc) as the lambdas of
// one node: descend, assoc, save!, start_txn, unlock, apply_txn.  Included inside R3 of dt_kernel<>, dtg_kernel<> and dtg4_kernel<> after the
// round's outputs (rep / r_*, n_out / o_*, need_words / done_*) are declared; dt_input.inc, after it, is what a node and the two services do
// with one input.  The kernel supplies
//   NODE_IX                  the node's index: its lane, or its lane in the group
//   REPLY_OK(type, cmsg)     the answer without a value (txn_ok before its payload is laid out, init_ok) to the client that cmsg names
//   REPLY_ERROR(code, cmsg)  the error answer
//   CLIENT_REF(qb, qsrc)     how a client's msg_id is stored: qb where the client lives in its node's lane, qb | qsrc << 24 where it is an endpoint
//   DT_WAIT_RING             defined where the waiting transactions are a ring of DG_WAITQ (several workers per node), else DT_WAITQ shifted down
// (macros, not variables or lambdas: what a lambda captures decides the device code, and dt_kernel<> is at its register budget)
// and the names of sim_kernel_dt.inc's scratch layout (g_rec, g_hash, g_first, g_kv, g_kvn, g_cas, my_wl, gen, TC).  group64_end.inc forgets the macros.
      auto rec_of = [&](u32 ptr) -> u32 * { return g_rec + ((size_t)(ptr >> 20) * TC + (ptr & 0xFFFFFu)) * DT_RW; };
      auto is_new = [&](u32 ptr) -> bool { return (ptr >> 20) == NODE_IX && (ptr & 0xFFFFFu) >= cu[DC_PSTART]; };
      auto has_key = [&](u32 k) -> bool {   // the key is in the lineage of the working tree
        if (g_first[k] <= cu[DC_RV]) return true;   // (DT_NONE is above every version)
        const u32 no = cu[DC_NOWN];
        for (u32 i = 0; i < no; i++) if (cu[DC_OWN + i] == k) return true;
        return false;
      };
      auto br_index = [&](u32 w0, u32 h) -> u32 {   // branch_index (:231-247) with the split's bounds (:170-181)
        const u32 lo = (w0 >> 8) & 0xFFu, hi = (w0 >> 16) & 0xFFu, bs = (hi - lo) / 8u;
        for (u32 i = 0; i < 7u; i++) if (h < lo + (i + 1u) * bs) return i;
        return 7u;
      };
      auto send1 = [&](u32 dest, u32 type, u32 a, u32 b) { o_dest = dest; n_out = 1; o1_type = type; o1_a = a; o1_b = b; };
      auto start_txn = [&](u32 cmsg, u32 ref) {   // the lock is ours: current_tree (:358-365)
        cu[DC_STAGE] = DS_ROOT; cu[DC_CMSG] = cmsg; cu[DC_REF] = ref; cu[DC_J] = 0; cu[DC_NOWN] = 0;
        const u32 rid = ++node_msgid; cu[DC_RPC] = rid;
        send1(D_LIN, M_READ, 0, rid);
        wait_until = T + DT_AWAIT_US;
      };
      // the next waiting transaction takes the lock (:348, :371), in arrival order; wq_push() is the other end of the queue
#ifdef DT_WAIT_RING   // a ring of DG_WAITQ x {client reference, txn ref}; cu[DG_WQN] = count | head << 8
      constexpr u32 stk_at = DG_STK;   // (the save stack lies behind the queue)
      auto unlock = [&]() {
        cu[DC_STAGE] = DS_IDLE;
        wait_until = INF;
        const u32 wq = cu[DG_WQN], cnt = wq & 0xFFu, head = wq >> 8;
        if (cnt) {
          const u32 cmsg = cu[DG_WQ + 2u * head], ref = cu[DG_WQ + 2u * head + 1u];
          cu[DG_WQN] = (cnt - 1u) | (((head + 1u) & (DG_WAITQ - 1u)) << 8);
          start_txn(cmsg, ref);
        }
      };
      auto wq_push = [&](u32 cmsg, u32 ref) {
        const u32 wq = cu[DG_WQN], cnt = wq & 0xFFu;
        if (cnt == DG_WAITQ) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
        else { const u32 sl = ((wq >> 8) + cnt) & (DG_WAITQ - 1u); cu[DG_WQ + 2u * sl] = cmsg; cu[DG_WQ + 2u * sl + 1u] = ref; cu[DG_WQN] = wq + 1u; }
      };
#else                 // an array of DT_WAITQ x {client reference, txn ref}, shifted down
      constexpr u32 stk_at = DC_STK;
      auto unlock = [&]() {
        cu[DC_STAGE] = DS_IDLE;
        wait_until = INF;
        const u32 wqn = cu[DC_WQN];
        if (wqn) {
          const u32 cmsg = cu[DC_WQ], ref = cu[DC_WQ + 1];
          for (u32 i = 1; i < wqn; i++) { cu[DC_WQ + 2 * (i - 1)] = cu[DC_WQ + 2 * i]; cu[DC_WQ + 2 * (i - 1) + 1] = cu[DC_WQ + 2 * i + 1]; }
          cu[DC_WQN] = wqn - 1;
          start_txn(cmsg, ref);
        }
      };
      auto wq_push = [&](u32 cmsg, u32 ref) {
        const u32 wqn = cu[DC_WQN];
        if (wqn == DT_WAITQ) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
        else { cu[DC_WQ + 2u * wqn] = cmsg; cu[DC_WQ + 2u * wqn + 1u] = ref; cu[DC_WQN] = wqn + 1u; }
      };
#endif
      auto load = [&](u32 ptr) {   // Tree.load with a cache miss (:83-101)
        const u32 rid = ++node_msgid;
        cu[DC_STAGE] = DS_LOAD; cu[DC_TARGET] = ptr; cu[DC_RPC] = rid;
        send1(D_LWW, M_READ, ptr, rid);
        wait_until = T + DT_AWAIT_US;
      };
      // walks to the key's leaf; the first tree node on the way that has to be fetched, DT_NONE if the path is in memory.  One round trip per
      // level: a record's kind / range, its flags word (which nodes have loaded it) and its eight children are loaded together.
      auto descend = [&](u32 k) -> u32 {
        const u32 h = g_hash[k];
        u32 pt = cu[DC_T];
        for (u32 d = 0; d < DT_MAXDEPTH; d++) {
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0], w3 = __hip_atomic_load(r + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (word 3 is the one word of a record that changes after its creation, by L2 atomics: read past the L1)
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          if (!is_new(pt) && !((w3 >> (2u + NODE_IX)) & 1u)) return pt;   // neither created by this transaction nor loaded by this node
          if ((w0 & 1u) == 0u) return DT_NONE;
          const u32 ci = br_index(w0, h);
          pt = ch[0];
#pragma unroll
          for (u32 c = 1; c < 8u; c++) pt = c == ci ? ch[c] : pt;
        }
        my_flags |= MSIM_FLAG_ARENA_OVERRUN;
        return DT_NONE;
      };
      // assoc (:158-197, :256-268) along a path that is in memory.  New pointers go leaf first, then upwards: with n branches above a
      // leaf level of L new nodes (1, or 8 leaves + their branch) the leaf level takes base+1 .. base+L, the branch at depth i
      // base+L+(n-i) — known before the walk down that writes the copies.
      auto assoc = [&](u32 k) {
        const u32 h = g_hash[k];
        u32 n = 0, pt = cu[DC_T];
        for (; n + 1u < DT_MAXDEPTH; n++) {
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0];
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          if ((w0 & 1u) == 0u) break;
          const u32 ci = br_index(w0, h);
          pt = ch[0];
#pragma unroll
          for (u32 c = 1; c < 8u; c++) pt = c == ci ? ch[c] : pt;
        }
        const u32 *const lf = rec_of(pt);
        const u32 lw0 = lf[0], lcount = lf[1];
        if (lw0 & 1u) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; return; }
        const bool has = has_key(k);
        const u32 L = (has || lcount < 8u) ? 1u : 9u, base = next_p, ver = cu[DC_RV] + 1u;
        if (base + L + n >= TC) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; return; }   // engine capacity
        const u32 lo = (lw0 >> 8) & 0xFFu, hi = (lw0 >> 16) & 0xFFu;
        auto put = [&](u32 idx, u32 w0, u32 cnt) -> u32 * { u32 *const r = g_rec + ((size_t)NODE_IX * TC + idx) * DT_RW; r[0] = w0; r[1] = cnt; r[2] = ver; __hip_atomic_store(r + 3, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return r; };   // (word 3: lww-kv replica in bits 0-1, 3 = not written; bit 2 + i: node i has loaded it)
        if (L == 1u) put(base + 1u, lw0, lcount + (has ? 0u : 1u));
        else {   // eight leaves under a new branch: the lineage's keys of this range (and the new one) by sub-range
          const u32 bs = (hi - lo) / 8u, nk = gen[32];
          u64 c_lo = 0, c_hi = 0;   // 4 x 16-bit counters each
          for (u32 q = 0; q < nk; q++) {
            if (q != k && !has_key(q)) continue;
            const u32 hq = g_hash[q];
            if (hq < lo || hq >= hi) continue;
            const u32 ci = bs ? min((hq - lo) / bs, 7u) : 7u;
            if (ci < 4u) c_lo += 1ull << (16u * ci); else c_hi += 1ull << (16u * (ci - 4u));
          }
          u32 *const br = put(base + 9u, 1u | (lo << 8) | (hi << 16), 0u);
          for (u32 i = 0; i < 8u; i++) {
            const u32 b_lo = lo + i * bs, b_hi = i == 7u ? hi : b_lo + bs;
            const u32 cnt = (u32)((i < 4u ? c_lo >> (16u * i) : c_hi >> (16u * (i - 4u))) & 0xFFFFu);
            put(base + 1u + i, (b_lo << 8) | (b_hi << 16), cnt);
            br[4u + i] = (NODE_IX << 20) | (base + 1u + i);
          }
        }
        pt = cu[DC_T];
        for (u32 i = 0; i < n; i++) {   // a copy of every branch above, pointing at the new child
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0], ci = br_index(w0, h);
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          u32 *const nr = put(base + L + (n - i), w0, 0u);
          const u32 child_new = (NODE_IX << 20) | (i + 1u == n ? base + L : base + L + (n - i - 1u));
#pragma unroll
          for (u32 c = 0; c < 8u; c++) nr[4u + c] = c == ci ? child_new : ch[c];
          pt = ch[0];
#pragma unroll
          for (u32 c = 1; c < 8u; c++) pt = c == ci ? ch[c] : pt;
        }
        next_p = base + L + n;
        cu[DC_T] = (NODE_IX << 20) | next_p;
        if (!has) { const u32 no = cu[DC_NOWN]; if (no < 8u) { cu[DC_OWN + no] = k; cu[DC_NOWN] = no + 1u; } }
      };
      // save! (:212-224, :291-320): the new tree nodes the final tree reaches, children before their parent.  A stack entry is a tree node and
      // the mask of its new children still to visit (a branch's eight children are loaded together: one round trip per visit).
      auto save = [&]() {
        u32 *const stk = cu + stk_at;
        u32 sp = 1, wn = 0;
        const u32 wlo = node_msgid + 1u;
        stk[0] = cu[DC_T]; stk[1] = 0x100u;   // (0x100: not looked at yet)
        while (sp) {
          const u32 pt = stk[2u * (sp - 1u)];
          u32 mask = stk[2u * (sp - 1u) + 1u];
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0];
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          if (mask & 0x100u) {
            mask = 0;
            if (w0 & 1u) {
#pragma unroll
              for (u32 c = 0; c < 8u; c++) mask |= is_new(ch[c]) ? 1u << c : 0u;
            }
          }
          if (mask) {
            const u32 ci = (u32)__builtin_ctz(mask);
            u32 nxt = ch[0];
#pragma unroll
            for (u32 c = 1; c < 8u; c++) nxt = c == ci ? ch[c] : nxt;
            stk[2u * (sp - 1u) + 1u] = mask & (mask - 1u);
            if (sp > DT_MAXDEPTH) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; stk[2u * (sp - 1u) + 1u] = 0; continue; }
            stk[2u * sp] = nxt; stk[2u * sp + 1u] = 0x100u; sp++;
            continue;
          }
          if (wn >= DT_MAXW) my_flags |= MSIM_FLAG_ARENA_OVERRUN; else my_wl[wn++] = pt;
          sp--;
        }
        node_msgid += wn;
        cu[DC_STAGE] = DS_SAVE; cu[DC_WLO] = wlo; cu[DC_WN] = wn; cu[DC_WOUT] = wn;
        o_dest = D_LWW; n_out = wn; o_wlo = wlo;
        wait_until = T + DT_AWAIT_US;   // `tree2.save!.await` (:366)
      };
      auto reply_txn_ok = [&]() {   // the completed transaction: its reads see the version read + its own appends
        REPLY_OK(M_TXN_OK, cu[DC_CMSG]);
        done_ref = cu[DC_REF]; done_rv = cu[DC_RV];
        const u32 off0 = done_ref & 0xFFFFFFu, n = done_ref >> 24;
        for (u32 j = 0; j < n; j++) {
          const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
          need_words++;
          if (!(w & 1u)) {
            u32 len = visible(k, done_rv);
            for (u32 e = 0; e < j; e++) { const u32 we = g_pay[off0 + e]; if ((we & 1u) && ((we >> 1) & 0x7FFFu) == k) len++; }
            need_words += (len + 3u) / 4u;
          }
        }
      };
      // apply_txn (:391-415) from micro-op j on; stops at the first tree node that has to be fetched
      auto apply = [&]() {
        const u32 ref = cu[DC_REF], off0 = ref & 0xFFFFFFu, n = ref >> 24;
        u32 j = cu[DC_J];
        while (j < n) {
          const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
          const u32 miss = descend(k);   // t[k] — for an append too (:405)
          if (miss != DT_NONE) { cu[DC_J] = j; load(miss); return; }
          if (w & 1u) assoc(k);
          j++;
        }
        cu[DC_J] = j;
        if (cu[DC_T] == cu[DC_P1]) { reply_txn_ok(); unlock(); return; }   // nothing appended: no write, no cas
        save();
      };
