// mk_node.inc — the multi-key transactional node (demo/js/multi_key_txn.js, specification: oracle/mk_nodes.inc) as the lambdas of one node:
// the thunk cache, thunk_of, casRoot, writeThunks, transact / getState.  Included inside R3 of mk_kernel<> and mkg_kernel<> after the round's
// outputs (rep, n_out / o_*, need_words, done_slot) are declared; mk_input.inc, after it, is what a node and the two services do with one
// input.  In both kernels a node's index is its lane.  The kernel supplies
//   MK_NSLOTS               transactions in flight per node
//   REPLY_TO(cmsg)          starts the answer to the client that a stored client reference names (rep, o_b and where it goes)
//   CLIENT_REF(qb, qsrc)    how a client's msg_id is stored: qb where the client lives in its node's lane, qb | qsrc << 24 where it is an endpoint
// group64_end.inc forgets them.
      u32 *const my_out = mout + lane * (MK_KEYS * 3u);
      auto out_msg = [&](u32 dest, u32 type, u32 a, u32 b) { o_dest = dest; my_out[n_out * 3u] = type; my_out[n_out * 3u + 1u] = a; my_out[n_out * 3u + 2u] = b; n_out++; };
      // the node's thunk cache (multi_key_txn.js:17,80-106): one bit per thunk id <node>.<i>, [owner][i / 32] in the first N x TC / 32 words of the
      // node's CC-word area
      auto cached = [&](u32 tid) -> bool { const u32 i = tid & 0xFFFFFu; return (my_cache[(tid >> 20) * (TC >> 5) + (i >> 5)] >> (i & 31u)) & 1u; };
      auto cache_add = [&](u32 tid) { const u32 i = tid & 0xFFFFFu; my_cache[(tid >> 20) * (TC >> 5) + (i >> 5)] |= 1u << (i & 31u); };
      // the thunk the root of version v names for `k` (MK_NONE: the map does not have the key)
      auto thunk_of = [&](u32 k, u32 v) -> u32 {
        const u32 first = g_first[k], cnt = g_updn[k];   // (never entered: MK_NONE > any version)
        if (first > v) return MK_NONE;
        if (mw1 <= 17u) {   // the versions of the key's thunks grow along the row: count those <= v with independent loads, then one more for the id
          u32 row[17];
#pragma unroll
          for (u32 i = 0; i < 17u; i++) row[i] = i < cnt ? g_upd_v[k * mw1 + i] : 0xFFFFFFFFu;
          u32 n = 0;
#pragma unroll
          for (u32 i = 0; i < 17u; i++) n += (i < cnt && row[i] <= v) ? 1u : 0u;
          return n ? g_upd_t[k * mw1 + n - 1u] : MK_NONE;
        }
        u32 t = MK_NONE;
        for (u32 i = 0; i < cnt && g_upd_v[k * mw1 + i] <= v; i++) t = g_upd_t[k * mw1 + i];
        return t;
      };
      auto send_cas = [&](u32 *sl, u32 si) {   // casRoot, :120-137
        const u32 rid = ++node_msgid;
        sl[SK_HDR] = 1u | (3u << 8); sl[SK_RPC] = rid;
        out_msg(D_LIN, M_CAS, sl[SK_RV] | (si << 16), rid);
      };
      // writeThunks (:160-177): state2's keys in insertion order — the thunks read, then the keys the transaction creates
      auto begin_writes = [&](u32 *sl, u32 si) {
        const u32 nk = sl[SK_NK], ns = sl[SK_NSTATE];
        u32 ord[MK_KEYS], n = 0, in_state = 0;
        for (u32 i = 0; i < ns; i++) { const u32 j = sl[SK_SORD + i]; ord[n++] = j; in_state |= 1u << j; }
        for (u32 i = 0; i <= MK_KEYS; i++)
          for (u32 j = 0; j < nk; j++) if (!((in_state >> j) & 1u) && sl[SK_WR + j] && sl[SK_FA + j] == i) ord[n++] = j;
        sl[SK_HDR] = 1u | (2u << 8); sl[SK_NNEW] = 0;
        u32 wr_out = 0;
        for (u32 i = 0; i < n; i++) {
          const u32 j = ord[i];
          if (!sl[SK_WR + j]) continue;
          if (next_tid >= TC) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; continue; }   // engine capacity
          const u32 tid = (lane << 20) | next_tid++;
          cache_add(tid);
          const u32 rid = ++node_msgid;
          sl[SK_WRTID + j] = tid; sl[SK_WRRPC + j] = rid; wr_out++;
          out_msg(D_LWW, M_WRITE, tid, rid);
        }
        sl[SK_WROUT] = wr_out;
        if (wr_out == 0) send_cas(sl, si);
      };
      auto thunk_ready = [&](u32 *sl, u32 j) { const u32 ns = sl[SK_NSTATE]; sl[SK_SORD + ns] = j; sl[SK_NSTATE] = ns + 1u; sl[SK_RDRPC + j] = 0; };
      // transact (:213-236) from the node's cached root; getState (:141-156) walks the root's keys in map order
      auto start_attempt = [&](u32 *sl, u32 si) {
        const u32 nk = sl[SK_NK], rv = root_v;
        sl[SK_RV] = rv; sl[SK_HDR] = 1u | (1u << 8); sl[SK_NSTATE] = 0;
        u32 posn[MK_KEYS], tids[MK_KEYS], rd_out = 0;
        for (u32 j = 0; j < nk; j++) { sl[SK_RDRPC + j] = 0; const u32 k = sl[SK_KEY + j]; tids[j] = thunk_of(k, rv); posn[j] = tids[j] == MK_NONE ? MK_NONE : g_pos[k]; }
        for (u32 done = 0;;) {   // ascending position in the root map
          u32 best = MK_NONE, bj = 0;
          for (u32 j = 0; j < nk; j++) if (!((done >> j) & 1u) && posn[j] < best) { best = posn[j]; bj = j; }
          if (best == MK_NONE) break;
          done |= 1u << bj;
          if (cached(tids[bj])) thunk_ready(sl, bj);
          else { const u32 rid = ++node_msgid; sl[SK_RDTID + bj] = tids[bj]; sl[SK_RDRPC + bj] = rid; rd_out++; out_msg(D_LWW, M_READ, tids[bj], rid); }
        }
        sl[SK_RDOUT] = rd_out;
        if (rd_out == 0) begin_writes(sl, si);
      };
