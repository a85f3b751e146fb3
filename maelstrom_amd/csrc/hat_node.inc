// hat_node.inc — R3 of the txn-rw-register (HAT) node, demo/clojure/txn_rw_register_hat.clj (specification: oracle/hat_nodes.inc): a due replication tick or the due message of every node, the
// shared areas they need (txn slots, payload words, list words), the handlers, and the wavefront-wide passes over long lists.  Included in
// hat_kernel<> and hatg_kernel<> after the round's outputs (rep, dmask, o_*) are declared; in both a node's index is its lane.  The timer
// in the time jump stays each kernel's own (docs/KERNELS.md).  The kernel supplies
//   REPLY_TO(cmsg)         starts the answer to the client that a client reference names (rep, o_b and where it goes)
//   CLIENT_REF(qb, qsrc)   a client reference: qb where the client lives in its node's lane, qb | qsrc << 24 where it is an endpoint
// group64_end.inc forgets them.
      const bool tick = is_node && timer_next <= T;
      const bool msg = is_node && !tick && deliver_at <= T;
      const u32 jd_mask = jcap ? (u32)__ballot(msg) : 0u;
      uint4 q = make_uint4(0, 0, 0, 0);
      if (msg) {
        q = cm; deliver_at = INF;
        if ((q.w >> 24) >= N) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, q.z, q.w & 0xFFFFFFu, q.w >> 24, lane);
      }
      n_ev += __popc(jd_mask);
      const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = msg ? (q.y & 0xFFu) : 0u, qa = q.z;

      // what this round's inputs need from the shared areas: txn slots + payload words (txn), list words (tick)
      const bool in_txn = qtype == M_TXN;
      u32 need_pay = in_txn ? (qa >> 24) : 0u, need_area = 0, t_dest = 0;
      // replicate-step!, :92-105: the oldest unreplicated txn, the lowest node it still has to reach.  After a partition heals the
      // acknowledgements clear hundreds of pending bytes at once: a long way to the oldest one left is searched by the whole wavefront,
      // 64 slots per step (round 3; as one lane's loop every slot was an HBM round trip)
      for (u32 tm = (u32)__ballot(tick && n_txn - lo > HAT_SHORT); tm; tm &= tm - 1) {
        const u32 x = (u32)__builtin_ctz(tm), lo_x = rdlane(lo, x);
        const unsigned char *const px = pend_all + (size_t)x * G;
        u32 first = n_txn;
        for (u32 g0 = lo_x; g0 < n_txn; g0 += 64) {
          const u32 g = g0 + lane, m = g < n_txn ? (u32)px[g] : 0u;
          const u64 bal = __ballot(m != 0);
          if (bal) { first = g0 + (u32)__builtin_ctzll(bal); break; }
        }
        if (lane == x) lo = first;
      }
      if (tick) {
        timer_next = T + HAT_TICK_US;
        while (lo < n_txn && !g_pend[lo]) lo++;
        if (lo >= n_txn) timer_next = INF;
        else t_dest = (u32)__builtin_ctz((u32)g_pend[lo]);
      }
      // The lists of the ticking nodes are counted here and written below by the whole wavefront, 64 txn slots per step:
      // behind a partition a node holds hundreds of unreplicated txns and lists them all again every 100 ms.
      const u32 tk = (u32)__ballot(tick && lo < n_txn);
      u32 area_total = 0;
      for (u32 tm = tk; tm; tm &= tm - 1) {
        const u32 x = (u32)__builtin_ctz(tm), lo_x = rdlane(lo, x), d_x = rdlane(t_dest, x);
        const unsigned char *const px = pend_all + (size_t)x * G;
        u32 c = 0;
        for (u32 g0 = lo_x; g0 < n_txn; g0 += 64) {
          const u32 g = g0 + lane, m = g < n_txn ? (u32)px[g] : 0u;
          c += (u32)__popcll(__ballot((m >> d_x) & 1u));
        }
        if (lane == x) need_area = c;
        area_total += c;
      }
      const u32 txn_mask = (u32)__ballot(in_txn);
      const u32 pay_incl = scan32(need_pay);
      const u32 pay_total = rdlane(pay_incl, 31);
      bool txn_ok = in_txn;
      if (txn_mask) {
        if (n_txn + __popc(txn_mask) > G || __ballot(in_txn && lamport >= (1u << 21) - 1)) { flags |= MSIM_FLAG_ARENA_OVERRUN; txn_ok = false; }
        else if (n_payload + pay_total > max_pay) { flags |= MSIM_FLAG_PAYLOAD_OVERFLOW; txn_ok = false; }
      }
      bool area_ok = true;
      if (area_total && n_area + area_total > area_cap) { flags |= MSIM_FLAG_ARENA_OVERRUN; area_ok = false; }  // engine capacity; nothing is sent
      if (area_ok) {
        u32 w_run = n_area;
        for (u32 tm = tk; tm; tm &= tm - 1) {
          const u32 x = (u32)__builtin_ctz(tm), lo_x = rdlane(lo, x), d_x = rdlane(t_dest, x);
          const unsigned char *const px = pend_all + (size_t)x * G;
          const u32 w0 = w_run;
          for (u32 g0 = lo_x; g0 < n_txn; g0 += 64) {
            const u32 g = g0 + lane, m = g < n_txn ? (u32)px[g] : 0u;
            const bool bit = ((m >> d_x) & 1u) != 0;
            const u64 bal = __ballot(bit);
            if (bit) g_area[w_run + (u32)__popcll(bal & lt_mask)] = g | (m << 24);
            w_run += (u32)__popcll(bal);
          }
          if (lane == x) { o_type = M_REPLICATE; o_a = w0; o_b = need_area; dmask = 1u << d_x; }
        }
      }

      if (tick) {
        // (its replicate, if any, was set up above)
      } else if (txn_ok) {  // :120-130
        const u32 g = n_txn + __popc(txn_mask & lt32), off0 = qa & 0xFFFFFFu, n = qa >> 24;
        const u32 off = n_payload + pay_incl - need_pay, ts = (lamport++ << 3) | lane;
        for (u32 j = 0; j < n; j++) {  // micro-ops in order: a read sees the transaction's own earlier writes
          const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu, cur = g_kv[k];
          if (w & 1) { if (!(cur && (cur >> 8) > ts)) g_kv[k] = (ts << 8) | ((w >> 16) & 0xFFu); g_pay[off + j] = w; }
          else g_pay[off + j] = (k << 1) | ((cur ? cur & 0xFFu : 0xFFu) << 16);
        }
        g_tab[2 * g] = ts; g_tab[2 * g + 1] = qa;
        g_pend[g] = (unsigned char)(all_nodes & ~(1u << lane));  // later-replicate!, :85-90
        if (npend++ == 0) { lo = g; if (timer_next == INF) timer_next = (T / HAT_TICK_US + 1u) * HAT_TICK_US; }
        REPLY_TO(CLIENT_REF(qb, qsrc)); o_type = M_TXN_OK; o_a = off | (n << 24);
      } else if (qtype == M_INIT) { REPLY_TO(CLIENT_REF(qb, qsrc)); o_type = M_INIT_OK; }
      else if (qtype == M_REPLICATE && qb <= HAT_SHORT) {  // :132-150 (a long list: below, by the whole wavefront)
        for (u32 i = 0; i < qb; i++) {
          const u32 w = g_area[qa + i], g = w & 0xFFFFFFu, ts = g_tab[2 * g], ref = g_tab[2 * g + 1];
          lamport = max(lamport, (ts >> 3) + 1);
          const u32 off0 = ref & 0xFFFFFFu, n = ref >> 24;
          for (u32 j = 0; j < n; j++) {  // apply-txn+ at the txn's own timestamp: last write wins
            const u32 mw_ = g_pay[off0 + j], k = (mw_ >> 1) & 0x7FFFu;
            if (!(mw_ & 1)) continue;
            const u32 cur = g_kv[k];
            if (!(cur && (cur >> 8) > ts)) g_kv[k] = (ts << 8) | ((mw_ >> 16) & 0xFFu);
          }
          const u32 rest = (w >> 24) & ~(1u << lane);
          if (rest) {  // still pending elsewhere: this node relays it (its own entry for that timestamp is replaced)
            if (!g_pend[g]) { if (npend++ == 0) { lo = g; if (timer_next == INF) timer_next = (T / HAT_TICK_US + 1u) * HAT_TICK_US; } else lo = min(lo, g); }
            g_pend[g] = (unsigned char)rest;
          }
        }
        o_type = M_REPLICATE_ACK; o_a = qa; o_b = qb; dmask = all_nodes & ~(1u << lane);
      } else if (qtype == M_REPLICATE_ACK && qb <= HAT_SHORT) {  // :152-172
        for (u32 i = 0; i < qb; i++) {
          const u32 g = g_area[qa + i] & 0xFFFFFFu;
          u32 m = g_pend[g];
          if (!m) continue;  // txn already fully replicated
          m &= ~(1u << qsrc);
          g_pend[g] = (unsigned char)m;
          if (!m) npend--;
        }
        if (npend == 0) timer_next = INF;
      }
      // Long lists (hundreds of txns once a partition has healed): one receiving node at a time, 64 entries per step.  A register takes
      // the write with the highest timestamp (last write wins; the entries of a list are different txns, so their order does not matter:
      // an atomic max on timestamp | value — two writes of ONE txn to a register carry increasing values, the later one is the larger
      // word); the entries name different slots, so the pending bytes do not collide.  (Round 3; csrc/hat8.hip has the same passes.)
      {
        const bool is_rep = msg && qtype == M_REPLICATE && qb > HAT_SHORT, is_ack = msg && qtype == M_REPLICATE_ACK && qb > HAT_SHORT;
        const u32 ack_m = (u32)__ballot(is_ack);
        for (u32 lw = (u32)__ballot(is_rep || is_ack); lw; lw &= lw - 1) {
          const u32 x = (u32)__builtin_ctz(lw), x_qa = rdlane(qa, x), x_qb = rdlane(qb, x), x_src = rdlane(qsrc, x);
          u32 *const xkv = g_scr + (size_t)x * K;
          unsigned char *const xp = pend_all + (size_t)x * G;
          if (!((ack_m >> x) & 1u)) {
            u32 lam = 0, newly = 0, lo_min = INF;
            for (u32 i0 = 0; i0 < x_qb; i0 += 64) {
              const u32 i = i0 + lane;
              if (i < x_qb) {
                const u32 w = g_area[x_qa + i], g = w & 0xFFFFFFu, ts = g_tab[2 * g], ref = g_tab[2 * g + 1];
                lam = max(lam, (ts >> 3) + 1);
                const u32 off0 = ref & 0xFFFFFFu, n = ref >> 24;
                for (u32 j = 0; j < n; j++) {
                  const u32 mw_ = g_pay[off0 + j];
                  if (mw_ & 1) atomicMax(&xkv[(mw_ >> 1) & 0x7FFFu], (ts << 8) | ((mw_ >> 16) & 0xFFu));
                }
                const u32 rest = (w >> 24) & ~(1u << x);
                if (rest) {
                  if (!xp[g]) { newly++; lo_min = min(lo_min, g); }
                  xp[g] = (unsigned char)rest;
                }
              }
            }
            const u32 lam_w = ~wave_min(~lam), lo_w = wave_min(lo_min), newly_w = wave_sum(newly);
            if (lane == x) {
              lamport = max(lamport, lam_w);
              if (newly_w) {
                if (npend == 0) { lo = lo_w; if (timer_next == INF) timer_next = (T / HAT_TICK_US + 1u) * HAT_TICK_US; } else lo = min(lo, lo_w);
                npend += newly_w;
              }
              o_type = M_REPLICATE_ACK; o_a = qa; o_b = qb; dmask = all_nodes & ~(1u << lane);
            }
          } else {
            u32 cleared = 0;
            for (u32 i0 = 0; i0 < x_qb; i0 += 64) {
              const u32 i = i0 + lane;
              if (i < x_qb) {
                const u32 g = g_area[x_qa + i] & 0xFFFFFFu;
                u32 m = xp[g];
                if (m) {
                  m &= ~(1u << x_src);
                  xp[g] = (unsigned char)m;
                  if (!m) cleared++;
                }
              }
            }
            const u32 cleared_w = wave_sum(cleared);
            if (lane == x) { npend -= cleared_w; if (npend == 0) timer_next = INF; }
          }
        }
      }
      if (txn_mask && __ballot(txn_ok)) { n_txn += __popc(txn_mask); n_payload += pay_total; }
      if (area_ok) n_area += area_total;
