// mk_input.inc — one input of the multi-key transactional cluster: a node's input switch (slot search, start_attempt, the thunk read, write
// and cas stages), the lin-kv lane (root read, cas with create_if_not_exists) and the lww-kv lane.  Included where the kernel has taken the
// envelope apart into qtype, qa, qb, qsrc; mk_node.inc has the node's lambdas and says what the kernel supplies.
        if (is_node) {
          switch (qtype) {
            case M_INIT: REPLY_TO(CLIENT_REF(qb, qsrc)); o_type = M_INIT_OK; break;
            case M_TXN: {
              u32 si = 0; while (si < MK_NSLOTS && (slot_of(my_node, si)[SK_HDR] & 0xFFu)) si++;
              if (si == MK_NSLOTS) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; break; }   // engine capacity; the reference has no bound
              u32 *const sl = slot_of(my_node, si);
              for (u32 i = 0; i < MKW; i++) sl[i] = 0;
              sl[SK_HDR] = 1u; sl[SK_CMSG] = CLIENT_REF(qb, qsrc); sl[SK_REF] = qa;
              const u32 off0 = qa & 0xFFFFFFu, n = qa >> 24;
              u32 nk = 0;
              for (u32 i = 0; i < n; i++) {   // readSet / writeSet (:180-197)
                const u32 w = g_pay[off0 + i], k = (w >> 1) & 0x7FFFu;
                u32 j = 0; while (j < nk && sl[SK_KEY + j] != k) j++;
                if (j == nk) { sl[SK_KEY + j] = k; nk++; }
                if ((w & 1u) && !sl[SK_WR + j]) { sl[SK_WR + j] = 1u; sl[SK_FA + j] = i; }
              }
              sl[SK_NK] = nk;
              start_attempt(sl, si);
            } break;
            case M_READ_OK: case M_WRITE_OK: case M_CAS_OK: case M_ERROR: {
              bool found = false;
              for (u32 si = 0; si < MK_NSLOTS && !found; si++) {
                u32 *const sl = slot_of(my_node, si);
                const u32 hdr = sl[SK_HDR];
                if (!(hdr & 0xFFu)) continue;
                const u32 stage_ = (hdr >> 8) & 0xFFu, nk = sl[SK_NK];
                if (stage_ == 1u) {
                  for (u32 j = 0; j < nk; j++) if (qb && sl[SK_RDRPC + j] == qb) {
                    found = true;
                    const u32 tid = sl[SK_RDTID + j];
                    if (qtype == M_READ_OK) { cache_add(tid); thunk_ready(sl, j); sl[SK_RDOUT]--; }
                    else if (qa == 20u) {   // not on the replica that answered: getThunk again (:92-96), from the cache if it is there by now
                      if (cached(tid)) { thunk_ready(sl, j); sl[SK_RDOUT]--; }
                      else { const u32 rid = ++node_msgid; sl[SK_RDRPC + j] = rid; out_msg(D_LWW, M_READ, tid, rid); }
                    }
                    if (sl[SK_RDOUT] == 0) begin_writes(sl, si);
                    break;
                  }
                } else if (stage_ == 2u) {
                  for (u32 j = 0; j < nk; j++) if (qb && sl[SK_WR + j] && sl[SK_WRRPC + j] == qb) {
                    found = true;
                    sl[SK_WRRPC + j] = 0;
                    if (thunk_of(sl[SK_KEY + j], sl[SK_RV]) == MK_NONE) { const u32 nn = sl[SK_NNEW]; sl[SK_NORD + nn] = j; sl[SK_NNEW] = nn + 1u; }
                    if (--sl[SK_WROUT] == 0) send_cas(sl, si);
                    break;
                  }
                } else if (sl[SK_RPC] == qb) {
                  found = true;
                  if (stage_ == 3u) {
                    if (qtype == M_CAS_OK) {   // :226-229: the cached root becomes the new map, the client gets the completed transaction
                      u32 writes = 0; for (u32 j = 0; j < nk; j++) writes |= sl[SK_WR + j];
                      const u32 rv = sl[SK_RV];
                      root_v = rv + (writes ? 1u : 0u);
                      REPLY_TO(sl[SK_CMSG]); o_type = M_TXN_OK; done_slot = si;
                      const u32 ref = sl[SK_REF], off0 = ref & 0xFFFFFFu, n = ref >> 24;
                      for (u32 j = 0; j < n; j++) {
                        const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
                        need_words++;
                        if (!(w & 1u)) {
                          u32 len = visible(k, rv);
                          for (u32 e = 0; e < j; e++) { const u32 we = g_pay[off0 + e]; if ((we & 1u) && ((we >> 1) & 0x7FFFu) == k) len++; }
                          need_words += (len + 3u) / 4u;
                        }
                      }
                    } else { const u32 rid = ++node_msgid; sl[SK_HDR] = 1u | (4u << 8); sl[SK_RPC] = rid; out_msg(D_LIN, M_READ, 0, rid); }   // :230-234
                  } else {   // getRoot (:112-116)
                    root_v = qtype == M_READ_OK ? qa : 0u;
                    start_attempt(sl, si);
                  }
                }
              }
            } break;   // no handler under that id: ignored (node.js:152-156)
            default: break;
          }
        } else if (is_lin) {   // lin-kv over the key "root" (service.clj:31-61)
          svc_rep = true; o_to = qsrc; o_b = qb;
          if (qtype == M_READ) {
            if (!root_exists) { o_type = M_ERROR; o_a = 20; } else { o_type = M_READ_OK; o_a = cur_v; }
          } else {   // cas with create_if_not_exists
            const u32 from = qa & 0xFFFFu, si = qa >> 16;
            if (root_exists && cur_v != from) { o_type = M_ERROR; o_a = 22; }
            else {
              const u32 *const sl = slot_of(qsrc, si);
              const u32 nk = sl[SK_NK], ref = sl[SK_REF], off0 = ref & 0xFFFFFFu, n = ref >> 24;
              u32 writes = 0; for (u32 j = 0; j < nk; j++) writes |= sl[SK_WR + j];
              root_exists = 1u;
              if (writes) {
                const u32 v = ++cur_v;
                const u32 nn = sl[SK_NNEW];
                for (u32 i = 0; i < nn; i++) { const u32 k = sl[SK_KEY + sl[SK_NORD + i]]; g_pos[k] = n_order++; g_first[k] = v; }
                for (u32 j = 0; j < nk; j++) if (sl[SK_WR + j]) { const u32 k = sl[SK_KEY + j], c = g_updn[k]; g_upd_v[k * mw1 + c] = v; g_upd_t[k * mw1 + c] = sl[SK_WRTID + j]; g_updn[k] = c + 1u; }
                for (u32 i = 0; i < n; i++) { const u32 w = g_pay[off0 + i];
                  if (w & 1u) { const u32 k = (w >> 1) & 0x7FFFu, c = g_kvn[k]; g_kv[k * mw + c] = ((w >> 16) & 0xFFu) | (v << 8); g_kvn[k] = c + 1u; } }
              }
              o_type = M_CAS_OK; o_a = 0;
            }
          }
        } else {   // lww-kv (service.clj:214-243 as written): merge-source, merge-dest, then the replica that serves the request
          svc_rep = true; o_to = qsrc; o_b = qb;
          svc_ctr += 2u;   // (merge-source and merge-dest are drawn and dropped)
          const u32 r = scale32(draw32(key, 12u /* S_SVC */, svc_ctr++), 2), tid = qa, tn = tid >> 20, ti = tid & 0xFFFFFu;
          unsigned char *const rp = g_rep + (size_t)tn * TC + ti;
          if (qtype == M_WRITE) { *rp = (unsigned char)r; o_type = M_WRITE_OK; o_a = tid; }
          else if (*rp == r) { o_type = M_READ_OK; o_a = tid; }
          else { o_type = M_ERROR; o_a = 20; }
        }
