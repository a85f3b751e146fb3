// dt_input.inc — one input of the Datomic-style transactor cluster: a node's input switch, the lin-kv lane (root read / write, the
// self-contained cas) and the lww-kv lane.  Included where the kernel has taken the envelope apart into qtype, qa, qb, qsrc; dt_node.inc has
// the node's lambdas and says what the kernel supplies.
        if (is_node) {
          const u32 st = cu[DC_STAGE];
          switch (qtype) {
            case M_INIT:
              if (NODE_IX != 0u) { REPLY_OK(M_INIT_OK, CLIENT_REF(qb, qsrc)); break; }
              {   // the first node writes the initial state (:337-345): Tree.empty, then the root pointer
                u32 *const r = g_rec;
                r[0] = (128u << 16); r[1] = 0; r[2] = 0; __hip_atomic_store(r + 3, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u32 rid = ++node_msgid;
                cu[DC_STAGE] = DS_INIT_LEAF; cu[DC_CMSG] = CLIENT_REF(qb, qsrc); cu[DC_RPC] = rid;
                send1(D_LWW, M_WRITE, 0, rid);
              } break;
            case M_TXN:
              if (st == DS_IDLE) start_txn(CLIENT_REF(qb, qsrc), qa);
              else wq_push(CLIENT_REF(qb, qsrc), qa);
              break;
            case M_READ_OK: case M_WRITE_OK: case M_CAS_OK: case M_ERROR:
              switch (st) {
                case DS_INIT_LEAF:
                  if (qb != cu[DC_RPC]) break;
                  { const u32 rid = ++node_msgid; cu[DC_STAGE] = DS_INIT_ROOT; cu[DC_RPC] = rid; send1(D_LIN, M_WRITE, 0, rid); }
                  break;
                case DS_INIT_ROOT:
                  if (qb != cu[DC_RPC]) break;
                  cu[DC_STAGE] = DS_IDLE; REPLY_OK(M_INIT_OK, cu[DC_CMSG]);
                  break;
                case DS_ROOT:
                  if (qb != cu[DC_RPC]) break;
                  if (qtype != M_READ_OK) { REPLY_ERROR(14, cu[DC_CMSG]); unlock(); break; }   // "Unsure how to handle" (:364)
                  cu[DC_P1] = qa; cu[DC_T] = qa; cu[DC_PSTART] = next_p + 1u;
                  { const u32 *const rr = rec_of(qa); const u32 rv2 = rr[2], rw3 = __hip_atomic_load(rr + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); cu[DC_RV] = rv2; if ((rw3 >> (2u + NODE_IX)) & 1u) apply(); else load(qa); }
                  break;
                case DS_LOAD:
                  if (qb != cu[DC_RPC]) break;
                  if (qtype == M_READ_OK) { atomicOr(rec_of(cu[DC_TARGET]) + 3, 1u << (2u + NODE_IX)); apply(); }   // @@cache[ptr] = tree (:95)
                  else load(cu[DC_TARGET]);   // "Retrying read of tree node" (:97)
                  break;
                case DS_SAVE:
                  if (qb < cu[DC_WLO] || qb >= cu[DC_WLO] + cu[DC_WN]) break;
                  { const u32 left = cu[DC_WOUT] - 1u; cu[DC_WOUT] = left;
                    if (left == 0u) { const u32 rid = ++node_msgid; cu[DC_STAGE] = DS_CAS; cu[DC_RPC] = rid;   // advance_root! (:376-388): cas root from the pointer read to the new one
                      { u32 *const ce = g_cas + ((size_t)NODE_IX * DT_CASQ + (casn++ % DT_CASQ)) * 3u; ce[0] = rid; ce[1] = cu[DC_P1]; ce[2] = cu[DC_REF]; }
                      send1(D_LIN, M_CAS, cu[DC_T], rid); wait_until = T + DT_AWAIT_US; } }
                  break;
                case DS_CAS:
                  if (qb != cu[DC_RPC]) break;
                  if (qtype == M_CAS_OK) reply_txn_ok();
                  else REPLY_ERROR(30, cu[DC_CMSG]);   // txn_conflict (:385)
                  unlock();
                  break;
                default: break;   // "Ignoring reply ... with no callback" (node.rb:160-162)
              }
              break;
            default: break;
          }
        } else if (is_lin) {   // lin-kv over the key "root" (service.clj:31-61)
          svc_rep = true; o_to = qsrc; o_b = qb;
          if (qtype == M_READ) {
            if (!root_exists) { o_type = M_ERROR; o_a = 20; } else { o_type = M_READ_OK; o_a = root; }
          } else if (qtype == M_WRITE) { root = qa; root_exists = 1u; o_type = M_WRITE_OK; o_a = 0; }
          else {   // cas, no create_if_not_exists.  The request is self-contained (:376-388): its `from` and its transaction come from the sender's
            // table of cas requests under the msg_id, not from what the sender holds NOW (it may have given up on this cas and moved on)
            u32 c_from = 0, c_ref = 0; bool c_hit = false;
            { const u32 *const ce = g_cas + (size_t)qsrc * DT_CASQ * 3u;
#pragma unroll
              for (u32 i = 0; i < DT_CASQ; i++) { const u32 e0 = ce[3u * i], e1 = ce[3u * i + 1u], e2 = ce[3u * i + 2u]; if (e0 == qb) { c_hit = true; c_from = e1; c_ref = e2; } } }
            if (!c_hit) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; o_type = M_ERROR; o_a = 22; }   // engine capacity: DT_CASQ outstanding cas requests per node
            else if (!root_exists) { o_type = M_ERROR; o_a = 20; }
            else if (root != c_from) { o_type = M_ERROR; o_a = 22; }
            else {
              const u32 ref = c_ref, off0 = ref & 0xFFFFFFu, n = ref >> 24, v = ++cur_v;
              root = qa;
              for (u32 i = 0; i < n; i++) { const u32 w = g_pay[off0 + i];
                if (w & 1u) { const u32 k = (w >> 1) & 0x7FFFu, c = g_kvn[k]; if (g_first[k] == DT_NONE) g_first[k] = v;
                  g_kv[k * mw + c] = ((w >> 16) & 0xFFu) | (v << 8); g_kvn[k] = c + 1u; } }
              o_type = M_CAS_OK; o_a = 0;
            }
          }
        } else {   // lww-kv (service.clj:214-243 as written): merge-source, merge-dest, then the replica that serves the request
          svc_rep = true; o_to = qsrc; o_b = qb;
          svc_ctr += 2u;
          const u32 r = scale32(draw32(key, 12u /* S_SVC */, svc_ctr++), 2);
          u32 *const rp = rec_of(qa) + 3;   // (the replica bits; the nodes set their "loaded" bits in the same word: atomics)
          if (qtype == M_WRITE) { atomicAnd(rp, ~3u); atomicOr(rp, r); o_type = M_WRITE_OK; o_a = qa; }
          else if ((__hip_atomic_load(rp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 3u) == r) { o_type = M_READ_OK; o_a = qa; }
          else { o_type = M_ERROR; o_a = 20; }
        }
