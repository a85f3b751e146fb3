// kafka_node.inc — one input of a kafka node (demo/clojure/kafka.clj over lin-kv, specification: oracle/kafka_nodes.inc): the request handlers
// for send / poll / list_committed_offsets / commit_offsets, their chunk reads and cas through lin-kv, and the sizing of a poll_ok /
// list_committed_offsets_ok block.  Included in kafka_kernel<> and kafkag_kernel<> where the node has taken its envelope apart into qtype, qa,
// qb, qsrc; kafka_blocks.inc then lays the blocks out in the payload area and kafka_svc.inc is the lin-kv lane.  The client side differs by
// design and stays in each kernel.  In both a node's index is its lane.  The kernel supplies
//   KF_NSLOTS              request handlers in flight per node
//   REPLY_TO(cmsg)         starts the answer to the client that a stored client reference names (rep, o_b and where it goes)
//   CLIENT_REF(qb, qsrc)   how a client's msg_id is stored: qb where the client lives in its node's lane, qb | qsrc << 24 where it is an endpoint
// group64_end.inc forgets them.
        {
          // read the chunk of `offset` of key `k_` for handler `sl`
          auto read_chunk = [&](u32 *sl, u32 fl, u32 k_, u32 offset) {
            const u32 rid = ++node_msgid;
            sl[2] = rid; sl[3] = (fl & ~(7u << 6)) | (k_ << 6); sl[5] = offset;
            to_svc = true; o_type = M_READ; o_a = k_ | ((offset / KF_CHUNK) << 8); o_b = rid;
          };
          switch (qtype) {
            case M_INIT: REPLY_TO(CLIENT_REF(qb, qsrc)); o_type = M_INIT_OK; break;
            case M_SEND: case M_POLL: case M_LIST_OFFSETS: case M_COMMIT_OFFSETS: {
              u32 i = 0; while (i < KF_NSLOTS && KS_USED(my_slots[i * KSW + 3])) i++;
              if (i == KF_NSLOTS) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; break; }
              u32 *sl = my_slots + i * KSW;
              sl[0] = CLIENT_REF(qb, qsrc); sl[1] = 0; sl[4] = 0; sl[6] = 0; sl[7] = 0;
              if (qtype == M_SEND) {
                sl[4] = (qa >> 6) << 16;
                read_chunk(sl, KS_MAKE(KK_SEND, 1u, 0u, 0u, 0u), qa & 7u, my_cache[qa & 7u]);
              } else if (qtype == M_POLL) {
                const u32 nk = qa >> 24;
                if (nk == 0) { REPLY_TO(CLIENT_REF(qb, qsrc)); o_type = M_POLL_OK; o_a = 0; break; }   // no offsets: {:msgs {}}
                sl[1] = qa & 0xFFFFFFu;
                const u32 w = g_pay[qa & 0xFFFFFFu];
                read_chunk(sl, KS_MAKE(KK_POLL, 1u, 0u, 0u, nk), w & 7u, w >> 8);
              } else {
                const u32 rid = ++node_msgid;
                sl[1] = qa & 0xFFFFFFu; sl[2] = rid; sl[3] = KS_MAKE(qtype == M_LIST_OFFSETS ? KK_LIST : KK_COMMIT, 1u, 0u, 0u, qa >> 24);
                to_svc = true; o_type = M_READ; o_a = KF_OFFSETS_KEY; o_b = rid;   // get-offsets, :141-147
              }
            } break;
            case M_READ_OK: case M_CAS_OK: case M_ERROR: {
              u32 i = 0;
              while (i < KF_NSLOTS) { if (KS_USED(my_slots[i * KSW + 3]) && my_slots[i * KSW + 2] == qb) break; i++; }
              if (i == KF_NSLOTS) break;  // handle-reply!: no such rpc
              u32 *sl = my_slots + i * KSW;
              const u32 fl = sl[3], k_ = KS_KEY(fl), off = sl[5], base = off - off % KF_CHUNK;
              switch (KS_KIND(fl)) {
                case KK_SEND:
                  if (KS_STAGE(fl) == 1) {
                    const u32 cnt = qtype == M_READ_OK ? qa : 0u;   // (exceptionally [_] [])
                    my_cache[k_] = max(my_cache[k_], base + cnt);
                    if (cnt >= KF_CHUNK) { my_cache[k_] = max(my_cache[k_], base + KF_CHUNK); read_chunk(sl, fl, k_, my_cache[k_]); break; }   // chunk full: recur
                    const u32 rid = ++node_msgid;
                    sl[2] = rid; sl[3] = (fl & ~(3u << 4)) | (2u << 4); sl[4] = (sl[4] & 0xFFFF0000u) | cnt;
                    to_svc = true; o_type = M_CAS; o_a = k_ | ((off / KF_CHUNK) << 3) | (cnt << 9) | ((sl[4] >> 16) << 14); o_b = rid;
                  } else {
                    REPLY_TO(sl[0]);
                    if (qtype == M_CAS_OK) { const u32 o = base + (sl[4] & 0xFFFFu); my_cache[k_] = max(my_cache[k_], o + 1u); o_type = M_SEND_OK; o_a = o; }
                    else { o_type = M_ERROR; o_a = qa == 22 ? 30u : qa; }   // "cas conflict", :108-110
                    sl[3] = 0;
                  }
                  break;
                case KK_POLL: {
                  const u32 cnt = qtype == M_READ_OK ? qa : 0u, j = KS_J(fl), nk = KS_NK(fl);
                  my_cache[k_] = max(my_cache[k_], base + cnt);
                  sl[6 + (j >> 2)] |= cnt << (8u * (j & 3u));
                  if (j + 1 < nk) { const u32 w = g_pay[sl[1] + j + 1]; read_chunk(sl, (fl & ~(15u << 9)) | ((j + 1u) << 9), w & 7u, w >> 8); break; }
                  // poll_ok: sized here, written below (payload words are handed out in node order)
                  REPLY_TO(sl[0]); o_type = M_POLL_OK; done_slot = i;
                  for (u32 e = 0; e < nk; e++) {
                    const u32 w = g_pay[sl[1] + e], i0 = (w >> 8) % KF_CHUNK, c = (sl[6 + (e >> 2)] >> (8u * (e & 3u))) & 0xFFu;
                    const u32 n = c > i0 ? c - i0 : 0u;
                    need_words += 1u + (n + 1u) / 2u;
                  }
                } break;
                case KK_LIST:
                  REPLY_TO(sl[0]); o_type = M_LIST_OFFSETS_OK; done_slot = i;
                  sl[4] = qtype == M_READ_OK ? qa : KF_ABSENT;   // (exceptionally [res] {})
                  need_words = KS_NK(fl);
                  break;
                default:   // KK_COMMIT
                  if (KS_STAGE(fl) == 1) {
                    const u32 from = qtype == M_READ_OK ? qa : KF_ABSENT, rid = ++node_msgid;
                    sl[2] = rid; sl[3] = (fl & ~(3u << 4)) | (2u << 4); sl[4] = from;
                    to_svc = true; o_type = M_CAS; o_a = KF_OFFSETS_KEY | from | (i << 16); o_b = rid;
                  } else {
                    REPLY_TO(sl[0]);
                    if (qtype == M_CAS_OK) { o_type = M_COMMIT_OFFSETS_OK; o_a = 0; } else { o_type = M_ERROR; o_a = qa == 22 ? 30u : qa; }
                    sl[3] = 0;
                  }
                  break;
              }
            } break;
            default: break;
          }
        }
