// kafka_svc.inc — the lin-kv lane of the kafka cluster (service.clj:31-61 over the chunk keys and "offsets") with one request qtype, qa, qb
// from qsrc: read, and cas with create_if_not_exists; the commit of offsets reads the sender's handler table and the blocks the nodes have finished.
        svc_rep = true; o_dest = qsrc; o_b = qb;
        if (qtype == M_READ) {
          if (qa & KF_OFFSETS_KEY) { if (off_exists) { o_type = M_READ_OK; o_a = off_ver; } else { o_type = M_ERROR; o_a = 20; } }
          else { const u32 c = chunk_count(qa & 7u, qa >> 8); if (c) { o_type = M_READ_OK; o_a = c; } else { o_type = M_ERROR; o_a = 20; } }
        } else if (qtype == M_CAS) {
          if (qa & KF_OFFSETS_KEY) {
            const u32 from = qa & 0xFFFFu, i = (qa >> 16) & (2u * KF_NSLOTS - 1u);   // (the handler's index: KF_NSLOTS takes one bit less)
            if (off_exists && from != off_ver) { o_type = M_ERROR; o_a = 22; }   // (from {} never equals a stored map: they are not empty)
            else {
              // the value did not change since it was read (or the key is created): to = (merge-with max from (:offsets body))
              const u32 *sl = slots + (qsrc * KF_NSLOTS + i) * KSW;
              u32 pp = sl[1]; const u32 end = pp + KS_NK(sl[3]), newver = off_ver + 1u; bool changed = false;
              while (pp < end) {
                const u32 h = g_pay[pp], k_ = h & 7u, n = (h >> 8) & 0xFFu, o = h >> 16;
                pp += 1u + (n + 1u) / 2u;
                if (!n) continue;   // txn-offsets: only keys something was polled from
                const u32 hi = o + n - 1u, cur = committed_at(k_, off_ver);
                if (cur == 0 || hi > cur - 1u) { const u32 e = nupd[k_]; g_upd[(size_t)k_ * (cap + 1) + e] = (newver << 16) | hi; nupd[k_] = e + 1u; changed = true; }
              }
              off_exists = 1;
              if (changed) off_ver = newver;
              o_type = M_CAS_OK; o_a = 0;
            }
          } else {
            const u32 k_ = qa & 7u, ch = (qa >> 3) & 63u, from = (qa >> 9) & 31u, msg = qa >> 14;
            const u32 cur = chunk_count(k_, ch);
            if (cur != 0 && cur != from) { o_type = M_ERROR; o_a = 22; }
            else {   // the chunk is what was read, or does not exist (create_if_not_exists, :52-55): it becomes that + [msg]
              const u32 o = ch * KF_CHUNK + (cur ? from : 0u);
              if (o >= cap) { my_flags |= MSIM_FLAG_VALUES_OVERFLOW; o_type = M_ERROR; o_a = 22; }
              else { g_log[(size_t)k_ * cap + o] = msg; klen[k_] = o + 1u; o_type = M_CAS_OK; o_a = 0; }
            }
          }
        } else svc_rep = false;
