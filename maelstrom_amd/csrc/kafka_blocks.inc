// kafka_blocks.inc — the poll_ok / list_committed_offsets_ok blocks of this round in the payload area: `incl` is the kernel's prefix sum of
// need_words over the lanes, `total` its last value; each node writes its own block (kafka_node.inc sized it).
        if (total) {
          const bool fits = n_payload + total <= max_pay;
          if (!fits) flags |= MSIM_FLAG_PAYLOAD_OVERFLOW;
          if (need_words) {
            u32 *sl = my_slots + done_slot * KSW;
            if (!fits) { rep = false; sl[3] = 0; }   // (the oracle drops the reply with the handler)
            else {
              const u32 fl = sl[3], nk = KS_NK(fl);
              u32 pp = n_payload + incl - need_words;
              o_a = pp | (need_words << 24);
              if (KS_KIND(fl) == KK_POLL) {
                for (u32 e = 0; e < nk; e++) {
                  const u32 w = g_pay[sl[1] + e], k_ = w & 7u, o = w >> 8, i0 = o % KF_CHUNK, c = (sl[6 + (e >> 2)] >> (8u * (e & 3u))) & 0xFFu;
                  const u32 n = c > i0 ? c - i0 : 0u;
                  g_pay[pp++] = k_ | (n << 8) | (o << 16);
                  for (u32 x = 0; x < n; x += 2) g_pay[pp++] = g_log[(size_t)k_ * cap + o + x] | (x + 1 < n ? g_log[(size_t)k_ * cap + o + x + 1] << 16 : 0u);
                }
              } else {
                const u32 ver = sl[4];
                for (u32 e = 0; e < nk; e++) {
                  const u32 k_ = g_pay[sl[1] + e] & 7u, c = ver == KF_ABSENT ? 0u : committed_at(k_, ver);
                  g_pay[pp++] = k_ | (c ? (((c - 1u) << 8) | 0x80000000u) : 0u);   // select-keys: only the keys the map has
                }
              }
              sl[3] = 0;
            }
          }
          if (fits) n_payload += total;
        }
