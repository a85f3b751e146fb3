// dt_reads.inc — the completed transactions of this round in the payload area: `incl` is the kernel's prefix sum of need_words over the lanes
// of the cluster, `total` its last value; each node writes its own (reply_txn_ok() of dt_node.inc sized it): the appends as they are, a read
// as the key's elements visible at the version read + the transaction's own earlier appends.
        if (total) {
          if (n_payload + total > max_pay) { flags |= MSIM_FLAG_PAYLOAD_OVERFLOW; if (need_words) r_a = 0; }
          else {
            if (need_words) {
              const u32 off0 = done_ref & 0xFFFFFFu, n = done_ref >> 24;
              u32 pp = n_payload + incl - need_words;
              r_a = pp | (need_words << 24);
              for (u32 j = 0; j < n; j++) {
                const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
                if (w & 1u) { g_pay[pp++] = w; continue; }
                const u32 vis = visible(k, done_rv);
                u32 e = 0, acc = 0;
                const u32 hdr = pp++;
                for (u32 i = 0; i < vis; i++) { acc |= (g_kv[k * mw + i] & 0xFFu) << (8 * (e & 3)); if ((++e & 3) == 0) { g_pay[pp++] = acc; acc = 0; } }
                for (u32 i = 0; i < j; i++) { const u32 wi = g_pay[off0 + i];
                  if ((wi & 1u) && ((wi >> 1) & 0x7FFFu) == k) { acc |= ((wi >> 16) & 0xFFu) << (8 * (e & 3)); if ((++e & 3) == 0) { g_pay[pp++] = acc; acc = 0; } } }
                if (e & 3) g_pay[pp++] = acc;
                g_pay[hdr] = (k << 1) | ((e ? e : 0xFFu) << 16);  // a key without elements reads nil
              }
            }
            n_payload += total;
          }
        }
