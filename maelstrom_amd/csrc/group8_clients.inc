// group8_clients.inc — body fragment shared by all eight eight-clusters-per-wavefront kernels, included after the COMMIT of the round: the
// clients' recv! loops (client.clj:94-107) — queued (stale, older) envelopes first, then the fresh reply of this round; an envelope that
// finds nobody in recv! waits in the client's inbox (CQ envelopes in LDS, up.client_spill more in HBM).  Uses the kernel's names:
// c_arr, ca_y, ca_a, ca_b, busy, normal, cin_n, csp_n, my_cq, my_cspill, up, client_deliver, my_flags, T, l.
      // ---- R4: the clients' recv! loops (client.clj:94-107) ----
      if (__ballot(c_arr || (busy && (cin_n | csp_n) != 0))) {
        for (;;) {
          const bool stale = normal && busy && (cin_n | csp_n) != 0;
          const bool fresh = normal && !stale && busy && c_arr;
          if (!__ballot(stale || fresh)) break;
          if (stale) {
            u32 best = 0; bool in_spill = false;
            uint2 bk = make_uint2(INF, INF);
            for (u32 i = 0; i < cin_n; i++) {
              const uint2 kk = *reinterpret_cast<const uint2 *>(&my_cq[i * 64u]);
              if (kk.x < bk.x || (kk.x == bk.x && kk.y < bk.y)) { bk = kk; best = i; }
            }
            for (u32 i = 0; i < csp_n; i++) {
              const uint2 kk = *reinterpret_cast<const uint2 *>(&my_cspill[i]);
              if (kk.x < bk.x || (kk.x == bk.x && kk.y < bk.y)) { bk = kk; best = i; in_spill = true; }
            }
            uint4 e;
            if (in_spill) { e = my_cspill[best]; csp_n--; if (best != csp_n) my_cspill[best] = my_cspill[csp_n]; }
            else { e = my_cq[best * 64u]; cin_n--; if (best != cin_n) my_cq[best * 64u] = my_cq[cin_n * 64u]; }
            client_deliver(e.y & 0xFFu, e.z, e.w & 0xFFFFFFu);
          } else if (fresh) {
            c_arr = false;
            client_deliver(ca_y & 0xFFu, ca_a, ca_b);
          }
        }
        if (c_arr && normal) {  // nobody is in recv!: the envelope waits for the next RPC (and is skipped there as stale)
          const uint4 e = make_uint4(T, ca_y, ca_a, ca_b | (l << 24));
          if (cin_n < CQ) { my_cq[cin_n * 64u] = e; cin_n++; }
          else if (csp_n < up.client_spill) my_cspill[csp_n++] = e;
          else my_flags |= MSIM_FLAG_INBOX_OVERFLOW;
        }
      }
    }

