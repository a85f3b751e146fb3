// txn_lin.inc — the lin-kv lane of the single-root txn-list-append cluster (service.clj:31-61 over the key "root") with one request qtype, qa
// from qsrc, after the kernel has addressed the answer: read, and cas with create_if_not_exists, which commits the sender's transaction to
// the append log at the new version.  Included in txn_kernel<>, txng_kernel<> and txng4_kernel<>; the answer goes to rep_type / rep_a.  The
// kernel supplies TXN_REF_OF(node, i), the transaction (payload offset | micro-ops << 24) of that node's request handler i.
          if (qtype == M_READ) {
            if (root == V_NIL) { rep_type = M_ERROR; rep_a = 20; } else { rep_type = M_READ_OK; rep_a = root; }
          } else {  // cas with create_if_not_exists
            const u32 from = qa & 0xFFFFu, i = qa >> 16;
            if (root != V_NIL && root != from) { rep_type = M_ERROR; rep_a = 22; }
            else {
              const u32 base = root == V_NIL ? 0u : root;
              const u32 ref = TXN_REF_OF(qsrc, i), off0 = ref & 0xFFFFFFu, n = ref >> 24;
              u32 na = 0;
              for (u32 j = 0; j < n; j++) na += g_pay[off0 + j] & 1;
              for (u32 j = 0; j < n; j++) {
                const u32 w = g_pay[off0 + j];
                if (w & 1) { const u32 k = (w >> 1) & 0x7FFFu; const u32 c = g_kvn[k]; g_kv[k * mw + c] = ((w >> 16) & 0xFFu) | ((base + na) << 8); g_kvn[k] = c + 1; }
              }
              root = base + na;
              rep_type = M_CAS_OK; rep_a = 0;
            }
          }
