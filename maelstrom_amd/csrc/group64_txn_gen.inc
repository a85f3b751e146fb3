// group64_txn_gen.inc — body fragment shared by the eight transactional one-cluster-per-wavefront kernels (dt, dtg, hat, hatg, mk, mkg,
// txn, txng), included in R1 where the generator has picked a free worker: the transaction of [upstream] elle's list-append / rw-register
// generator — n_mops micro-ops over the active keys, written to the payload area by lane 0, which owns the key pool in `gen` (active[16],
// next_val[16], next_key); a key that has had its max_writes_per_key appends is replaced by a fresh one.  `bad` is the overflow flag to
// stop on, the same in every lane.  Uses the kernel's names: key, kk, p, n_payload, max_pay, g_pay, gen, mw, lane.
              const u32 n_mops = 1 + scale32((u32)(draw64(key, S_GEN2, kk) >> 32), p.cfg.max_txn_length);
              u32 bad = 0;
              if (n_payload + n_mops > max_pay) bad = MSIM_FLAG_PAYLOAD_OVERFLOW;
              else if (lane == 0) {
                const u32 kc = p.cfg.key_count;
                for (u32 j = 0; j < n_mops; j++) {
                  const u64 h3 = draw64(key, S_GEN3, (u64)kk * 8 + j);
                  const u32 x = scale32((u32)(h3 >> 32), (1u << kc) - 1) + 1;
                  const u32 ki = 31 - (u32)__clz((int)x);
                  const u32 k = gen[ki];
                  if (h3 & 1) {
                    const u32 v = gen[16 + ki];
                    gen[16 + ki] = v + 1;
                    g_pay[n_payload + j] = 1u | (k << 1) | (v << 16);
                    if (v + 1 > mw) {
                      const u32 nk = gen[32];
                      if (nk >= p.cfg.max_values) { bad = MSIM_FLAG_VALUES_OVERFLOW; break; }
                      gen[ki] = nk; gen[32] = nk + 1; gen[16 + ki] = 1;
                    }
                  } else g_pay[n_payload + j] = (k << 1) | (0xFFu << 16);
                }
              }
              bad = rdlane(bad, 0);
