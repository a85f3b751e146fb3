// group64_nemesis.inc — body fragment shared by the one-cluster-per-wavefront kernels (all but sim_kernel_wide.inc, whose node masks are
// wider than a word), included in R1 (scheduler) under `case PH_MAIN`: the partition nemesis' flip-flop (nemesis.clj:10-16 + [upstream]
// jepsen.nemesis.combined/partition-package: one / majority / majorities-ring / minority-third grudges drawn per start, the shuffle done
// by lane 0 in `misc`), its two history rows and the payload words of the grudge.  group8_nemesis.inc with `act` true and `l` = lane is other
// device code for the NEM instantiations (tried on txn_kernel<>: its start / stop goes through ballots of `act` that a whole-wavefront
// cluster does not need, and it orders the shuffle in `misc` with wave_lds_fence() where these kernels use __syncthreads()), so the text
// these kernels had stays a fragment of its own.  Uses the kernel's names: nem_live, nem_next, nem_j, nem_rows,
// nem_f, nem_v1, nem_v2, nem_len2, part, misc, lane, N, all_nodes, is_node, key, T, n_payload, max_pay, g_pay, flags, p.
            if (NEM && nem_live && nem_next <= T) {  // flip-flop start/stop (nemesis.clj:10-16 + [upstream] partition package)
              const u32 j = nem_j++;
              nem_rows = 2;
              if ((j & 1) == 0) {
                const u32 spec = scale32(draw32(key, S_NEM_SPEC, j), 4);
                if (lane < N) misc[lane] = lane;
                __syncthreads();
                if (lane == 0 && spec != MSIM_SPEC_ONE) {
                  for (u32 i = N - 1; i >= 1; i--) {
                    const u32 kk = scale32(draw32(key, S_NEM_SHUFFLE, ((u64)j << 16) | i), i + 1);
                    const u32 t = misc[i]; misc[i] = misc[kk]; misc[kk] = t;
                  }
                }
                __syncthreads();
                u32 my_part = 0;
                if (is_node) {
                  if (spec == MSIM_SPEC_ONE) {
                    const u32 loner = scale32(draw32(key, S_NEM_PICK, j), N);
                    my_part = lane == loner ? (all_nodes & ~(1u << loner)) : (1u << loner);
                  } else if (spec == MSIM_SPEC_MAJORITY || spec == MSIM_SPEC_MINORITY_THIRD) {
                    const u32 cnt = spec == MSIM_SPEC_MAJORITY ? N / 2 : (N - 1) / 3;
                    u32 comp = 0;
                    for (u32 i = 0; i < cnt; i++) comp |= 1u << misc[i];
                    my_part = ((comp >> lane) & 1) ? (all_nodes & ~comp) : comp;
                  } else {
                    const u32 m = N / 2 + 1;
                    u32 pos = 0;
                    for (u32 i = 0; i < N; i++) if (misc[i] == lane) pos = i;
                    const u32 i0 = (pos + N - (m / 2) % N) % N;
                    u32 vis = 0;
                    for (u32 kk = 0; kk < m; kk++) vis |= 1u << misc[(i0 + kk) % N];
                    my_part = all_nodes & ~vis;
                  }
                }
                part |= my_part;
                const u32 words = N * MSIM_MASK_WORDS;
                u32 off = 0;
                if (n_payload + words > max_pay) flags |= MSIM_FLAG_PAYLOAD_OVERFLOW;
                else {
                  off = n_payload; n_payload += words;
                  if (is_node) { g_pay[off + lane * 4] = part; g_pay[off + lane * 4 + 1] = 0; g_pay[off + lane * 4 + 2] = 0; g_pay[off + lane * 4 + 3] = 0; }
                }
                nem_f = MSIM_F_START_PARTITION; nem_v1 = spec; nem_v2 = off; nem_len2 = words;
              } else {
                part = 0;
                nem_f = MSIM_F_STOP_PARTITION; nem_v1 = MSIM_NO_VALUE; nem_v2 = MSIM_NO_VALUE; nem_len2 = 0;
              }
              nem_next = T + __umulhi(draw32(key, S_NEM_STAGGER, j), p.nem_period2_us);
            }
