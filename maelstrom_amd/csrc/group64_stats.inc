// group64_stats.inc — body fragment shared by the one-cluster-per-wavefront kernels (all but general, which folds a shorter range of the
// lanes' flags, colo, whose counters are wave-uniform and whose flags live in LDS, and wide), included after the round loop: the last
// partial block of rows from the staging ring to HBM, the cluster's message counters and flags, its net stats and meta record.  Uses the
// kernel's names: stage, g_rows, n_rows, s_send_cl, s_send_sv, s_recv_cl, s_recv_sv, my_flags, flags, lane, p, inst, n_payload, rounds,
// jcap, n_ev.
  // ---- epilogue ----
  __syncthreads();
  {
    const u32 blk = n_rows >> 6;
    const u32 gi = blk * 64 + lane;
    if (gi < n_rows) reinterpret_cast<uint4 *>(g_rows)[gi] = stage[gi % STAGE_ROWS];
  }
  const u32 t_send_cl = wave_sum(s_send_cl), t_send_sv = wave_sum(s_send_sv);
  const u32 t_recv_cl = wave_sum(s_recv_cl), t_recv_sv = wave_sum(s_recv_sv);
  for (u32 b = 1; b <= MSIM_FLAG_ARENA_OVERRUN; b <<= 1) if (__ballot((my_flags & b) != 0)) flags |= b;
  if (lane == 0) {
    msim_net_stats st;
    st.all_send = (u64)t_send_cl + t_send_sv; st.all_recv = (u64)t_recv_cl + t_recv_sv;
    st.clients_send = t_send_cl; st.clients_recv = t_recv_cl;
    st.servers_send = t_send_sv; st.servers_recv = t_recv_sv;
    p.stats[inst] = st;
    msim_inst_meta m; m.n_rows = n_rows; m.n_payload_words = n_payload; m.flags = flags; m.n_rounds = rounds;
    m.n_events = jcap ? n_ev : 0; m.reserved[0] = 0; m.reserved[1] = 0; m.reserved[2] = 0;
    p.meta[inst] = m;
  }
