// group64_jump.inc — body fragment shared by the one-cluster-per-wavefront kernels, included after group64_time.inc (or the kernel's own
// `due` and `my_t`) and the kernel's own timers: when nothing is due now, time jumps to the cluster's earliest event — a lane's my_t, a
// client's reply timeout, the scheduler's due time; a jump to a timeout makes this a timeout round, and a cluster with no event left
// stops.  Uses the kernel's names: my_t, due, T, busy, timeout_at, flags.
    bool timeout_round = false;
    if (due > T && !__ballot(my_t <= T)) {  // nothing due now: jump to the next event
      u32 k = my_t == INF ? INF : my_t * 2;
      if (busy) k = min(k, timeout_at * 2 + 1);
      u32 km = wave_min(k);
      if (due != INF) km = min(km, due * 2);
      if (km == INF) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }  // stuck
      timeout_round = (km & 1) != 0;
      T = max(T, km >> 1);
    }
