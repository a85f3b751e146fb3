// group8_jump.inc — body fragment shared by the eight-clusters-per-wavefront kernels, included after group8_time.inc (and the kernel's
// own timers): when nothing of the cluster is due now, time jumps to its earliest event — a lane's my_t, a client's reply timeout, the
// scheduler's due time; a jump to a timeout makes this a timeout round.  Uses the kernel's names: GS, my_t, due, alive, T, busy,
// timeout_at, flags, GB.
    bool timeout_round = false;
    {
      const bool none_due = GB(my_t <= T) == 0;
      const bool jump = alive && due > T && none_due;
      if (__ballot(jump)) {
        u32 k = my_t == INF ? INF : my_t * 2;
        if (busy) k = min(k, timeout_at * 2 + 1);
        u32 km = g8_min<GS>(k);
        if (due != INF) km = min(km, due * 2);
        if (jump) {
          if (km == INF) { flags |= MSIM_FLAG_ROUND_LIMIT; alive = false; }
          else { timeout_round = (km & 1) != 0; T = max(T, km >> 1); }
        }
      }
    }
