// group16_phase.inc — body fragment shared by the four-clusters-per-wavefront kernels (raft4.hip, svc4.hip, txng4.hip, dtg4.hip), included
// at the top of the round: the busy clients of the cluster (busy_mask), the phase transitions that take no time (a cluster whose phase is
// done stops), the round limit.  Uses the kernel's names: busy, alive, phase, rate, gen_next, nem_next, cutoff, T, p, next_msg_id,
// loss_on, worker_mask, rounds, round_limit, flags, GB.
    const u32 busy_mask = GB(busy);

    // ---- time-free phase transitions: lin-kv has no final generator (core.clj:74-80 applies only with one) ----
    if (__ballot(alive && !(phase == PH_MAIN && ((rate > 0 && gen_next < cutoff) || (NEM && nem_next < cutoff))))) {
      for (;;) {
        bool ch = false;
        if (alive) {
          if (phase == PH_INIT_WAIT && !busy_mask) { phase = PH_MAIN_START; ch = true; }
          if (phase == PH_MAIN_START) { cutoff = T + p.cfg.time_limit_ms * 1000u; gen_next = T; nem_next = T; next_msg_id = 0; loss_on = 1; phase = PH_MAIN; ch = true; }
          if (phase == PH_MAIN && !((rate > 0 && gen_next < cutoff) || (NEM && nem_next < cutoff)) && !(rate == 0 && T < cutoff)) { phase = PH_DRAIN; ch = true; }
          if (phase == PH_DRAIN && !(busy_mask & worker_mask)) { phase = PH_DONE; ch = true; }
        }
        if (!__ballot(ch)) break;
      }
      if (phase == PH_DONE) alive = false;
      if (!__ballot(alive)) break;
    }
    if (alive && ++rounds > round_limit) { flags |= MSIM_FLAG_ROUND_LIMIT; alive = false; }
