// group64_phase.inc — body fragment shared by the one-cluster-per-wavefront kernels whose run is init, main phase and drain (dt, dtg, hat,
// hatg, mk, mkg, raft, svc, txn, txng; the kernels with final-read, sleep or final-poll phases keep their loops), included at the top of
// the round: the busy clients (busy_mask), the phase transitions that take no time, the round limit.  A drain ends when no WORKER is busy
// (WORKERS_OF, group64_net.inc).  Uses the kernel's names: busy, phase, rate, gen_next, nem_next, cutoff, T, p, next_msg_id, loss_on,
// rounds, flags.
    const auto busy_mask = WB(busy);

    // ---- time-free phase transitions ----
    if (!(phase == PH_MAIN && ((rate > 0 && gen_next < cutoff) || (NEM && nem_next < cutoff)))) {
      for (bool again = true; again;) {
        again = false;
        switch (phase) {
          case PH_INIT_WAIT: if (!busy_mask) { phase = PH_MAIN_START; again = true; } break;
          case PH_MAIN_START:
            cutoff = T + p.cfg.time_limit_ms * 1000u; gen_next = T; nem_next = T;
            next_msg_id = 0; loss_on = 1; phase = PH_MAIN; again = true; break;
          case PH_MAIN: {
            const bool gl = rate > 0 && gen_next < cutoff, nl = NEM && nem_next < cutoff;
            if (gl || nl) break;
            if (rate == 0 && T < cutoff) break;
            phase = PH_DRAIN; again = true;
          } break;
          case PH_DRAIN: if (!WORKERS_OF(busy_mask)) { phase = PH_DONE; again = true; } break;  // no final phase
          default: break;
        }
      }
      if (phase == PH_DONE) break;
    }
    if (++rounds > ROUND_LIMIT) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }
