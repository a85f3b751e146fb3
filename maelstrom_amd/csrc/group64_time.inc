// group64_time.inc — body fragment shared by the one-cluster-per-wavefront kernels of group64_phase.inc, included after it: R0 — when the
// scheduler is due (the nemesis, the generator with a free worker, the end of the time limit) and this lane's next event, my_t (its
// committed envelope), to which a kernel adds its own timer before group64_jump.inc.  Uses the kernel's names: rate, gen_next, nem_next,
// cutoff, worker_mask (all_nodes where lane i is node i and its client), busy_mask, phase, T, deliver_at, NOTHING_COMMITTED.
    // ---- R0: time ----
    const bool gen_live = rate > 0 && gen_next < cutoff;
    const bool nem_live = NEM && nem_next < cutoff;
    const auto free_mask = worker_mask & ~busy_mask;
    u32 due = INF;
    switch (phase) {
      case PH_INIT: due = T; break;
      case PH_MAIN:
        if (nem_live) due = max(nem_next, T);
        if (gen_live && free_mask) due = min(due, max(gen_next, T));
        if (rate == 0 && !nem_live) due = min(due, cutoff);
        break;
      default: break;
    }
    u32 my_t = COMMITTED_AT;
