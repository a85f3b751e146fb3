// group8_time.inc — body fragment shared by the eight-clusters-per-wavefront kernels, included after the phase transitions of the round:
// R0 — when the cluster's scheduler is due (the nemesis, the generator with a free worker, the end of the time limit; a kernel with phases of
// its own adds their due times after the include) and this lane's next event, my_t (its committed envelope), to which a kernel adds its own
// timers before group8_jump.inc.  Uses the kernel's names: rate, gen_next, nem_next, cutoff, all_nodes, busy_mask, phase, T, deliver_at.
    // ---- R0: time ----
    const bool gen_live = rate > 0 && gen_next < cutoff;
    const bool nem_live = NEM && nem_next < cutoff;
    const u32 free_mask = all_nodes & ~busy_mask;
    u32 due = INF;
    if (phase == PH_INIT) due = T;
    else if (phase == PH_MAIN) {
      if (nem_live) due = max(nem_next, T);
      if (gen_live && free_mask) due = min(due, max(gen_next, T));
      if (rate == 0 && !nem_live) due = min(due, cutoff);
    }
    u32 my_t = deliver_at;
