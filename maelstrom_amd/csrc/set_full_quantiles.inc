// set_full_quantiles.inc — QUANT_Q[0..4] = the quantiles {0 .5 .95 .99 1} of the QUANT_N latencies of QUANT_ARR[0 .. v_lat) that are not
// NOLAT: the idx-th smallest by bisection on the value.  Text included by set_full_body.inc, once per latency array (a lambda or a loop
// over the arrays changes what check_kernel compiles to); lane, v_lat and c_wave_sum are the body's.
  if (QUANT_N) {
    u32 lmax = 0;  // the search range is [0, largest latency]
    for (u32 e = lane; e < v_lat; e += 64) { const u32 l = QUANT_ARR[e]; if (l != NOLAT) lmax = max(lmax, l); }
    for (int o = 32; o; o >>= 1) lmax = max(lmax, (u32)__shfl_xor((int)lmax, o));
    const double pts[5] = {0.0, 0.5, 0.95, 0.99, 1.0};
    for (int qi = 0; qi < 5; qi++) {
      const u32 want = min(QUANT_N - 1, (u32)floor((double)QUANT_N * pts[qi]));
      u32 lo = 0, hi = lmax;  // smallest v with count(lat <= v) > want
      while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2;
        u32 c = 0;
        for (u32 e = lane; e < v_lat; e += 64) { const u32 l = QUANT_ARR[e]; c += (l != NOLAT && l <= mid) ? 1u : 0u; }
        if (c_wave_sum(c) > want) hi = mid; else lo = mid + 1;
      }
      QUANT_Q[qi] = lo;
    }
  }
#undef QUANT_ARR
#undef QUANT_N
#undef QUANT_Q
