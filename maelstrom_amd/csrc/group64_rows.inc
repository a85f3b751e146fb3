// group64_rows.inc — body fragment shared by the one-cluster-per-wavefront kernels, included at the end of the round: the round's history
// rows in canonical order (nemesis rows, invocations in lane order, completions in lane order) into the staging ring in LDS, and every
// completed block of 64 rows from there to HBM as one coalesced 1 KiB append.  A kernel whose rows carry no length declares inv_len /
// cmp_len as constant zero.  sim_kernel_kafkag.inc (two passes: its final phase makes more rows in a round than the ring holds) and
// sim_kernel_wide.inc keep their own.  Uses the kernel's names: inv_row, inv_packed, inv_value, inv_len, cmp_row, cmp_packed, cmp_value,
// cmp_len, nem_rows, nem_f, nem_v1, nem_v2, nem_len2, n_rows, max_rows, g_rows, stage, flags, T, lane, WB, WPOP, WLT.
    // ---- history rows ----
    {
      const auto imask = WB(inv_row), cmask = WB(cmp_row);
      const u32 ni = WPOP(imask);
      const u32 nr = nem_rows + ni + WPOP(cmask);
      if (nr) {
        if (n_rows + nr > max_rows) { flags |= MSIM_FLAG_ROWS_OVERFLOW; break; }
        const u32 tlo = (u32)((u64)T * 1000ull), thi = (u32)(((u64)T * 1000ull) >> 32);
        if (NEM && nem_rows && lane == 0) {
          const u32 pk = MSIM_T_INFO | (nem_f << 2) | (MSIM_PROCESS_NEMESIS << 12);
          stage[n_rows % STAGE_ROWS] = make_uint4(tlo, thi, pk, nem_v1);
          stage[(n_rows + 1) % STAGE_ROWS] = make_uint4(tlo, thi | (nem_len2 << 16), pk, nem_v2);
        }
        if (inv_row) stage[(n_rows + nem_rows + WPOP(imask & WLT)) % STAGE_ROWS] = make_uint4(tlo, thi | (inv_len << 16), inv_packed, inv_value);
        if (cmp_row) stage[(n_rows + nem_rows + ni + WPOP(cmask & WLT)) % STAGE_ROWS] = make_uint4(tlo, thi | (cmp_len << 16), cmp_packed, cmp_value);
        const u32 new_n = n_rows + nr;
        if ((new_n >> 6) != (n_rows >> 6)) {  // a 64-row block completed
          __syncthreads();
          for (u32 blk = n_rows >> 6; blk < (new_n >> 6); blk++) {
            const u32 gi = blk * 64 + lane;
            if (gi < max_rows) reinterpret_cast<uint4 *>(g_rows)[gi] = stage[gi % STAGE_ROWS];
          }
          __syncthreads();
        }
        n_rows = new_n;
      }
    }
