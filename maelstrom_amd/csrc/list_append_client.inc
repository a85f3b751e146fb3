// list_append_client.inc — the client of the txn-list-append kernels with one cluster per wavefront (txn, txng, mk, mkg, dt, dtg): how an
// operation completes and what the client's recv! does with one envelope (client.clj:94-107).  Included inside the round loop after the
// round's row variables (cmp_row, cmp_packed, cmp_value, cmp_len) are declared.  The kernel supplies
//   CRASH_STRIDE      what a crashed process's successor adds to its number: N with one worker per node, C with several
//   NODE_GIVES_UP     defined where the node answers with codes of its own besides the services': 0 (:timeout, not :definite?) and 14 (abort)
//   OWN_CLIENT_DELIVER  defined where the kernel spells recv! out itself and takes `complete` only (txng, dtg: the lambda is other device code there)
// group64_end.inc forgets them.
    auto complete = [&](u32 type, u32 err, u32 ref) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) my_flags |= MSIM_FLAG_ROUND_LIMIT; return; }
      cmp_row = true; cmp_packed = type | (MSIM_F_TXN << 2) | (err << 7) | (process << 12);
      cmp_value = ref & 0xFFFFFFu; cmp_len = ref >> 24;
      if (type == MSIM_T_INFO) process += CRASH_STRIDE;  // crashed process; the Reusable client itself lives on
    };
#ifndef OWN_CLIENT_DELIVER
    auto client_deliver = [&](u32 qtype, u32 qa, u32 qb) {
      s_recv_cl++;
      if (busy && qb == want) {  // else stale (client.clj:105-107)
        if (qtype == M_TXN_OK) complete(MSIM_T_OK, 0, qa);
        else if (qtype == M_ERROR)
#ifdef NODE_GIVES_UP
          if (qa == 0u) complete(MSIM_T_INFO, MSIM_ERR_TIMEOUT, c_value);   // code 0 :timeout is not :definite? (errors.edn:2-4)
          else complete(MSIM_T_FAIL, qa == 11 ? MSIM_ERR_TEMPORARILY_UNAVAILABLE : qa == 20 ? MSIM_ERR_KEY_DOES_NOT_EXIST : qa == 30 ? MSIM_ERR_TXN_CONFLICT : qa == 14 ? MSIM_ERR_ABORT : MSIM_ERR_PRECONDITION_FAILED, c_value);
#else
          complete(MSIM_T_FAIL, qa == 11 ? MSIM_ERR_TEMPORARILY_UNAVAILABLE : qa == 20 ? MSIM_ERR_KEY_DOES_NOT_EXIST : qa == 30 ? MSIM_ERR_TXN_CONFLICT : MSIM_ERR_PRECONDITION_FAILED, c_value);
#endif
        else complete(MSIM_T_OK, 0, c_value);  // init_ok
      }
    };
#endif
