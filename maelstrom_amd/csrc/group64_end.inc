// group64_end.inc — included after a one-cluster-per-wavefront kernel that took group64_net.inc: forgets the names the kernel gave the
// fragments and those group64_net.inc derived from them, so that the next kernel of the unit states its own.
#undef PAYS_LATENCY
#undef POLL_LANE
#undef ENDPOINT_LANES
#undef COMMIT_FLAG
#undef OWN_JWRITE
#undef WB
#undef WPOP
#undef WLT
#undef WORKERS_OF
#undef NOTHING_COMMITTED
#undef COMMITTED_AT
// ... and what it told its program's fragments (dt_*.inc, mk_*.inc, hat_node.inc, kafka_*.inc, txn_lin.inc, list_append_client.inc)
#undef CLIENT_REF
#undef REPLY_OK
#undef REPLY_ERROR
#undef NODE_IX
#undef DT_WAIT_RING
#undef MK_NSLOTS
#undef KF_NSLOTS
#undef REPLY_TO
#undef TXN_REF_OF
#undef CRASH_STRIDE
#undef NODE_GIVES_UP
#undef OWN_CLIENT_DELIVER
