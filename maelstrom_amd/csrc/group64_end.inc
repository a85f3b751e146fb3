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
