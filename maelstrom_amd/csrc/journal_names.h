// journal_names.h — how the net journal's endpoints and message types are spelled, for the host-side writers of the journal
// (fressian.cpp, journal_svg.cpp).  Host only.
#ifndef MSIM_JOURNAL_NAMES_H
#define MSIM_JOURNAL_NAMES_H

#include <cstdio>
#include <string>

#include "../../include/maelsim.h"

namespace journal_names {

// endpoints behind the client slots are services (service.clj:290-296): the proxy's is the one it was pointed at, the single-root
// transactional node uses lin-kv, the multi-key one lin-kv then lww-kv
inline std::string endpoint(uint32_t e, uint32_t n_nodes, uint32_t slots, const msim_config *cfg) {
  char b[16];
  if (e < n_nodes) std::snprintf(b, sizeof b, "n%u", e);
  else if (e < n_nodes + slots) std::snprintf(b, sizeof b, "c%u", e - n_nodes);
  else {
    const char *name = "lin-kv";
    if (cfg->node_program == MSIM_NODE_LIN_KV_PROXY) name = cfg->proxy_service == MSIM_SVC_SEQ_KV ? "seq-kv" : cfg->proxy_service == MSIM_SVC_LWW_KV ? "lww-kv" : "lin-kv";
    else if ((cfg->node_program == MSIM_NODE_TXN_MULTI_KEY || cfg->node_program == MSIM_NODE_TXN_DATOMIC) && e == n_nodes + slots + 1) name = "lww-kv";
    else if (cfg->node_program == MSIM_NODE_TSO_IDS) name = "lin-tso";
    std::snprintf(b, sizeof b, "%s", name);
  }
  return b;
}

const char *const MSG_TYPES[] = {"", "init", "init_ok", "topology", "topology_ok", "echo", "echo_ok", "broadcast", "broadcast_ok", "read", "read_ok",
                                 "add", "add_ok", "replicate", "write", "write_ok", "cas", "cas_ok", "error", "request_vote", "request_vote_res",
                                 "append_entries", "append_entries_res", "txn", "txn_ok", "generate", "generate_ok", "replicate_ack", "ts", "ts_ok",
                                 "send", "send_ok", "poll", "poll_ok", "list_committed_offsets", "list_committed_offsets_ok", "commit_offsets", "commit_offsets_ok",
                                 "broadcast_many", "broadcast_many_ok"};

}  // namespace journal_names

#endif
