// journal.cpp — the net journal's messages on the host: msim_journal_messages_rows, the walk include/maelsim_journal.h states (the
// reference's net/viz.clj:27-56 `messages` and net/checker.clj:28-41 `basic-stats`, plus the delivery counts and latencies).  One
// sequential pass with a map id -> the latest send; exact for every journal, which is why journal_dev.hip hands it the journals that
// are not well-formed.  Host only: no device is touched.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/maelsim.h"

namespace {

struct IdState { uint32_t latest = 0 /* record index + 1 of the latest send; 0: none yet */, classes = 0 /* bit c: an event of class c carries the id */; };

// the ids' states: a flat table where the ids are as small as the engine's (dense from 0), a hash map otherwise
struct IdMap {
  std::vector<IdState> flat;
  std::unordered_map<uint32_t, IdState> sparse;
  IdMap(const msim_event *ev, uint32_t n) {
    uint32_t top = 0;
    for (uint32_t i = 0; i < n; i++) top = std::max(top, ev[i].msg >> 8);
    if (n && top <= 2u * n + 64u) flat.resize((size_t)top + 1);
  }
  IdState &at(uint32_t id) { return flat.empty() ? sparse[id] : flat[id]; }
};

void quantiles(std::vector<uint32_t> &lat, msim_latency_dist *d) {
  std::memset(d, 0, sizeof *d);
  const uint32_t n = (uint32_t)lat.size();
  if (!n) return;
  std::sort(lat.begin(), lat.end());
  const double pts[5] = {0.0, 0.5, 0.95, 0.99, 1.0};
  d->count = n;
  for (int q = 0; q < 5; q++) d->q_us[q] = lat[std::min(n - 1, (uint32_t)std::floor((double)n * pts[q]))];
  for (uint32_t l : lat) d->sum_us += l;
}

}  // namespace

extern "C" int msim_journal_messages_rows(const msim_event *events, uint32_t n_events, uint32_t n_nodes, uint32_t client_slots, msim_journal_summary *summary,
                                          msim_journal_msg *msgs, uint32_t max_msgs) {
  if ((!events && n_events) || !summary || (!msgs && max_msgs)) return MSIM_E_INVALID;
  msim_journal_summary s;
  std::memset(&s, 0, sizeof s);
  s.n_events = n_events; s.n_nodes = n_nodes; s.client_slots = client_slots;
  if (max_msgs) std::memset(msgs, 0, (size_t)max_msgs * sizeof *msgs);
  struct Rec { uint32_t recv, time, cls; };   // (every send's, whatever max_msgs is: the summary does not depend on it)
  std::vector<Rec> recs;
  std::vector<uint32_t> lat[2];
  IdMap ids(events, n_events);
  uint32_t n_ids = 0, ids_of[2] = {0, 0};
  bool in_range = true;
  for (uint32_t i = 0; i < n_events; i++) {
    const msim_event &e = events[i];
    const uint32_t id = e.msg >> 8, src = e.route & 0xFFu, dest = (e.route >> 8) & 0xFFu;
    const bool recv = (e.msg & 0x80u) != 0, client = src - n_nodes < client_slots || dest - n_nodes < client_slots;   // (unsigned: e < n_nodes wraps beyond every slot count)
    const uint32_t cls = client ? 0u : 1u;
    s.endpoints[src >> 5] |= 1u << (src & 31u); s.endpoints[dest >> 5] |= 1u << (dest & 31u);
    if (id >= n_events) in_range = false;
    IdState &st = ids.at(id);
    if (!st.classes) n_ids++;
    if (!(st.classes >> cls & 1u)) { st.classes |= 1u << cls; ids_of[cls]++; }
    if (!recv) {
      s.send_count[0]++; s.send_count[1 + cls]++;
      if (st.latest) s.dup_sends++;
      const uint32_t k = (uint32_t)recs.size();
      recs.push_back(Rec{MSIM_NO_VALUE, e.time_us, cls});
      st.latest = k + 1;
      if (k < max_msgs) msgs[k] = msim_journal_msg{id, i, MSIM_NO_VALUE, e.time_us, MSIM_NO_VALUE, (e.msg & 0x7Fu) | (client ? 0x80u : 0u), e.route, e.a};
    } else {
      s.recv_count[0]++; s.recv_count[1 + cls]++;
      if (!st.latest) { s.orphan_recvs++; continue; }
      Rec &r = recs[st.latest - 1];
      if (r.recv != MSIM_NO_VALUE) { s.extra_recvs++; continue; }
      const uint32_t l = e.time_us > r.time ? e.time_us - r.time : 0u;
      r.recv = i;
      lat[r.cls].push_back(l);
      if (st.latest - 1 < max_msgs) { msgs[st.latest - 1].recv_event = i; msgs[st.latest - 1].latency_us = l; }
    }
  }
  s.n_msgs = (uint32_t)recs.size();
  if (s.n_msgs > max_msgs) s.flags |= MSIM_JOURNAL_TABLE_TRUNCATED;
  s.msg_count[0] = n_ids; s.msg_count[1] = ids_of[0]; s.msg_count[2] = ids_of[1];
  for (const Rec &r : recs) if (r.recv == MSIM_NO_VALUE) { s.undelivered[0]++; s.undelivered[1 + r.cls]++; }
  for (int c = 0; c < 2; c++) quantiles(lat[c], &s.latency[c]);
  s.valid = (in_range && !s.dup_sends && !s.orphan_recvs && !s.extra_recvs) ? 1u : 0u;
  *summary = s;
  return MSIM_OK;
}
