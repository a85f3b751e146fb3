/* hat_nodes.inc — txn-rw-register served by the highly-available-transactions node (SURVEY.md §8f rank 4).
 * Included by maelsim_oracle.c.  TEST INFRASTRUCTURE.
 *
 *   node      demo/clojure/txn_rw_register_hat.clj (the --bin of the reference's own demo, core.clj:115-121):
 *               txn           :120-130  apply the transaction to the local state at a fresh timestamp [lamport, node]
 *                                       (apply-txn+ :34-74: reads return the register or nil, a write replaces the register
 *                                       unless the one in place has a LATER timestamp), advance the Lamport clock, remember
 *                                       the txn as unreplicated to every other node (:85-90), reply txn_ok;
 *               every 100 ms  :92-118   take one unreplicated txn, one node it still has to reach, and send that node ALL
 *                                       unreplicated txns that still have to reach it, each with its timestamp and the set
 *                                       of nodes it is still pending for (`replicate`, no msg_id);
 *               replicate     :132-150  apply every txn at its own timestamp (clock := max(clock, ts + 1)); a txn whose
 *                                       pending set minus this node is not empty REPLACES this node's own entry for that
 *                                       timestamp (the receiver relays it); then replicate_ack {node, tss} to every other node;
 *               replicate_ack :152-172  strike `node` from the pending set of each listed txn; drop entries that emptied.
 *   client    workload/txn_rw_register.clj:108-139 (Reusable, txn! RPC, no idempotent ops => a timeout is :info)
 *   generator [upstream] elle.rw-register/gen via jepsen.tests.cycle.wr (txn_rw_register.clj:162): the same key pool /
 *             length / unique-writes-per-key generator as list-append (txn_nodes.inc txn_generate), writes in place of appends.
 *
 * Canonical choices where the reference leaves the order to Clojure's hash maps / sets: "first" unreplicated txn = the
 * oldest one this node holds (creation order over the whole cluster), "first" node of a pending set = the lowest id.
 * The replication thread sleeps 100 ms in a loop from process start: ticks sit at multiples of 100 ms of virtual time; a
 * tick of a node without unreplicated txns does nothing and is not simulated (the timer is armed for the next multiple of
 * 100 ms when the set becomes non-empty, disarmed when it empties) — same observable behaviour, fewer rounds.
 *
 * Every txn of the cluster gets a slot g in one table (timestamp + where its micro-ops are); a node's unreplicated map is
 * pend[node][g] = bit mask of nodes (0 = no entry).  A replicate message refers to a list of words g | mask << 24 in the
 * replication area (cfg.replication_words); its acks refer to the same list.  A register is lamport << 11 | node << 8 |
 * value, 0 = never written.  Parity unpinned: no Clojure runtime here and the reference holds no test for this node. */

typedef struct hat_s {
  u32 *lamport, *lo, *npend; /* [N]: Lamport clock; no pending entry below lo; entries with pend != 0 */
  u32 *kv;                   /* [N][max_values] registers */
  u32 *tab;                  /* [G][2]: ts = lamport << 3 | node, request micro-ops ref = off | n << 24 */
  u8 *pend;                  /* [N][G] */
  u32 n_txn, G;
  u32 *area; u32 n_area;     /* replicate lists */
} hat_t;

static hat_t *hat_new(const sim_t *s) {
  hat_t *h = (hat_t *)calloc(1, sizeof(hat_t));
  h->G = s->cfg.max_rows / 2; /* every txn a node handles has an :invoke and a completion row */
  h->lamport = (u32 *)calloc(s->N, 4); h->lo = (u32 *)calloc(s->N, 4); h->npend = (u32 *)calloc(s->N, 4);
  h->kv = (u32 *)calloc((size_t)s->N * s->cfg.max_values, 4);
  h->tab = (u32 *)calloc((size_t)h->G * 2 + 2, 4);
  h->pend = (u8 *)calloc((size_t)s->N * h->G + 1, 1);
  h->area = (u32 *)calloc(s->cfg.replication_words + 1, 4);
  return h;
}
static void hat_free(hat_t *h) { free(h->lamport); free(h->lo); free(h->npend); free(h->kv); free(h->tab); free(h->pend); free(h->area); free(h); }

/* the unreplicated set of `node` went from empty to non-empty at time T: the replication thread's next wake-up */
static void hat_arm(sim_t *s, u32 node) {
  if (s->timer_next[node] == INF) s->timer_next[node] = (s->T / 100000u + 1u) * 100000u;
}

/* apply-txn+ writes (:55-63): last write wins by timestamp; ts = lamport << 3 | node */
static void hat_apply_writes(sim_t *s, u32 node, u32 ts, u32 ref) {
  u32 *kv = s->hat->kv + (size_t)node * s->cfg.max_values;
  u32 off = ref & 0xFFFFFFu, n = ref >> 24;
  for (u32 j = 0; j < n; j++) {
    u32 w = s->payload[off + j], key = (w >> 1) & 0x7FFFu;
    if (!(w & 1)) continue;
    if (kv[key] && (kv[key] >> 8) > ts) continue; /* (pos? (compare (:ts current-value) ts)): leave in place */
    kv[key] = (ts << 8) | ((w >> 16) & 0xFFu);
  }
}

static void hat_node_handle(sim_t *s, u32 node, const qent *q) {
  hat_t *h = s->hat;
  u8 *pend = h->pend + (size_t)node * h->G;
  switch (q->type) {
    case M_INIT: out_send(s, node, q->src, M_INIT_OK, 0, q->b); break;
    case M_TXN: { /* :120-130 */
      u32 off0 = q->a & 0xFFFFFFu, n = q->a >> 24;
      if (h->n_txn >= h->G || h->lamport[node] >= (1u << 21) - 1) {
        /* an engine capacity, mirrored while the engine runs: a kernel stops its cluster at the end of the round whose rows did not fit,
         * this run goes on dropping rows, and what it meets in later rounds no kernel ever sees */
        if (!s->rows_stop_round || s->rows_stop_round == s->rounds) s->meta.flags |= MSIM_FLAG_ARENA_OVERRUN;
        break;
      }
      u32 off = payload_alloc(s, n);
      if (off == INF) break;
      u32 g = h->n_txn++, ts = (h->lamport[node]++ << 3) | node;
      u32 *kv = h->kv + (size_t)node * s->cfg.max_values;
      for (u32 j = 0; j < n; j++) { /* micro-ops in order: a read sees the transaction's own earlier writes */
        u32 w = s->payload[off0 + j], key = (w >> 1) & 0x7FFFu;
        if (w & 1) { if (!(kv[key] && (kv[key] >> 8) > ts)) kv[key] = (ts << 8) | ((w >> 16) & 0xFFu); s->payload[off + j] = w; }
        else s->payload[off + j] = (key << 1) | ((kv[key] ? kv[key] & 0xFFu : 0xFFu) << 16);
      }
      h->tab[2 * g] = ts; h->tab[2 * g + 1] = q->a;
      pend[g] = (u8)(((1u << s->N) - 1) & ~(1u << node)); /* later-replicate!, :85-90 */
      if (h->npend[node]++ == 0) { h->lo[node] = g; hat_arm(s, node); }
      out_send(s, node, q->src, M_TXN_OK, off | (n << 24), q->b);
    } break;
    case M_REPLICATE: { /* :132-150 */
      u32 off = q->a, n = q->b;
      for (u32 i = 0; i < n; i++) {
        u32 w = h->area[off + i], g = w & 0xFFFFFFu, mask = w >> 24, ts = h->tab[2 * g];
        if (h->lamport[node] < (ts >> 3) + 1) h->lamport[node] = (ts >> 3) + 1;
        hat_apply_writes(s, node, ts, h->tab[2 * g + 1]);
        u32 rest = mask & ~(1u << node);
        if (rest) {
          if (!pend[g]) { if (h->npend[node]++ == 0) { h->lo[node] = g; hat_arm(s, node); } else if (g < h->lo[node]) h->lo[node] = g; }
          pend[g] = (u8)rest;
        }
      }
      for (u32 i = 0; i < s->N; i++) if (i != node) out_send(s, node, i, M_REPLICATE_ACK, off, n);
    } break;
    case M_REPLICATE_ACK: { /* :152-172 */
      u32 off = q->a, n = q->b;
      for (u32 i = 0; i < n; i++) {
        u32 g = h->area[off + i] & 0xFFFFFFu;
        if (!pend[g]) continue; /* txn already fully replicated */
        pend[g] &= (u8)~(1u << q->src);
        if (!pend[g]) h->npend[node]--;
      }
      if (h->npend[node] == 0) s->timer_next[node] = INF;
    } break;
    default: break;
  }
}

/* replicate-step!, :92-105 */
static void hat_tick(sim_t *s, u32 node) {
  hat_t *h = s->hat;
  u8 *pend = h->pend + (size_t)node * h->G;
  s->timer_next[node] = s->T + 100000u;
  u32 lo = h->lo[node];
  while (lo < h->n_txn && !pend[lo]) lo++;
  h->lo[node] = lo;
  if (lo >= h->n_txn) { s->timer_next[node] = INF; return; } /* cannot happen while npend > 0 */
  u32 dest = (u32)__builtin_ctz(pend[lo]), cnt = 0;
  for (u32 g = lo; g < h->n_txn; g++) if ((pend[g] >> dest) & 1) cnt++;
  if (h->n_area + cnt > s->cfg.replication_words) { s->meta.flags |= MSIM_FLAG_ARENA_OVERRUN; return; } /* engine capacity; nothing is sent */
  u32 off = h->n_area;
  for (u32 g = lo; g < h->n_txn; g++) if ((pend[g] >> dest) & 1) h->area[h->n_area++] = g | ((u32)pend[g] << 24);
  out_send(s, node, dest, M_REPLICATE, off, cnt);
}
