"""Reference model of the reference's batched-gossip broadcast node (demo/python/broadcast.py over demo/python/maelstrom.py), written
as a state machine for the process bridge's in-process node hook (maelstrom_amd/bridge.py node_factory), as DESIGN.md §2.4 states it:

  * the node's values in an append-only ARRIVAL LOG (a value is appended when it is first seen, a batch's new values in batch order);
  * per topology neighbour (a link) the acknowledged prefix of that log, and while an RPC is in flight the end of its batch, its RPC id
    and its deadline (1 s after the send, maelstrom.py:89).  What broadcast.py calls `sent` is always the acknowledged prefix;
  * a grown log wakes every idle link; a link's batch is log[acked:len(log)]; replies go out before the new batches, new RPCs in
    ascending neighbour order with ids from the node's one counter (maelstrom.py:67); all deadlines of the node that are due expire
    together as its one timer input, and every expired link re-sends at once.

Test infrastructure: run_model() gives the bridge run the GPU engine's general kernel (MSIM_NODE_BCAST_BATCH) is held to."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from maelstrom_amd import bridge as B  # noqa: E402

INF = B.INF
RPC_TIMEOUT_US = 1_000_000   # maelstrom.py:89


class Link:
    __slots__ = ("acked", "end", "rpc", "deadline")

    def __init__(self):
        self.acked, self.end, self.rpc, self.deadline = 0, None, 0, INF   # end is None: idle (the gossip task waits)


class BatchNode:
    def __init__(self, name):
        self.id = name
        self.log, self.seen = [], set()
        self.links = {}          # neighbour -> Link, in topology order (ascending node index)
        self.next_msg_id = 0     # the last RPC id handed out (maelstrom.py:67 starts at 1)

    # ---- timers ----
    def next_timer(self):
        return min((lk.deadline for lk in self.links.values() if lk.end is not None), default=INF)

    def on_timer(self, T):
        return self._send([p for p, lk in self.links.items() if lk.end is not None and lk.deadline <= T], T)

    # ---- messages ----
    def _send(self, peers, T):
        out = []
        for p in peers:
            lk = self.links[p]
            self.next_msg_id += 1
            lk.end, lk.rpc, lk.deadline = len(self.log), self.next_msg_id, T + RPC_TIMEOUT_US
            out.append({"src": self.id, "dest": p, "body": {"type": "broadcast_many", "messages": self.log[lk.acked:lk.end], "msg_id": lk.rpc}})
        return out

    def _add(self, values):
        grew = False
        for v in values:
            if v not in self.seen:
                self.seen.add(v)
                self.log.append(v)
                grew = True
        return grew

    def handle(self, msg, T):
        src, body = msg["src"], msg["body"]
        t = body.get("type")
        out = []

        def reply(b):
            out.append({"src": self.id, "dest": src, "body": {**b, "in_reply_to": body.get("msg_id")}})
        if "in_reply_to" in body:   # a reply to one of our RPCs
            lk = self.links.get(src)
            if lk is None or lk.end is None or lk.rpc != body["in_reply_to"]:
                return out          # late: its RPC already timed out (maelstrom.py:100,153)
            if t == "broadcast_many_ok":
                lk.acked = lk.end
            lk.end, lk.deadline = None, INF
            if lk.acked < len(self.log):
                out += self._send([src], T)
            return out
        grew = False
        if t == "init":
            self.id = body["node_id"]
            reply({"type": "init_ok"})
        elif t == "topology":
            self.links = {p: Link() for p in body["topology"][self.id]}
            reply({"type": "topology_ok"})
        elif t == "broadcast":
            grew = self._add([body["message"]])
            reply({"type": "broadcast_ok"})
        elif t == "broadcast_many":
            grew = self._add(body["messages"])
            reply({"type": "broadcast_many_ok"})
        elif t == "read":
            reply({"type": "read_ok", "messages": sorted(self.seen)})
        else:
            reply({"type": "error", "code": 10, "text": "RPC type is not supported"})
        if grew:
            out += self._send([p for p, lk in self.links.items() if lk.end is None], T)
        return out


class RecordingNode(BatchNode):
    """BatchNode that keeps its inputs and what it emitted for each: trace = [(T, message or None for the timer, [messages])]"""

    def __init__(self, name):
        super().__init__(name)
        self.trace = []

    def on_timer(self, T):
        out = super().on_timer(T)
        self.trace.append((T, None, out))
        return out

    def handle(self, msg, T):
        out = super().handle(msg, T)
        self.trace.append((T, msg, out))
        return out


def run_model(journal=True, node=BatchNode, **kw):
    """One instance of the model on the bridge's scheduler; kw are Bridge options (node_count, rate, latency, ...)"""
    b = B.Bridge("broadcast", None, journal=journal, node_factory=node, **kw)
    nodes = b.nodes
    b.run()
    return b, nodes


def engine_events(b, nodes):
    """The bridge journal in the engine's event words (include/maelsim.h msim_event) as tuples (time_us, msg, a, route); `a` is None
    where the engine's word is a payload reference or a value the body does not carry (compare those by other means)."""
    code = {n: i for i, n in enumerate(__import__("maelstrom_amd._abi", fromlist=["MSG_TYPES"]).MSG_TYPES) if n}
    ep = b.ep
    by_name = {nd.id: nd for nd in nodes}
    out = []
    for ev in b.journal:
        m = ev["message"]
        body = m["body"]
        t = body["type"]
        a = None
        if t == "broadcast":
            a = body["message"]
        elif t == "broadcast_many":
            log = by_name[m["src"]].log
            frm = log.index(body["messages"][0])
            a = frm | ((frm + len(body["messages"])) << 16)
        elif t in ("init", "topology", "read", "broadcast_many_ok", "init_ok", "topology_ok"):
            a = 0
        b16 = body.get("msg_id", body.get("in_reply_to")) or 0
        route = ep[m["src"]] | (ep[m["dest"]] << 8) | ((b16 & 0xFFFF) << 16)
        out.append((ev["time"] // 1000, (m["id"] << 8) | (0x80 if ev["type"] == ":recv" else 0) | code[t], a, route))
    return out


def values_carried(b):
    """values in all broadcast_many bodies sent (journal :send events)"""
    return sum(len(ev["message"]["body"]["messages"]) for ev in b.journal if ev["type"] == ":send" and ev["message"]["body"]["type"] == "broadcast_many")


STAT_KEYS = ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv")


def digest(history, stats, rounds, events=None):
    """sha256 of what an instance is compared on: its normalised history, net stats, round count and (journal on) its events"""
    import hashlib
    h = hashlib.sha256()
    h.update(json.dumps(norm_history(history), sort_keys=True).encode())
    h.update(json.dumps([int(x) for x in stats] + [int(rounds)]).encode())
    if events is not None:
        h.update(json.dumps([list(e) for e in events]).encode())
    return h.hexdigest()


def model_digest(b, nodes):
    return digest(b.history, [b.stats[k] for k in STAT_KEYS], b.rounds, engine_events(b, nodes) if b.journal is not None else None)


def engine_digest(eng, i):
    """digest() of engine instance i (fetched; journal off) in the same form as model_digest"""
    from maelstrom_amd import engine as E
    cfg = eng.cfg
    rows, pay = eng.raw_history(i)
    st = eng.net_stats_raw(i)
    return digest(E.decode_history(rows, pay, cfg.n_nodes, cfg.workload, cfg.node_program), [getattr(st, k) for k in STAT_KEYS], eng.meta(i).n_rounds)


def norm_history(ops):
    """the fields both histories carry (tests/test_process_bridge.py compares the same way)"""
    out = []
    for op in ops:
        o = {k: op[k] for k in ("index", "time", "type", "f", "process", "value") if k in op}
        if "error" in op:
            o["error"] = op["error"] if isinstance(op["error"], str) else op["error"][0]
        if op.get("final?"):
            o["final?"] = True
        out.append(o)
    return out


def compare_engine_instance(eng, i, kw):
    """Engine instance i (fetched) against the model run of (kw, instance i): history, rounds, net stats, flags and — with the journal
    on — every event (read_ok bodies through the payload they point at).  Returns a list of differences (empty: equal)."""
    from maelstrom_amd import engine as E
    import numpy as np
    cfg = eng.cfg
    b, nodes = run_model(journal=bool(cfg.journal_capacity), instance=i, **kw)
    bad = []
    if b.errors:
        bad.append(f"model errors {b.errors[:3]}")
    rows, pay = eng.raw_history(i)
    got = norm_history(E.decode_history(rows, pay, cfg.n_nodes, cfg.workload, cfg.node_program))
    want = norm_history(b.history)
    if got != want:
        k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
        bad.append(f"history differs at row {k} of {len(got)}/{len(want)}: {got[k] if k < len(got) else None} != {want[k] if k < len(want) else None}")
    m = eng.meta(i)
    if m.flags != 0:
        bad.append(f"flags {m.flags:#x}")
    if m.n_rounds != b.rounds:
        bad.append(f"rounds {m.n_rounds} != {b.rounds}")
    st = eng.net_stats_raw(i)
    keys = ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv")
    if tuple(getattr(st, k) for k in keys) != tuple(b.stats[k] for k in keys):
        bad.append(f"stats {tuple(getattr(st, k) for k in keys)} != {tuple(b.stats[k] for k in keys)}")
    if cfg.journal_capacity:
        ev = eng.raw_journal(i)
        want_ev = engine_events(b, nodes)
        if len(ev) != len(want_ev):
            bad.append(f"journal length {len(ev)} != {len(want_ev)}")
        for j in range(min(len(ev), len(want_ev))):
            t, msg, a, route = want_ev[j]
            g = (int(ev["time_us"][j]), int(ev["msg"][j]), int(ev["a"][j]), int(ev["route"][j]))
            ok = g[0] == t and g[1] == msg and g[3] == route and (a is None or g[2] == a)
            if ok and a is None and (msg & 0x7F) == 10:   # read_ok: the payload words the event points at
                words = pay[g[2] & 0xFFFFFF:(g[2] & 0xFFFFFF) + (g[2] >> 24)]
                body = b.journal[j]["message"]["body"]
                ok = E.bitmap_to_list(np.asarray(words)) == sorted(body["messages"])
            if not ok:
                bad.append(f"journal event {j}: {g} != {want_ev[j]}")
                break
    return bad


if __name__ == "__main__":
    # python tests/bcast_batch_ref.py '<json: test_config keywords + "n" instances + optional "flags">' — runs the engine (MSIM_LIB picks
    # the library: the device one or the host emulator's) and compares every instance with the model; prints "<case>: OK" or the differences
    from maelstrom_amd import engine as E
    for arg in sys.argv[1:]:
        kw = json.loads(arg)
        n, flags, cap = kw.pop("n", 1), kw.pop("flags", None), kw.pop("journal_capacity", 0)
        cfg = E.test_config("broadcast", bin="broadcast-batch", **kw, **({"journal_capacity": cap} if cap else {}))
        with E.Engine(cfg, device=0) as eng:
            if flags is not None:
                eng.set_dev_flags(flags)
            eng.run(0, n)
            eng.fetch()
            bad = [f"instance {i}: {d}" for i in range(n) for d in compare_engine_instance(eng, i, kw)]
        print(f"{arg}: OK" if not bad else f"{arg}: FAIL\n  " + "\n  ".join(bad[:10]), flush=True)
