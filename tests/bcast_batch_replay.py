"""Replay of the batched-gossip model against the reference's own program: every node of a model run (tests/bcast_batch_ref.py on the
process bridge's scheduler) is re-run as a real, unmodified demo/python/broadcast.py process (from MAELSTROM_REFERENCE) under
tests/py_clock_launcher.py, which gives it a virtual asyncio clock.  The process gets exactly the inputs the model's node got — the
messages it received, in order, and its timer inputs as moves of the clock to the due deadline — and what it prints for each input must
be what the model emitted for it:
  * compared as a set per input (the program prints from executor threads: the order of a batch of sends is not the model's);
  * list order inside a body is ignored (the program's `messages` is a set);
  * the program's RPC ids are renamed to the model's consistently per node (its tasks take ids from one counter in the order asyncio
    wakes them; the model hands them out in ascending neighbour order): the first time a model id is matched it is bound to the
    program's id, both one-to-one for the rest of the run, and replies fed to the process carry its own ids.
"Done with an input" is decided from /proc (maelstrom_amd/bridge.py NodeProcess.idle: stdin consumed, every thread asleep, no CPU time
between two looks), never from a wall-clock sleep.  Test infrastructure only."""
import collections
import os
import select
import sys
import time

import bcast_batch_ref as M
from maelstrom_amd import bridge as B

HERE = os.path.dirname(os.path.abspath(__file__))
LAUNCHER = os.path.join(HERE, "py_clock_launcher.py")


def program_path():
    root = os.environ.get("MAELSTROM_REFERENCE")
    if not root:
        raise RuntimeError("set MAELSTROM_REFERENCE to the reference tree to replay demo/python/broadcast.py")
    return os.path.join(root, "demo", "python", "broadcast.py")


def _collect(proc, limit_s=10.0):
    """lines the process prints until it is done with what it was given (/proc idleness, twice the same look)"""
    got, last = [], None
    hard = time.monotonic() + limit_s
    while True:
        r, _, _ = select.select([proc.fd], [], [], 0.0003)
        if r:
            lines = proc.lines()
            if not lines and proc.p.poll() is not None:
                raise AssertionError(f"{proc.node_id}: the process exited")
            got += lines
            last = None
            continue
        cur = proc.idle()
        if cur is None:
            raise RuntimeError("the replay needs /proc to tell when a process is done")
        if cur[0] and cur == last:
            return got
        last = cur
        if time.monotonic() > hard:
            raise AssertionError(f"{proc.node_id}: not idle after {limit_s} s")


def _key(m, rename):
    """a message as compared: dest, type, contents as a set, request ids through `rename`"""
    body = m["body"]
    t = body["type"]
    content = frozenset(body["messages"]) if "messages" in body else body.get("message")
    return (m["dest"], t, content, body.get("in_reply_to"), rename(body["msg_id"]) if "msg_id" in body else None)


def replay_node(nd, program):
    """Drives one real process through node `nd`'s recorded trace; returns (inputs, timer inputs, sends compared) or raises"""
    import json
    proc = B.NodeProcess([sys.executable, LAUNCHER, program], nd.id)
    m2r, r2m = {}, {}   # model RPC id <-> the program's
    now, n_timer, n_out = 0, 0, 0
    try:
        for k, (T, msg, outs) in enumerate(nd.trace):
            if T != now:
                proc.write({"__clock__": T})   # swallowed by the launcher: moves the process's clock; due timeouts fire
                now = T
            if msg is None:
                n_timer += 1
            else:
                body = msg["body"]
                if "in_reply_to" in body and msg["src"] in nd.links:   # a reply to one of the node's RPCs: the program's own id
                    body = {**body, "in_reply_to": m2r.get(body["in_reply_to"], -1)}
                proc.write({**msg, "body": body})
            printed = [json.loads(line) for line in _collect(proc)]
            # bind the program's broadcast_many ids to the model's: same destination, same set of values
            want_ids = {(o["dest"], frozenset(o["body"]["messages"])): o["body"]["msg_id"] for o in outs if o["body"]["type"] == "broadcast_many"}
            for p in printed:
                if p.get("body", {}).get("type") == "broadcast_many":
                    mid = want_ids.get((p["dest"], frozenset(p["body"]["messages"])))
                    rid = p["body"]["msg_id"]
                    if mid is not None and mid not in m2r and rid not in r2m:
                        m2r[mid], r2m[rid] = rid, mid
            got = collections.Counter(_key(p, lambda r: r2m.get(r, ("unbound", r))) for p in printed)
            want = collections.Counter(_key(o, lambda x: x) for o in outs)
            if got != want:
                raise AssertionError(f"{nd.id}: input {k} at T={T} us ({'timer' if msg is None else msg['body']['type']}): "
                                     f"the program printed {sorted(map(str, got - want))[:4]}, the model emitted {sorted(map(str, want - got))[:4]}")
            n_out += len(outs)
    finally:
        proc.stop()
    return len(nd.trace), n_timer, n_out


def replay(kw, instance=0, program=None):
    """Model run of (kw, instance), then every node replayed against the real program.  Returns the model run and summary counts."""
    program = program or program_path()
    b, nodes = M.run_model(node=M.RecordingNode, instance=instance, **kw)
    assert not b.errors, b.errors
    stats = collections.Counter()
    for nd in nodes:
        n_in, n_timer, n_out = replay_node(nd, program)
        stats.update(inputs=n_in, timer_inputs=n_timer, sends=n_out)
    stats["max_batch"] = max((len(ev["message"]["body"]["messages"]) for ev in b.journal
                              if ev["type"] == ":send" and ev["message"]["body"]["type"] == "broadcast_many"), default=0)
    return b, nodes, dict(stats)
