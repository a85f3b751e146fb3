"""The generic process bridge (maelstrom_amd/bridge.py; process.clj:136-215 on the deterministic scheduler): real node PROCESSES
over pipes, in virtual time.  A run is reproducible from its seed, and — because the bridge restates the same rounds and draws the
same random numbers as the engine's specification — a node program that behaves like a built-in node yields exactly the history
the oracle (and therefore the GPU engine) emits: broadcast with this repository's fire-and-forget node process, echo with the
REFERENCE's own demo/python/echo.py.  The runs of the reference's own programs (replay_*: they need the reference tree and node.js) are
recorded by tests/golden/make_reference_runs.py (tests/reference_runs.py); the tests hold the oracle to them."""
import os
import sys

import pytest

from maelstrom_amd import bridge as B
from maelstrom_amd import engine as E
import oracle_lib as O
import reference_runs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FF_NODE = [sys.executable, os.path.join(ROOT, "tools", "harness_node.py")]
TSO_NODE = [sys.executable, os.path.join(ROOT, "tools", "harness_tso_node.py")]


def _norm(ops):
    out = []
    for op in ops:
        o = {k: op[k] for k in ("index", "time", "type", "f", "process", "value") if k in op}
        if "error" in op:
            o["error"] = op["error"] if isinstance(op["error"], str) else op["error"][0]
        if op.get("final?"):
            o["final?"] = True
        out.append(o)
    return out


def _against_oracle(workload, argv, oracle_bin=None, **kw):
    cfg = E.test_config(workload, bin=oracle_bin, **kw)
    ora = O.run(cfg, 0, 1)
    want = E.decode_history(*ora.history(0), cfg.n_nodes, cfg.workload, cfg.node_program)
    for attempt in (0, 1):
        b = B.Bridge(workload, argv, **kw)
        got = b.run()
        # The bridge decides that real processes are DONE with a round from /proc (NodeProcess.idle): on a machine busy with something else a
        # node has once been seen idle a moment before it printed (1 run in 13 of a ten-worker case right after a parallel build, round 6).  A
        # run that differs is repeated ONCE; a program that differs from the oracle differs both times.
        if attempt == 0 and (b.errors or _norm(got) != _norm(want)):
            continue
        break
    assert b.errors == []
    assert _norm(got) == _norm(want)
    assert b.rounds == int(ora.meta["n_rounds"][0])
    st = ora.stats[0]
    assert tuple(b.stats[k] for k in ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv")) == tuple(int(x) for x in st)
    return b


def _oracle_run(workload, oracle_bin=None, **kw):
    """digest of what _against_oracle compares: the oracle's history, round count and net stats"""
    cfg = E.test_config(workload, bin=oracle_bin, **kw)
    ora = O.run(cfg, 0, 1)
    want = E.decode_history(*ora.history(0), cfg.n_nodes, cfg.workload, cfg.node_program)
    return R.digest(_norm(want), int(ora.meta["n_rounds"][0]), [int(x) for x in ora.stats[0]])


@pytest.mark.parametrize("kw", [
    dict(node_count=5, rate=10, time_limit=5, seed=7),
    dict(node_count=5, rate=20, time_limit=5, latency=20, latency_dist="exponential", p_loss=0.05, nemesis=["partition"], nemesis_interval=2, seed=8),
    dict(node_count=9, rate=30, time_limit=4, latency=10, topology="tree3", seed=9),
    dict(node_count=4, concurrency=8, rate=20, time_limit=4, latency=5, latency_dist="uniform", topology="line", seed=10),
])
def test_broadcast_node_processes_reproduce_the_oracle_history(kw):
    b = _against_oracle("broadcast", FF_NODE, **kw)
    m = b.net_stats()
    assert m["all"]["send-count"] == b.stats["all_send"] and m["servers"]["msgs-per-op"] > 0


ECHO_CASES = [dict(node_count=3, rate=10, time_limit=5, seed=1),
              dict(node_count=3, rate=20, time_limit=6, p_loss=0.1, seed=2)]   # timeouts -> :info, new processes


def test_reference_echo_py_reproduces_the_oracle_history():
    """BASELINE configs[0]: echo, 3 nodes — the runs in which the reference's own demo binary reproduced the oracle's history (replay_echo_py)"""
    for kw in ECHO_CASES:
        assert _oracle_run("echo", **kw) == R.recorded("bridge-echo-py", kw)


def replay_echo_py(kw):
    _against_oracle("echo", [sys.executable, R.reference_path("demo", "python", "echo.py")], **kw)


def test_runs_are_reproducible_and_journalled():
    kw = dict(node_count=5, rate=20, time_limit=4, latency=10, latency_dist="exponential", seed=11)
    a = B.Bridge("broadcast", FF_NODE, journal=True, **kw)
    ha = a.run()
    b = B.Bridge("broadcast", FF_NODE, journal=True, **kw)
    hb = b.run()
    assert ha == hb and a.journal == b.journal and len(a.journal) == a.stats["all_send"] + a.stats["all_recv"]
    assert [e["id"] for e in a.journal] == list(range(len(a.journal)))
    gossip = [e for e in a.journal if e["type"] == ":send" and e["message"]["src"].startswith("n") and e["message"]["dest"].startswith("n")]
    assert gossip and all(e["message"]["body"] == {"type": "broadcast", "message": e["message"]["body"]["message"]} for e in gossip)


def test_lin_tso_service_serves_a_unique_ids_node():
    """service.clj:116-132: a monotonically increasing stream of integers from 0; ids handed out through it are unique, and every
    client sees its own ids grow (lin-tso is linearizable)."""
    b = B.Bridge("unique-ids", TSO_NODE, node_count=3, rate=100, time_limit=3, latency=5, seed=3)
    hist = b.run()
    assert b.errors == []
    ids = [op["value"] for op in hist if op["type"] == ":ok"]
    assert len(ids) > 200 and sorted(ids) == list(range(len(ids)))     # 0, 1, 2, ... each exactly once
    per = {}
    for op in hist:
        if op["type"] == ":ok":
            assert per.get(op["process"], -1) < op["value"]
            per[op["process"]] = op["value"]
    assert b.stats["servers_send"] == 2 * len(ids)                     # one ts / ts_ok pair per id


@pytest.mark.parametrize("kw", [dict(node_count=3, rate=100, time_limit=3, latency=5, seed=3),
                                dict(node_count=5, concurrency=10, rate=200, time_limit=2, latency=10, latency_dist="exponential", seed=4),
                                dict(node_count=3, rate=100, time_limit=6, latency=3, nemesis=["partition"], nemesis_interval=2, seed=6)])
def test_oracle_tso_node_and_service_equal_the_process_node_over_the_bridges_lin_tso(kw):
    """oracle/svc_nodes.inc's lin-tso service and its unique-ids node against the real node process (tools/harness_tso_node.py)
    talking to the bridge's lin-tso (a transliteration of service.clj:116-132): same history, rounds and net statistics."""
    _against_oracle("unique-ids", TSO_NODE, oracle_bin="tso-ids", **kw)


def test_services_behind_the_bridge():
    """service.clj:31-61,161-210 through the bridge's own service objects (what a --bin talking to seq-kv / lin-kv / lww-kv gets)"""
    lin = B.default_services()["lin-kv"]
    assert lin.handle("n0", {"type": "read", "key": "x"}, None)["code"] == 20
    assert lin.handle("n0", {"type": "cas", "key": "x", "from": 1, "to": 2, "create_if_not_exists": True}, None)["type"] == "cas_ok"
    assert lin.handle("n1", {"type": "cas", "key": "x", "from": 1, "to": 3}, None)["code"] == 22
    assert lin.handle("n1", {"type": "read", "key": "x"}, None) == {"type": "read_ok", "value": 2}
    seq = B.default_services()["seq-kv"]
    for i in range(16):
        assert seq.handle("c0", {"type": "write", "key": "x", "value": i}, lambda n: 0)["type"] == "write_ok"
    vals = {seq.handle(f"fresh-{i}", {"type": "read", "key": "x"}, lambda n, i=i: i % n).get("value") for i in range(64)}
    assert len(vals) > 1                                              # service_test.clj:20-28
    seq.handle("me", {"type": "write", "key": "y", "value": 1}, lambda n: 0)
    assert seq.handle("me", {"type": "read", "key": "x"}, lambda n: 0)["value"] == 15   # service_test.clj:30-38


def test_cli(tmp_path):
    rc = B.main(["test", "-w", "broadcast", "--bin", FF_NODE[0], "--node-count", "3", "--rate", "10", "--time-limit", "2", "--history",
                 str(tmp_path / "history.edn"), "--", FF_NODE[1]])
    assert rc == 0
    lines = open(tmp_path / "history.edn").read().splitlines()
    assert lines and lines[0].startswith("{:index 0, :time ") and ":f :broadcast" in "".join(lines)


SINGLE_KEY_CASES = [
    dict(node_count=3, rate=20, time_limit=4, seed=5),
    dict(node_count=5, rate=50, time_limit=8, latency=5, nemesis=["partition"], nemesis_interval=2, seed=8),
    dict(node_count=3, rate=100, time_limit=5, latency=20, latency_dist="exponential", p_loss=0.05, seed=9),
    dict(node_count=2, rate=200, time_limit=3, latency=2, key_count=3, max_txn_length=4, max_writes_per_key=8, seed=10),
    dict(node_count=2, concurrency=8, rate=200, time_limit=3, latency=2, key_count=3, seed=11),   # several workers per node (--concurrency 4n)
    dict(node_count=1, concurrency=10, rate=100, time_limit=3, latency=1, seed=12),
]


@pytest.mark.parametrize("kw", SINGLE_KEY_CASES)
def test_reference_single_key_txn_js_reproduces_the_oracle_history(kw):
    """the run in which single_key_txn.js reproduced the oracle's history on the bridge (replay_single_key_txn_js)"""
    assert _oracle_run("txn-list-append", **kw) == R.recorded("bridge-single-key-txn-js", kw)


def replay_single_key_txn_js(kw):
    """BASELINE configs[4]'s node program: the REFERENCE's own demo/js/single_key_txn.js as real node.js processes, with the bridge's
    lin-kv service, yields the history, round count and net stats of the oracle's txn-list-append (restated from
    demo/clojure/single_key_txn.clj) — over whole runs, under partitions and loss.  (One corner is the two demos' own: when the
    root does not exist yet, the JS node compares `[]` and the Clojure node `nil` against a root another read-only transaction has
    just created as `[]` — the JS cas succeeds, the Clojure one, and the oracle, report a conflict.  The seeds here do not start
    with such a race.)"""
    _against_oracle("txn-list-append", ["node", R.reference_path("demo", "js", "single_key_txn.js")], **kw)


MULTI_KEY_CASES = [
    dict(node_count=2, rate=20, time_limit=2, latency=2, key_count=3, seed=5),
    dict(node_count=3, rate=50, time_limit=3, latency=5, seed=6),
    dict(node_count=5, rate=60, time_limit=3, latency=10, latency_dist="exponential", nemesis=["partition"], nemesis_interval=1, seed=7),
    dict(node_count=3, rate=150, time_limit=2, latency=3, latency_dist="uniform", key_count=2, max_txn_length=8, max_writes_per_key=32, seed=8),
    dict(node_count=7, rate=100, time_limit=2, latency=0, seed=9),
    dict(node_count=2, concurrency=8, rate=200, time_limit=3, latency=2, key_count=3, seed=11),   # several workers per node (--concurrency 4n): transactions of one node race for the root
    dict(node_count=1, concurrency=10, rate=100, time_limit=3, latency=1, seed=12),               # --concurrency 10n (doc/05-datomic/01-single-node.md:257)
]


@pytest.mark.parametrize("kw", MULTI_KEY_CASES)
def test_reference_multi_key_txn_js_reproduces_the_oracle_history(kw):
    """the run in which multi_key_txn.js reproduced the oracle's history on the bridge (replay_multi_key_txn_js)"""
    assert _oracle_run("txn-list-append", oracle_bin="multi-key-txn", **kw) == R.recorded("bridge-multi-key-txn-js", kw)


def replay_multi_key_txn_js(kw):
    """The canonical txn-list-append node (row a18): the REFERENCE's own demo/js/multi_key_txn.js as real node.js processes — thunks in
    the bridge's lww-kv, the root map in its lin-kv, retries after a lost root cas, thunk reads repeated while the other lww-kv replica
    answers — yields the history, the round count and the net stats of the oracle's restatement (oracle/mk_nodes.inc) over whole runs:
    contended keys, long transactions, partitions between the nodes, random latency.  Loss-free on purpose: node.js's rpc() gives up
    after one second of wall-clock time, which no virtual-time run can share."""
    _against_oracle("txn-list-append", ["node", R.reference_path("demo", "js", "multi_key_txn.js")], oracle_bin="multi-key-txn", **kw)


DATOMIC_NODE = [sys.executable, os.path.join(ROOT, "tools", "datomic_node.py")]


@pytest.mark.parametrize("kw", [
    dict(node_count=1, rate=40, time_limit=4, latency=2, seed=5),
    dict(node_count=3, rate=60, time_limit=4, latency=5, seed=6),
    dict(node_count=5, rate=80, time_limit=3, latency=10, latency_dist="exponential", nemesis=["partition"], nemesis_interval=1, seed=7),
    dict(node_count=3, rate=150, time_limit=3, latency=0, key_count=16, max_writes_per_key=2, seed=8),   # many keys: splits and chains
    dict(node_count=1, concurrency=10, rate=100, time_limit=4, latency=1, seed=9),                        # --concurrency 10n (doc/05-datomic/01-single-node.md:257): the lock's queue
    dict(node_count=2, concurrency=6, rate=120, time_limit=3, latency=3, latency_dist="uniform", seed=10),
])
def test_datomic_node_process_reproduces_the_oracle_history(kw):
    """The Datomic-style node (row a18) as REAL PROCESSES — the Ruby classes written out in Python (tests/datomic_ref.py) behind the wire protocol
    (tools/datomic_node.py): materialised trees, maps and lists, the node's lock as a FIFO, tree nodes as JSON values in the bridge's own lww-kv (two
    replicas that never exchange state), the root pointer in its lin-kv — under the bridge's scheduler yield the history, the round count and the
    net stats of the oracle's restatement (oracle/dt_nodes.inc: counts, versions and a lineage rule instead of values), whole runs, several
    workers per node included.  Not the replay of tests/test_datomic_tree.py (which feeds the classes the oracle's own journal): here nothing of
    the oracle steers the run.  The classes are the same author's reading of the Ruby — parity with the reference itself stays unpinned."""
    _against_oracle("txn-list-append", DATOMIC_NODE, oracle_bin="datomic", **kw)


STRICT_CASE = dict(node_count=5, rate=40, time_limit=3, latency=5, nemesis=["partition"], nemesis_interval=1, seed=8)


def test_reference_multi_key_txn_js_runs_strict_serializably_on_the_bridge():
    """demo/js/multi_key_txn.js (thunks in lww-kv, the root map in lin-kv, retry on a lost root cas) is not a built-in node of the
    GPU engine; on the bridge it runs as it is, against the bridge's lin-kv and eventually consistent lww-kv services, and the
    list-append analysis finds its histories clean — also under partitions.  The history is the one replay_multi_key_txn_js_strict
    recorded (two runs from the seed, identical)."""
    rec = R.recorded("bridge-multi-key-txn-js-strict", STRICT_CASE)
    ops = [o for o in rec["history"] if o["process"] != ":nemesis"]
    assert sum(o["type"] == ":ok" for o in ops) > 50
    res = E.check_txn_history(*E.encode_txn_history(ops))
    assert res["valid?"] is True and res["anomalies"] == [], res
    assert rec["servers_send"] > 6 * res["ok-count"]   # per transaction: root read / cas + thunk reads and writes


def replay_multi_key_txn_js_strict():
    """two bridge runs of multi_key_txn.js from STRICT_CASE's seed: the same history; returns what the test above checks"""
    hist = []
    for _ in range(2):
        b = B.Bridge("txn-list-append", ["node", R.reference_path("demo", "js", "multi_key_txn.js")], **STRICT_CASE)
        h = b.run()
        assert b.errors == []
        hist.append(h)
    assert hist[0] == hist[1]
    return {"history": hist[0], "servers_send": b.stats["servers_send"]}
