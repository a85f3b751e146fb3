"""The batched-gossip model (tests/bcast_batch_ref.py: demo/python/broadcast.py as a state machine on the process bridge's scheduler)
against an answer derived from the program text: with no loss, no partitions and a constant latency below 500 ms every RPC is answered
before its 1 s timeout (maelstrom.py:89), so a link sends each value exactly once — the values carried by all broadcast_many bodies add up
to 2E x the broadcast values, and at latency 0 (one value per batch) the servers exchange 4E messages per broadcast.  The histories of
those shapes are valid set-full histories."""
import pytest

from maelstrom_amd import bridge as B
import bcast_batch_ref as M
import setfull_ref as R


def _edges(topology, n):
    return sum(len(x) for x in B.topology(topology, n)) // 2


@pytest.mark.parametrize("kw", [
    dict(node_count=25, rate=50, time_limit=6, latency=0, seed=1),
    dict(node_count=25, rate=50, time_limit=6, latency=100, seed=2),
    dict(node_count=9, rate=40, time_limit=6, latency=499, topology="line", seed=3),
    dict(node_count=10, concurrency=4, rate=40, time_limit=6, latency=20, topology="tree4", seed=4),
    dict(node_count=7, rate=40, time_limit=6, latency=5, topology="total", seed=5),
])
def test_every_value_crosses_every_directed_edge_once(kw):
    b, nodes = M.run_model(**kw)
    assert not b.errors
    E2 = _edges(kw.get("topology", "grid"), kw["node_count"])
    bcasts = sum(1 for op in b.history if op["type"] == ":invoke" and op["f"] == ":broadcast")
    assert bcasts > 0
    assert M.values_carried(b) == 2 * E2 * bcasts
    if kw["latency"] == 0:
        assert b.stats["servers_send"] == 4 * E2 * bcasts
    assert all(len(nd.log) == bcasts for nd in nodes)   # every node ends with every value, each logged once


def test_grid_5x5_at_latency_0_is_160_server_messages_per_broadcast():
    b, _ = M.run_model(node_count=25, rate=20, time_limit=4, seed=6)
    bcasts = sum(1 for op in b.history if op["type"] == ":invoke" and op["f"] == ":broadcast")
    assert b.stats["servers_send"] == 160 * bcasts


@pytest.mark.parametrize("kw", [
    dict(node_count=25, rate=50, time_limit=6, latency=100, seed=7),
    dict(node_count=9, rate=40, time_limit=6, latency=50, topology="line", seed=8),
])
def test_fault_free_histories_are_valid(kw):
    b, _ = M.run_model(journal=False, **kw)
    res = R.set_full(b.history)
    assert res["valid?"] is True and res["lost-count"] == 0


def test_timeouts_resend_the_whole_unacknowledged_batch():
    """under partitions RPCs time out and their batches are re-sent whole: a batch holds more than the values of one broadcast"""
    b, nodes = M.run_model(node_count=9, rate=30, time_limit=8, latency=20, nemesis=["partition"], nemesis_interval=2, seed=9)
    sends = [ev["message"] for ev in b.journal if ev["type"] == ":send" and ev["message"]["body"]["type"] == "broadcast_many"]
    assert max(len(m["body"]["messages"]) for m in sends) > 10
    by = {}
    for m in sends:
        by.setdefault((m["src"], m["dest"]), []).append(m["body"]["messages"])
    # some link re-sent a batch: the same first value twice in a row (the acknowledged prefix did not move)
    assert any(x[0] == y[0] for v in by.values() for x, y in zip(v, v[1:]))
    final = [op for op in b.history if op.get("final?") and op["type"] == ":ok"]
    bcasts = sorted(op["value"] for op in b.history if op["type"] == ":invoke" and op["f"] == ":broadcast")
    assert final and all(op["value"] == bcasts for op in final)
