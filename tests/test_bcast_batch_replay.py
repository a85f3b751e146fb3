"""The batched-gossip model (tests/bcast_batch_ref.py) pinned against the reference's own demo/python/broadcast.py.

With MAELSTROM_REFERENCE set, real broadcast.py processes (unmodified, under tests/py_clock_launcher.py's virtual asyncio clock) get every
input the model's nodes got and must print, input by input, what the model emitted (tests/bcast_batch_replay.py: sets per input, list
order ignored, RPC ids renamed consistently per node) — on three shapes: exponential latency with p_loss 0.1, nine nodes under partitions
(1 s timeouts fire, whole batches are re-sent) and a line at 50 ms.  tests/golden/make_golden_bcast_batch.py records the digests of the
runs the real program reproduced; without the reference tree the model is held to those digests, and the device to the same model
(tests/test_bcast_batch_gpu.py, tests/test_bcast_batch_hipemu.py)."""
import json
import os

import pytest

import bcast_batch_ref as M

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bcast_batch_digests.json")))
_ids = lambda g: f"n{g['kw']['node_count']}-s{g['kw']['seed']}"


@pytest.mark.skipif(not os.environ.get("MAELSTROM_REFERENCE"), reason="needs the reference tree (MAELSTROM_REFERENCE) to run demo/python/broadcast.py")
@pytest.mark.parametrize("g", GOLDEN["pinned"], ids=_ids)
def test_real_broadcast_py_prints_what_the_model_emits(g):
    import bcast_batch_replay as R
    for i, d in zip(g["instances"], g["digests"]):
        b, nodes, st = R.replay(g["kw"], instance=i)
        assert st["inputs"] > 100 and st["sends"] > 100
        if g["kw"].get("nemesis") or g["kw"].get("p_loss"):
            assert st["timer_inputs"] > 0 and st["max_batch"] > 1   # RPCs timed out and batches of several values were re-sent
        assert M.model_digest(b, nodes) == d


@pytest.mark.parametrize("g", GOLDEN["pinned"], ids=_ids)
def test_model_reproduces_the_pinned_runs(g):
    """the runs in which the real program printed what the model emitted (recorded with the reference tree at hand)"""
    for i, d in zip(g["instances"], g["digests"]):
        b, nodes = M.run_model(instance=i, **g["kw"])
        assert not b.errors
        assert M.model_digest(b, nodes) == d


@pytest.mark.parametrize("g", GOLDEN["bench"], ids=lambda g: f"lat{g['kw'].get('latency', 0)}")
def test_model_reproduces_the_bench_shape_digests(g):
    """the cfg2-shape instances the device's 4096-cluster launch is held to"""
    for i, d in zip(g["instances"], g["digests"]):
        b, nodes = M.run_model(journal=False, instance=i, seed=g["seed"], **g["kw"])
        assert M.model_digest(b, nodes) == d
