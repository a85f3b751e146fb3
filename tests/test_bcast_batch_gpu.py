"""The batched-gossip broadcast node (demo/python/broadcast.py; MSIM_NODE_BCAST_BATCH, the general kernel's batch arm, k_general_d.hip)
on the device against its model on the process bridge's scheduler (tests/bcast_batch_ref.py): decoded history, net stats, round count
and journal, over every latency distribution, the topologies, partitions, loss and concurrency != n; a 4096-cluster launch at cfg2's
shape against the committed digests; the program's known answer; refusal of what the build does not hold; the layout trace and the
kernel's register budget."""
import json
import os
import subprocess
import sys

import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E
import bcast_batch_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bcast_batch_digests.json")

SHAPES = [
    dict(node_count=5, rate=20, time_limit=5, seed=11),
    dict(node_count=9, rate=30, time_limit=6, latency=20, latency_dist="uniform", topology="line", seed=12),
    dict(node_count=8, rate=30, time_limit=6, latency=30, latency_dist="exponential", p_loss=0.1, topology="total", seed=13),
    dict(node_count=9, rate=30, time_limit=8, latency=20, nemesis=["partition"], nemesis_interval=2, seed=14),
    dict(node_count=10, rate=40, time_limit=6, latency=400, latency_dist="exponential", nemesis=["partition"], nemesis_interval=2,
         p_loss=0.05, topology="tree4", seed=15),
    dict(node_count=4, concurrency=9, rate=40, time_limit=5, latency=10, topology="grid", seed=16),
    dict(node_count=7, concurrency=3, rate=20, time_limit=5, latency=50, topology="line", p_loss=0.2, seed=17),
]


def _run(kw, n, journal=0, flags=None):
    cfg = E.test_config("broadcast", bin="broadcast-batch", **kw, **({"journal_capacity": journal} if journal else {}))
    eng = E.Engine(cfg, device=0)
    if flags is not None:
        eng.set_dev_flags(flags)
    eng.run(0, n)
    eng.fetch()
    return eng


@pytest.mark.parametrize("journal", [0, 200000])
@pytest.mark.parametrize("kw", SHAPES, ids=[f"s{i}" for i in range(len(SHAPES))])
def test_engine_equals_the_model(kw, journal):
    with _run(kw, 3, journal) as eng:
        bad = [f"instance {i}: {d}" for i in range(3) for d in M.compare_engine_instance(eng, i, kw)]
    assert not bad, "\n".join(bad[:10])


def _edges(kw):
    from maelstrom_amd import bridge as B
    return sum(len(x) for x in B.topology(kw.get("topology", "grid"), kw["node_count"])) // 2


@pytest.mark.parametrize("latency", [0, 100, 499])
def test_known_answer_every_value_crosses_every_directed_edge_once(latency):
    """No loss, no partitions, constant latency below 500 ms: every RPC is answered before its 1 s timeout, so each link sends each value
    exactly once — the values carried by all broadcast_many bodies add up to 2E x the broadcast values; at latency 0 every batch holds one
    value: 4E server messages per broadcast (160 on a 5 x 5 grid)."""
    kw = dict(node_count=25, rate=50, time_limit=6, latency=latency, seed=21)
    E2 = _edges(kw)
    assert E2 == 40
    with _run(kw, 4, journal=400000) as eng:
        for i in range(4):
            rows, _ = eng.raw_history(i)
            bcasts = int((((rows["packed"] & 3) == A.T_INVOKE) & (((rows["packed"] >> 2) & 31) == A.F_BROADCAST)).sum())
            ev = eng.raw_journal(i)
            send = (ev["msg"] & 0x80) == 0
            many = send & ((ev["msg"] & 0x7F) == A.MSG_TYPES.index("broadcast_many"))
            carried = int(((ev["a"][many] >> 16) - (ev["a"][many] & 0xFFFF)).sum())
            assert bcasts > 0 and carried == 2 * E2 * bcasts
            if latency == 0:
                assert eng.net_stats_raw(i).servers_send == 4 * E2 * bcasts


def test_fault_free_histories_are_valid():
    for kw in (SHAPES[0], SHAPES[1], SHAPES[5], dict(node_count=25, rate=100, time_limit=10, latency=100, seed=22)):
        with _run(kw, 16) as eng:
            eng.check()
            res = eng.check_results()
            assert all(int(v) == 1 for v in res["valid"]), (kw, res["valid"])
            assert all(int(v) == 0 for v in res["lost_count"])


def _child(code, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


_DIGESTS = """
import json, sys
sys.path.insert(0, 'tests')
from maelstrom_amd import engine as E
import bcast_batch_ref as M
kw = json.loads(sys.argv[1]) if len(sys.argv) > 1 else {kw!r}
cfg = E.test_config('broadcast', bin='broadcast-batch', **kw)
with E.Engine(cfg, device=0) as eng:
    eng.run(0, 6); eng.fetch()
    print(json.dumps([M.engine_digest(eng, i) for i in range(6)]))
"""


def test_results_do_not_depend_on_poisoned_buffers():
    kw = SHAPES[4]
    code = _DIGESTS.format(kw=kw)
    a = _child(code, {}).stdout.strip().splitlines()[-1]
    b = _child(code, {"MSIM_POISON": "0xA5"}).stdout.strip().splitlines()[-1]
    c = _child(code, {"MSIM_POISON": "0x00"}).stdout.strip().splitlines()[-1]
    assert a == b == c


def test_layout_trace_names_the_kernel():
    r = _child(_DIGESTS.format(kw=SHAPES[0]), {"MSIM_DEV_FLAGS": "0x1000"})
    assert "[layout] general_d 6" in r.stderr, r.stderr[-2000:]


def test_more_than_32_nodes_is_refused():
    cfg = E.test_config("broadcast", bin="broadcast-batch", node_count=33, rate=10, time_limit=2)
    with pytest.raises(E.EngineError) as ex:
        E.Engine(cfg, device=0)
    assert f"({A.E_UNSUPPORTED})" in str(ex.value) and "broadcast-batch" in str(ex.value)
    cfg = E.test_config("broadcast", bin="broadcast-batch", node_count=20, concurrency=45, rate=10, time_limit=2)
    with pytest.raises(E.EngineError) as ex:
        E.Engine(cfg, device=0)
    assert f"({A.E_UNSUPPORTED})" in str(ex.value)


def test_kernel_has_no_private_memory():
    lib = os.path.join(ROOT, "maelstrom_amd", "libmaelsim.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "private_memory_audit.py"), lib], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "kernels" in r.stdout
    assert open(lib, "rb").read().count(b"_Z10sim_kernelILi16ELb") >= 4   # the four <NEM, NET_RANDOM> instantiations are in the library
    assert not [ln for ln in r.stdout.splitlines() if "sim_kernel<16," in ln], r.stdout


def test_bench_shape_launch_matches_the_golden_digests():
    """4096 clusters at cfg2's shape (tools/bench_configs.py, seed 99); the instances at the end of the slabs are held to the digests of
    the model runs recorded by tests/golden/make_golden_bcast_batch.py"""
    gold = json.load(open(GOLDEN))["bench"]
    for g in gold:
        cfg = E.test_config("broadcast", bin="broadcast-batch", seed=g["seed"], **g["kw"])
        with E.Engine(cfg, device=0) as eng:
            eng.run(0, 4096)
            eng.fetch()
            for i, d in zip(g["instances"], g["digests"]):
                assert eng.meta(i).flags == 0
                assert M.engine_digest(eng, i) == d, (g["kw"], i)
