"""tests/test_duo_hbm_sets_hipemu.py's cases on the device: the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip) with the nodes'
seen sets in HBM scratch, bit for bit against the oracle (history, payload, meta, net stats).  Then launches of 4096 and 4097 clusters (an
even grid, and one whose last wavefront's upper half holds no cluster) at the headline shape and at the three shapes of the latency sweep
(tools/cfg2_overlap.py): each runs once plain and once with every device buffer filled with 0xA5 before the launch (MSIM_POISON, read
once per process: each run is a child process), the two must be identical instance for instance, and the first and last instances
equal the oracle."""
import ast
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from maelstrom_amd import engine as E  # noqa: E402
from launch_digests import digest_engine, digest_oracle  # noqa: E402

SHAPES = {   # keywords of engine.test_config beside the headline's (bench.py headline_config, seed 99)
    "lat0": dict(bin="broadcast-ff", latency=0, inbox_capacity=6),
    "lat10": dict(latency=10),
    "lat100": dict(latency=100),
    "exp100": dict(latency=100, latency_dist="exponential"),
}
DUO = 0x400   # dev flag: the duo layout is required (an error, not another kernel, if it does not apply)


def _shape_config(shape):
    return E.test_config("broadcast", node_count=25, rate=100, time_limit=20, topology="grid", seed=99, **SHAPES[shape])


def _digests(shape, n):
    """(child process) the shape's n clusters in one launch: every instance's digest"""
    with E.Engine(_shape_config(shape), device=0) as eng:
        eng.set_dev_flags(DUO)
        eng.run(0, n)
        eng.fetch()
        return [digest_engine(eng, i) for i in range(n)]


def _child(shape, n, poison):
    env = dict(os.environ)
    env.pop("MSIM_POISON", None)
    if poison:
        env["MSIM_POISON"] = "0xA5"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), shape, str(n)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    print(json.dumps(_digests(sys.argv[1], int(sys.argv[2]))))
    sys.exit(0)

import oracle_lib as O  # noqa: E402
from test_duo_hbm_sets_hipemu import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_duo_hbm_sets_equal_the_oracle(lib, case):
    kw = ast.literal_eval(case)
    n = kw.pop("n", 2)
    flags = kw.pop("flags", 0)
    cfg = E.test_config(seed=kw.pop("seed", 7), **kw)
    ora = O.run(cfg, 0, n)
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags)
        eng.run(0, n)
        eng.fetch()
        for i in range(n):
            assert digest_engine(eng, i) == digest_oracle(ora, i), f"{case}: instance {i} differs from the oracle"


@pytest.mark.parametrize("n", [4096, 4097])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_duo_hbm_sets_large_launch_plain_equals_poisoned(lib, shape, n):
    plain = _child(shape, n, False)
    poisoned = _child(shape, n, True)
    assert len(plain) == len(poisoned) == n
    diff = [i for i in range(n) if plain[i] != poisoned[i]]
    assert not diff, f"{shape} x {n}: {len(diff)} instances differ under MSIM_POISON=0xA5, first {diff[:5]}"
    cfg = _shape_config(shape)
    for i in (0, n - 1):
        ora = O.run(cfg, i, 1)
        assert plain[i] == digest_oracle(ora, 0), f"{shape} x {n}: instance {i} differs from the oracle"
