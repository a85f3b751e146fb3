"""The launch-size floors of the packed layouts (the min_clusters column of csrc/launch_plan.h, csrc/layout_thresholds.h) at the edges
tests/test_large_launch_gpu.py does not reach: bcast8 (12288), dtg4 with two nodes (half of 16384), hat8 with three nodes (3 x 3200) —
one cluster below the floor the one-cluster kernel runs, at the floor the packed one — and the two developer bits around the floor:
bit 10 takes a packed layout at two clusters, bit 9 keeps one cluster per wavefront at the bench size.  Which kernel a launch took is
its `[layout] <kernel> <n>` line (MSIM_DEV_FLAGS bit 12); the first two and the last two instances of every launch are bit-compared
with the CPU oracle.  One second at 20 ops/s: a launch is milliseconds and the slabs are small."""
import re

import pytest

from maelstrom_amd import engine as E
from launch_digests import digest_engine, digest_oracle
import oracle_lib as O

pytestmark = pytest.mark.gpu

TRACE = 0x1000
SHORT = dict(rate=20, time_limit=1, seed=7)


def _bcast5():      # loss: not the two-clusters-per-wavefront layout
    return E.test_config("broadcast", bin="broadcast-ff", node_count=5, p_loss=0.05, **SHORT)


def _datomic2x6():
    return E.test_config("txn-list-append", bin="datomic", node_count=2, concurrency=12, **SHORT)


def _hat3():
    return E.test_config("txn-rw-register", node_count=3, **SHORT)


def _echo3():
    return E.test_config("echo", node_count=3, **SHORT)


# (id, config, developer flags, clusters, expected kernel)
CASES = [
    ("bcast8-below", _bcast5, 0, 12287, "general_b"), ("bcast8-floor", _bcast5, 0, 12288, "bcast8"),
    ("dtg4-2-nodes-below", _datomic2x6, 0, 8191, "dtg"), ("dtg4-2-nodes-floor", _datomic2x6, 0, 8192, "dtg4"),
    ("hat8-3-nodes-below", _hat3, 0, 9599, "hat1"), ("hat8-3-nodes-floor", _hat3, 0, 9600, "hat8"),
    ("uid8-bit10-two-clusters", _echo3, 0x400, 2, "uid8"), ("uid8-bit9-bench-size", _echo3, 0x200, 4096, "general_a"),
]


@pytest.mark.parametrize("name,make,flags,n,kernel", CASES, ids=[c[0] for c in CASES])
def test_floor_edge_takes_the_kernel_and_equals_the_oracle(lib, capfd, name, make, flags, n, kernel):
    cfg = make()
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(TRACE | flags)
        try:
            eng.run(0, n)
        finally:
            eng.set_dev_flags(0)
        err = capfd.readouterr().err
        assert re.findall(r"^\[layout\] (\S+) (\d+)$", err, re.M) == [(kernel, str(n))], (name, err[-2000:])
        eng.fetch()
        for first in sorted({0, n - 2}):
            ora = O.run(cfg, first, 2)
            for k in range(2):
                assert digest_engine(eng, first + k) == digest_oracle(ora, k), f"{name}: instance {first + k} of {n} differs from the oracle"
                assert eng.meta(first + k).flags == 0, name
