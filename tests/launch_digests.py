"""Digests of one instance's outputs — rows, payload, net stats, flags and round counts — from the engine and from the CPU oracle, for
the tests that bit-compare launches with the oracle (test_bench_shapes_gpu.py, test_large_launch_gpu.py).  TEST INFRASTRUCTURE ONLY."""
import hashlib

import numpy as np

from maelstrom_amd import _abi as A


def digest_engine(eng, i):
    rows, pay = eng.raw_history(i)
    st = eng.net_stats_raw(i)
    m = eng.meta(i)
    h = hashlib.sha256(rows.tobytes())
    h.update(pay.tobytes())
    h.update(np.array([getattr(st, f) for f, _ in A.NetStats._fields_], dtype=np.uint64).tobytes())
    h.update(np.array([m.n_rows, m.n_payload_words, m.flags, m.n_rounds], dtype=np.uint32).tobytes())
    return h.hexdigest()


def digest_oracle(ora, i):
    rows, pay = ora.history(i)
    m = ora.meta[i]
    h = hashlib.sha256(rows.tobytes())
    h.update(pay.tobytes())
    h.update(np.array([int(x) for x in ora.stats[i]], dtype=np.uint64).tobytes())
    h.update(np.array([m["n_rows"], m["n_payload_words"], m["flags"], m["n_rounds"]], dtype=np.uint32).tobytes())
    return h.hexdigest()
