"""The engine configurations the :stats / :perf tests run (tests/test_perf_stats.py on oracle histories, tests/test_perf_stats_gpu.py on
the engine's), and the window grids they are checked with."""
from maelstrom_amd import engine as E

CONFIGS = {
    "broadcast": lambda: E.test_config("broadcast", node_count=5, rate=20, time_limit=5, seed=1),
    "echo-lossy": lambda: E.test_config("echo", node_count=3, rate=20, time_limit=8, p_loss=0.2, seed=5),   # :info timeouts
    "raft-partitions": lambda: E.test_config("lin-kv", bin="raft", node_count=5, concurrency=10, rate=30, time_limit=8, latency=10,
                                             nemesis=["partition"], nemesis_interval=2, seed=7),             # :fail, :info, three :f
    "kafka": lambda: E.test_config("kafka", node_count=5, rate=60, time_limit=5, latency=5, seed=3),          # four :f, :crash among them
}
WINDOWS = [(None, 0), (1.0, 8)]   # (window_s, n_windows): off, 1 s x 8
