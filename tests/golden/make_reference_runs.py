#!/usr/bin/env python3
"""Records tests/golden/reference_runs.json (tests/reference_runs.py): every replay of the reference's own node programs against the
oracle — real demo/js processes over their pipes (tests/test_js_reference_replay.py), demo/python/raft.py fed the oracle's schedule
(tests/test_raft_reference_replay.py), demo/python/echo.py and demo/js/*_txn.js behind the process bridge (tests/test_process_bridge.py)
— must pass first; then what the tests recompute from the oracle alone is stored for that case.  Also checks that raft.py as shipped
diverges (the quirk of DESIGN.md §2.4).  Needs the reference tree and node.js:

    MAELSTROM_REFERENCE=<reference tree> python tests/golden/make_reference_runs.py"""
import json
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import reference_runs as R  # noqa: E402
import test_js_reference_replay as JS  # noqa: E402
import test_process_bridge as PB  # noqa: E402
import test_raft_reference_replay as RAFT  # noqa: E402


def main():
    R.reference_path()   # fails early without the reference tree
    out = {}

    def put(value, name, *case):
        out[R.key(name, *case)] = value
        print(name, json.dumps(case)[:100], str(value)[:24], flush=True)

    def tmp(fn, *a):
        with tempfile.TemporaryDirectory() as d:
            fn(*a, pathlib.Path(d))
    for workload, script, kw in JS.CRDT_CASES:
        tmp(JS.replay_crdt, workload, script, kw)
        put(JS.run_digest(workload, kw), "js-crdt", workload, script, kw)
    tmp(JS.replay_echo)
    put(JS.run_digest("echo", JS.ECHO_CASE), "js-echo", JS.ECHO_CASE)
    for kw in JS.TXN_CASES:
        tmp(JS.replay_single_key_txn, kw)
        put(JS.run_digest("txn-list-append", kw), "js-single-key-txn", kw)
    for kw in JS.GOSSIP_CASES:
        tmp(JS.replay_gossip, kw)
        put(JS.run_digest("broadcast", kw), "js-gossip", kw)
    for kw in RAFT.CASES + RAFT.EXTRA_CASES:
        RAFT.replay_raft(kw)
        put(RAFT.run_digests(kw), "raft-py", kw)
    RAFT.replay_unpatched_raft_diverges()
    for kw in PB.ECHO_CASES:
        PB.replay_echo_py(kw)
        put(PB._oracle_run("echo", **kw), "bridge-echo-py", kw)
    for kw in PB.SINGLE_KEY_CASES:
        PB.replay_single_key_txn_js(kw)
        put(PB._oracle_run("txn-list-append", **kw), "bridge-single-key-txn-js", kw)
    for kw in PB.MULTI_KEY_CASES:
        PB.replay_multi_key_txn_js(kw)
        put(PB._oracle_run("txn-list-append", oracle_bin="multi-key-txn", **kw), "bridge-multi-key-txn-js", kw)
    put(json.loads(json.dumps(PB.replay_multi_key_txn_js_strict())), "bridge-multi-key-txn-js-strict", PB.STRICT_CASE)
    with open(R.GOLD, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {R.GOLD}: {len(out)} runs")


if __name__ == "__main__":
    main()
