"""Runs of the reference's own node programs, recorded.  The replays that drive those programs (demo/js/*.js, demo/python/*.py of
the reference tree) with the oracle's schedule need the reference tree and node.js; tests/golden/make_reference_runs.py runs them
and, for every case that passes, stores a digest of the oracle's side of the run in tests/golden/reference_runs.json.  The tests
recompute that digest from the oracle alone: the oracle still produces the run the reference program reproduced message by message.
A case whose run changed has to be recorded again, against the reference, after the replay has been checked."""
import hashlib
import json
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_runs.json")


def reference_path(*parts):
    """A file of the reference tree (MAELSTROM_REFERENCE): only the recording replays read it."""
    root = os.environ.get("MAELSTROM_REFERENCE")
    if not root:
        raise RuntimeError("set MAELSTROM_REFERENCE to the reference tree to replay its programs (tests/golden/make_reference_runs.py)")
    return os.path.join(root, *parts)


def key(name, *case):
    return name + " " + json.dumps(case, sort_keys=True)


def digest(*values):
    return hashlib.sha256(json.dumps(values, sort_keys=True).encode()).hexdigest()


def recorded(name, *case):
    with open(GOLD) as f:
        runs = json.load(f)
    k = key(name, *case)
    assert k in runs, f"no recorded reference run for {k}: record it with tests/golden/make_reference_runs.py"
    return runs[k]
