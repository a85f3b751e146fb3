"""tests/test_duo_flood_table_hipemu.py's cases on the device: the flood table of the two-clusters-per-wavefront broadcast kernel
(csrc/duo.hip, "FLOOD TABLE": one wavefront records the floods of a context's configuration once, before the context's first launch, and
every wavefront of every launch starts from a copy of that table), bit for bit against the oracle (rows, payload, meta with n_rounds,
the six net-stats counters).  Every case is a handful of clusters at a time limit of at most 1 s of virtual time.  The device runs the
product build, so what the table holds is read from the line the library prints when it makes one (MSIM_DEV_FLAGS bit 12), in a process
of its own: all 5 origins in FULL_CASE, some of 25 in PARTIAL_CASE, none in FEW_OPS.  The counts of the profile build, the verifying
build (a mismatch there is a trap) and the comparison with a -DDUO_NO_FLOOD_TABLE build under round limits run on the emulator.
Here as well: the table does not depend on the instances that made it (MSIM_DUO_TABLE_FIRST, child processes, every byte equal); one
table per context (three runs of one engine, two engines with other topologies); three contexts in flight; a launch on a caller's
stream as a context's first launch; MSIM_POISON=0xA5 and MSIM_GUARD=1 in child processes; the capacity sweeps of the block-plan module."""
import os
import subprocess
import sys

import pytest
import torch   # before the engine's library is loaded, as in bench.py: the process then holds one HIP runtime, torch's

from test_duo_halves_gpu import _run
from test_duo_flood_table_hipemu import (CASES, FEW_OPS, FIRST_CASE, FULL_CASE, LINE5, PARTIAL_CASE, POISONED, ROOT, TRACE, _against_the_oracle, _child, _config,
                                         _last_json, three_in_flight)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES + [FULL_CASE, PARTIAL_CASE, FIRST_CASE, LINE5])
def test_duo_flood_table_equals_the_oracle(lib, case):
    _run(case, True)


@pytest.mark.parametrize("case,known", [(FULL_CASE, "all"), (PARTIAL_CASE, "some"), (FEW_OPS, "none")], ids=["full", "partial", "empty"])
def test_duo_flood_table_holds_what_the_table_wavefront_met(lib, case, known):
    """(the run itself is compared with the oracle by the test above; FEW_OPS is one of CASES)"""
    _, err = _child(None, ["digests", case], timeout=120)
    (k, n), = TRACE.findall(err)
    assert {"all": int(k) == int(n) == 5, "some": 0 < int(k) < int(n) == 25, "none": int(k) == 0 and int(n) == 25}[known], err[-2000:]


def test_duo_flood_table_does_not_depend_on_the_instances_that_made_it(lib):
    got = [_last_json(_child(None, ["digests", FIRST_CASE], timeout=120, MSIM_DUO_TABLE_FIRST=first)[0]) for first in ("0", "1000001")]
    assert got[0] == got[1]


def test_duo_flood_table_is_made_once_per_context(lib):
    out, err = _child(None, ["one_engine"], timeout=120)
    assert "one engine: OK" in out and len(TRACE.findall(err)) == 1 and err.count("[layout] duo") == 3, err[-2000:]
    out, err = _child(None, ["two_engines"], timeout=120)
    assert "two engines: OK" in out and len(TRACE.findall(err)) == 2 and err.count("[layout] duo") == 4, err[-2000:]


def test_duo_flood_table_with_three_contexts_in_flight(lib, capfd):
    three_in_flight()
    assert len(TRACE.findall(capfd.readouterr().err)) == 3


def test_duo_flood_table_when_the_first_launch_is_on_a_callers_stream(lib, capfd):
    """the table is made on the context's own stream and waited for, so the caller's stream needs no ordering against it"""
    E, cfg, n, flags = _config(FIRST_CASE)
    stream = torch.cuda.Stream()
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(flags | 0x1000)
        for first in (300, 0):
            eng.run_async(first, n, stream.cuda_stream)
            stream.synchronize()
            _against_the_oracle(eng, cfg, first, n)
    assert len(TRACE.findall(capfd.readouterr().err)) == 1


@pytest.mark.parametrize("env", [{"MSIM_POISON": "0xA5"}, {"MSIM_GUARD": "1"}], ids=["poison", "guard"])
def test_duo_flood_table_with_poisoned_or_fenced_buffers(lib, env):
    """MSIM_POISON and MSIM_GUARD are read once per process: the cases run in a process of their own"""
    cases = POISONED + [PARTIAL_CASE, FULL_CASE]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emu_compare.py")] + cases, cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") == len(cases), r.stdout
    if "MSIM_GUARD" in env:
        assert "guard: 0 damaged byte(s)" in r.stdout, r.stdout[-2000:]


def test_duo_flood_table_stopped_by_a_capacity(lib):
    from test_duo_block_plan_hipemu import plan_capacity_sweeps
    plan_capacity_sweeps()
