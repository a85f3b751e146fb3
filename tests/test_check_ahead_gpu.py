"""The set-full / echo check queued behind its simulation at launch time (csrc/engine.hip run_impl + msim_check, csrc/checker.hip
msim_check_enqueue / msim_check_wait): a context whose caller checks its launches is armed, its next launches on the context's own stream
queue the checker straight behind the simulation kernel, and check() only waits for it.  Under developer flag 0x1000 the engine names the
route beside its `[layout]` line: `[check] queued <n>` (the launch), `[check] taken <n>` / `[check] launched <n>` (check()).

  1. arm and take;  2. batch sizes 2 -> 9 -> 3 on one armed context (the checker's scratch grows in front of the launch);  3. two launches
  back to back without a check (the second launch's records; the context is disarmed);  4. check() twice on one run;  5. flag 0x40000 never
  queues, and d_check holds the same bytes as on the armed path;  6. fetch_begin() between an armed launch and its check;  7. the other
  users of the route: g-set, echo, echo at rate 0;  8. lin-kv never queues;  9. a caller's stream (device only);  10. cases 1 and 2 with
  every device buffer filled with 0xA5 before each launch (MSIM_POISON is read once per process: a process of their own).

Every comparison is exact and against the oracle and the host checker / the Python restatements (tests/pipeline_cases.py), never against
another run of the engine; nothing asserts a time.  The launches go through a helper of this file, not pipeline_cases.launch_async: that
one reads the captured stderr itself and keeps only the `[layout]` line.  tests/test_check_ahead_hipemu.py runs this file on the host
wavefront emulator (synchronous: the state machine)."""
import os
import re
import subprocess
import sys

import pytest

from maelstrom_amd import engine as E
import pipeline_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_QUEUE = 0x40000


def _lines(capfd):
    err = capfd.readouterr().err
    return re.findall(r"^\[layout\] (\S+) (\d+)$", err, re.M), re.findall(r"^\[check\] (queued|taken|launched) (\d+)$", err, re.M)


def _launch(eng, capfd, first, n, kernel="duo", flags=0, stream=None):
    """run_async under the trace flag (set around the call only); returns the routes the launch named: ["queued"] or []."""
    capfd.readouterr()
    eng.set_dev_flags(P.TRACE | flags)
    try:
        eng.run_async(first, n, stream)
    finally:
        eng.set_dev_flags(flags)
    lay, chk = _lines(capfd)
    assert [c for _, c in lay] == [str(n)] and (kernel is None or lay[0][0] == kernel), (kernel, n, lay)
    assert all(c == str(n) for _, c in chk), (n, chk)
    return [r for r, _ in chk]


def _check(eng, capfd, flags=0):
    """check() under the trace flag; returns the routes it named: ["taken"], ["launched"] or [] (a checker off the route)."""
    capfd.readouterr()
    eng.set_dev_flags(P.TRACE | flags)
    try:
        eng.check()
    finally:
        eng.set_dev_flags(flags)
    _, chk = _lines(capfd)
    assert all(c == str(eng.n) for _, c in chk), (eng.n, chk)
    return [r for r, _ in chk]


def _verify(eng, cfg, first, n, what):
    """The records of the last check against the reference checkers and the fetched batch against the oracle; returns the records."""
    res = eng.check_results()
    P.finite_ms(eng, what)
    eng.fetch()
    P.compare_batch(eng, cfg, first, n, what)
    P.compare_records(eng, cfg, res, what)
    return res


def _not_visible(eng):
    with pytest.raises(E.EngineError):
        eng.check_results()


# ---- 1. arm and take -----------------------------------------------------------------------------------------------------------------------
def test_arm_and_take(lib, capfd):
    cfg = P.config("headline")
    n1, n2 = P.sizes("headline")[2], P.sizes("headline")[0]
    with E.Engine(cfg) as eng:
        assert _launch(eng, capfd, 11, n1) == []
        _not_visible(eng)
        assert _check(eng, capfd) == ["launched"]
        _verify(eng, cfg, 11, n1, "the launch that arms the context")
        assert _launch(eng, capfd, 2011, n2) == ["queued"]
        _not_visible(eng)   # a queued check is not a check: nothing of it shows before check()
        assert _check(eng, capfd) == ["taken"]
        _verify(eng, cfg, 2011, n2, "the launch whose check was queued behind it")


# ---- 2. the scratch grows in front of the launch -----------------------------------------------------------------------------------------
def test_batch_sizes_grow_and_shrink_on_an_armed_context(lib, capfd):
    cfg = P.config("headline")
    with E.Engine(cfg) as eng:
        for k, n in enumerate((2, 9, 3)):
            first = 3000 + 100 * k
            assert _launch(eng, capfd, first, n) == (["queued"] if k else [])
            assert _check(eng, capfd) == (["taken"] if k else ["launched"])
            _verify(eng, cfg, first, n, f"batch {k} of 2 -> 9 -> 3 (n {n})")


# ---- 3. back to back without a check -----------------------------------------------------------------------------------------------------
def test_two_launches_without_a_check_disarm_the_context(lib, capfd):
    cfg = P.config("headline")
    n = P.sizes("headline")[2]
    with E.Engine(cfg) as eng:
        assert _launch(eng, capfd, 5, 2) == []
        assert _check(eng, capfd) == ["launched"]                    # armed
        assert _launch(eng, capfd, 4000, 4) == ["queued"]            # never taken
        assert _launch(eng, capfd, 4100, n) == []                    # disarmed by the run that found it untaken
        _not_visible(eng)
        assert _check(eng, capfd) == ["launched"]
        _verify(eng, cfg, 4100, n, "the second of two launches without a check")
        assert _launch(eng, capfd, 4200, 3) == ["queued"]            # (that check armed it again)
        assert _launch(eng, capfd, 4300, 2) == []
        assert _launch(eng, capfd, 4400, 3) == []                    # still disarmed: no `queued` until somebody checks
        assert _check(eng, capfd) == ["launched"]
        _verify(eng, cfg, 4400, 3, "the last of three launches without a check")


# ---- 4. check() twice ----------------------------------------------------------------------------------------------------------------------
def test_check_twice_on_one_run(lib, capfd):
    cfg = P.config("headline")
    n = P.sizes("headline")[2]
    with E.Engine(cfg) as eng:
        assert _launch(eng, capfd, 7, 2) == []
        assert _check(eng, capfd) == ["launched"]
        assert _launch(eng, capfd, 5000, n) == ["queued"]
        assert _check(eng, capfd) == ["taken"]
        res1 = eng.check_results()
        assert _check(eng, capfd) == ["launched"]
        res2 = _verify(eng, cfg, 5000, n, "the second check of one run")
        assert res1.tobytes() == res2.tobytes()
        assert _check(eng, capfd) == ["launched"]   # (and a third, after the fetch)
        assert eng.check_results().tobytes() == res1.tobytes()


# ---- 5. the developer flag ------------------------------------------------------------------------------------------------------------------
def test_flag_0x40000_never_queues_and_gives_the_same_bytes(lib, capfd):
    cfg = P.config("headline")
    n = P.sizes("headline")[2]
    got = {}
    for flags in (0, NO_QUEUE):
        with E.Engine(cfg) as eng:
            eng.set_dev_flags(flags)
            assert _launch(eng, capfd, 9, 3, flags=flags) == []
            assert _check(eng, capfd, flags) == ["launched"]
            assert _launch(eng, capfd, 6000, n, flags=flags) == ([] if flags else ["queued"])
            assert _check(eng, capfd, flags) == (["launched"] if flags else ["taken"])
            db = eng.device_buffers()
            assert db.check_bytes == n * 68
            got[flags] = P.device_bytes(db.check, db.check_bytes).tobytes()
            res = _verify(eng, cfg, 6000, n, f"dev flags {flags:#x}")
            assert res.tobytes() == got[flags]
            if flags:   # a context armed before the flag was set does not queue under it either
                eng.set_dev_flags(0)
                assert _launch(eng, capfd, 6100, 2) == []
                assert _check(eng, capfd) == ["launched"]
                assert _launch(eng, capfd, 6200, 2, flags=flags) == []
                assert _check(eng, capfd, flags) == ["launched"]
                _verify(eng, cfg, 6200, 2, "the flag set on an armed context")
    assert got[0] == got[NO_QUEUE]


# ---- 6. fetch_begin between the launch and its check ----------------------------------------------------------------------------------------
def test_fetch_begin_between_an_armed_launch_and_its_check(lib, capfd):
    cfg = P.config("headline")
    n = P.sizes("headline")[2]
    with E.Engine(cfg) as eng:
        assert _launch(eng, capfd, 13, 2) == []
        assert _check(eng, capfd) == ["launched"]
        assert _launch(eng, capfd, 7000, n) == ["queued"]
        eng.fetch_begin()
        _not_visible(eng)
        assert _check(eng, capfd) == ["taken"]
        _verify(eng, cfg, 7000, n, "fetch_begin between an armed launch and its check")
        assert _launch(eng, capfd, 7100, 3) == ["queued"]   # a launch over the fetched state, and the whole fetch in between
        eng.fetch()
        P.compare_batch(eng, cfg, 7100, 3, "fetch between an armed launch and its check")
        assert _check(eng, capfd) == ["taken"]
        P.compare_records(eng, cfg, eng.check_results(), "fetch between an armed launch and its check")


# ---- 7. the other users of the route ---------------------------------------------------------------------------------------------------------
ROUTE = {
    "g-set-5": lambda: E.test_config("g-set", node_count=5, rate=20, time_limit=2, latency=10, seed=P.SEED),
    "echo-3": lambda: E.test_config("echo", node_count=3, rate=20, time_limit=2, latency=5, seed=P.SEED),
    "echo-3-rate-0": lambda: E.test_config("echo", node_count=3, rate=0, time_limit=2, seed=P.SEED),   # every history empty
}


@pytest.mark.parametrize("name", list(ROUTE))
def test_other_workloads_of_the_route(lib, capfd, name):
    cfg = ROUTE[name]()
    with E.Engine(cfg) as eng:
        for k, n in enumerate((3, 5, 2)):
            first = 8000 + 50 * k
            assert _launch(eng, capfd, first, n, kernel=None) == (["queued"] if k else [])
            assert _check(eng, capfd) == (["taken"] if k else ["launched"])
            res = _verify(eng, cfg, first, n, f"{name} batch {k}")
            if name == "echo-3-rate-0":
                assert all(int(P.oracle(cfg, first, n).meta(i)["n_rows"]) == 0 for i in range(n))
                assert (res["valid"] == 1).all() and len(res) == n


# ---- 8. a checker off the route ---------------------------------------------------------------------------------------------------------------
def test_lin_kv_never_queues(lib, capfd):
    cfg = E.test_config("lin-kv", bin="raft", node_count=5, rate=30, time_limit=2, seed=P.SEED)
    with E.Engine(cfg) as eng:
        for k, n in enumerate((3, 4, 2)):
            first = 9000 + 50 * k
            assert _launch(eng, capfd, first, n, kernel=None) == []
            capfd.readouterr()
            eng.check()   # (without the trace flag: under it the lin-kv search writes its timings into fields of the records)
            assert "[check]" not in capfd.readouterr().err
            _verify(eng, cfg, first, n, f"lin-kv batch {k}")
        assert _launch(eng, capfd, 9500, 2, kernel=None) == []
        assert _check(eng, capfd) == []   # neither taken nor launched: msim_check_launch is not its checker


# ---- 9. a caller's stream ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(P.EMU, reason="the emulator has no streams")
def test_a_launch_on_the_callers_stream_never_queues(lib, capfd):
    torch = P.torch
    cfg = P.config("headline")
    n = P.sizes("headline")[2]
    stream = torch.cuda.Stream()
    with E.Engine(cfg) as eng:
        assert _launch(eng, capfd, 17, 2) == []
        assert _check(eng, capfd) == ["launched"]                                           # armed
        assert _launch(eng, capfd, 10000, n, stream=stream.cuda_stream) == []
        stream.synchronize()
        assert _check(eng, capfd) == ["launched"]
        _verify(eng, cfg, 10000, n, "a launch on the caller's stream, armed context")
        assert _launch(eng, capfd, 10100, 4) == ["queued"]                                  # still armed for its own stream
        assert _launch(eng, capfd, 10200, n, stream=stream.cuda_stream) == []               # over an untaken check: waits for it
        stream.synchronize()
        assert _check(eng, capfd) == ["launched"]
        _verify(eng, cfg, 10200, n, "a launch on the caller's stream over an untaken check")


# ---- 10. poisoned buffers ------------------------------------------------------------------------------------------------------------------------
def test_cases_1_and_2_with_poisoned_buffers(lib):
    env = dict(os.environ, MSIM_POISON="0xA5")   # (the child selects the two cases by name, never this one)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "test_arm_and_take or test_batch_sizes_grow_and_shrink_on_an_armed_context"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
