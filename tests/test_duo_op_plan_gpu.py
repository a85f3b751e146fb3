"""tests/test_duo_op_plan_hipemu.py's cases on the device: read runs of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip,
latency 0), bit for bit against the oracle (history, payload, meta, net stats); the shapes that a capacity stops, compared by their flags
as that module says; the sweep of round limits through a run of reads (against the oracle's prefix); and the headline shape at 4096 and 4097 clusters (a last wavefront with an empty upper half), a sample of instances
against the oracle."""
import pytest

from maelstrom_amd import engine as E
import oracle_lib as O
from test_duo_halves_gpu import _run
from test_duo_op_plan_hipemu import CASES, LIMITS, POISONED, check_stops, limit_sweep

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES + POISONED)
def test_duo_read_runs_equal_the_oracle(lib, case):
    _run(case, True)


def test_duo_read_runs_stopped_by_a_capacity(lib):
    check_stops()


def test_duo_read_runs_with_a_round_limit_inside_a_run(lib):
    digests, inside = limit_sweep()
    assert len(digests) == len(LIMITS)
    assert inside >= 5, f"only {inside} limits fell behind the first read of a run"


@pytest.mark.parametrize("n", [4096, 4097])
def test_duo_read_runs_at_the_headline_shape(lib, n):
    import bench
    cfg = bench.headline_config(E, 53)
    sample = [0, 1, 2, 3, 1023, 2046, 2047, 2048, n - 3, n - 2, n - 1]
    with E.Engine(cfg) as eng:
        eng.set_dev_flags(0x400)
        eng.run(0, n)
        eng.fetch()
        for i in sample:
            ora = O.run(cfg, i, 1)
            rows, pay = eng.raw_history(i)
            orows, opay = ora.history(0)
            assert rows.tobytes() == orows.tobytes() and pay.tobytes() == opay.tobytes(), f"instance {i} of {n} differs from the oracle"
            m, om = eng.meta(i), ora.meta[0]
            assert (m.n_rows, m.n_payload_words, m.flags, m.n_rounds) == (om["n_rows"], om["n_payload_words"], om["flags"], om["n_rounds"]), f"meta of instance {i} of {n}"
            assert m.flags == 0, f"instance {i} of {n} is flagged"
            st = eng.net_stats_raw(i)
            for f in ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv"):
                assert int(getattr(st, f)) == int(ora.stats[0][f]), f"{f} of instance {i} of {n}"
