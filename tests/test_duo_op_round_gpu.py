"""tests/test_duo_op_round_hipemu.py's cases on the device: the op round of the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip,
latency 0), bit for bit against the oracle (history, payload, meta, net stats); a shape that stops clusters through the row capacity
(history rows, their count and the flags: the oracle accounts for rounds and read payloads differently after such a stop); and the
headline shape at 4096 and 4097 clusters (a last wavefront with an empty upper half), a sample of instances against the oracle."""
import pytest

from maelstrom_amd import engine as E
import oracle_lib as O
from test_duo_halves_gpu import _run
from test_duo_op_round_hipemu import CASES

pytestmark = pytest.mark.gpu

STOPS = [
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':6,'max_rows':70,'seed':22,'flags':0x400}",
]


@pytest.mark.parametrize("case", CASES)
def test_duo_op_rounds_equal_the_oracle(lib, case):
    _run(case, True)


@pytest.mark.parametrize("case", STOPS)
def test_duo_op_rounds_stopped_by_the_row_capacity(lib, case):
    _run(case, False)


@pytest.mark.parametrize("n", [4096, 4097])
def test_duo_op_rounds_at_the_headline_shape(lib, n):
    import bench
    cfg = bench.headline_config(E, 31)
    sample = [0, 1, 2, 2047, 2048, n - 3, n - 2, n - 1]
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
