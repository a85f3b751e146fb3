"""tests/test_duo_halves_hipemu.py's cases on the device: the two-clusters-per-wavefront broadcast kernel (csrc/duo.hip) where the two
halves of a wavefront diverge, bit for bit against the oracle (history, payload, meta, net stats).  Two more shapes stop a cluster through
a capacity the oracle reports with the same flag and history rows but accounts differently after the stop (rounds and read payloads for
the row capacity, one send for a value overflow at latency > 0): for those the history rows, their count and the flags are compared."""
import ast

import pytest

from maelstrom_amd import engine as E
import oracle_lib as O
from test_duo_halves_hipemu import CASES

pytestmark = pytest.mark.gpu

NAMED = {   # the named cases of tools/emu_compare.py that CASES uses
    "duo25uni": dict(workload="broadcast", node_count=25, rate=50, time_limit=4, latency=30, latency_dist="uniform", n=3),
    "duo25lat10": dict(workload="broadcast", node_count=25, rate=50, time_limit=4, latency=10, n=4),
    "duo9total": dict(workload="broadcast", node_count=9, rate=50, time_limit=4, latency=100, latency_dist="exponential", topology="total", n=4),
}

STOPS = [
    "{'workload':'broadcast','node_count':25,'rate':80,'time_limit':4,'n':6,'max_rows':60,'seed':3,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':100,'time_limit':4,'n':7,'max_rows':90,'seed':11,'flags':0x400}",
    "{'workload':'broadcast','node_count':25,'rate':80,'time_limit':4,'latency':10,'n':5,'max_values':30,'max_payload_words':80,'seed':6,'flags':0x400}",
    "{'workload':'broadcast','node_count':9,'rate':60,'time_limit':4,'latency':30,'latency_dist':'uniform','n':5,'max_values':25,'seed':8,'flags':0x400}",
]


def _run(case, full):
    kw = dict(NAMED[case]) if case in NAMED else ast.literal_eval(case)
    n = kw.pop("n", 2)
    flags = kw.pop("flags", 0)
    cfg = E.test_config(seed=kw.pop("seed", 7), **kw)
    ora = O.run(cfg, 0, n)
    with E.Engine(cfg) as eng:
        if flags:
            eng.set_dev_flags(flags)
        eng.run(0, n)
        eng.fetch()
        for i in range(n):
            rows, pay = eng.raw_history(i)
            orows, opay = ora.history(i)
            assert rows.tobytes() == orows.tobytes(), f"{case}: history rows differ for instance {i}"
            m, om = eng.meta(i), ora.meta[i]
            assert (m.n_rows, m.flags) == (om["n_rows"], om["flags"]), f"{case}: meta differs for instance {i}"
            if full:
                assert pay.tobytes() == opay.tobytes(), f"{case}: payload differs for instance {i}"
                assert m.n_payload_words == om["n_payload_words"], f"{case}: payload words differ for instance {i}"
                assert m.n_rounds == om["n_rounds"], f"{case}: rounds differ for instance {i}"
                st = eng.net_stats_raw(i)
                for f in ("all_send", "all_recv", "clients_send", "clients_recv", "servers_send", "servers_recv"):
                    assert int(getattr(st, f)) == int(ora.stats[i][f]), f"{case}: {f} differs for instance {i}"


@pytest.mark.parametrize("case", CASES)
def test_duo_halves_equal_the_oracle(lib, case):
    _run(case, True)


@pytest.mark.parametrize("case", STOPS)
def test_duo_halves_stopped_by_a_capacity(lib, case):
    _run(case, False)
