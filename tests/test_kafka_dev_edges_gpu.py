"""kafka: the edge shapes of the device checker (csrc/kafka_check_dev.hip: kafka_body<CLASSIFY>, the one body of kafka_check_kernel and
kafka_classify_kernel) on BOTH routes — E.check_kafka_batch (the clean pass, then the host) and E.classify_kafka_batch (the clean pass, the classification, then the
host) — against the host checker (msim_check_kafka_rows; the `_host` of tests/test_kafka_check_gpu.py), field by field over that
module's FIELDS, with the number of histories handed to the host asserted.

tests/test_kafka_classify_gpu.py sends its EDGES through the classification only; here they go through the clean route, next to clean
twins of them (where the clean pass has to PROVE the history clean: a block header read from HBM behind the 128 staged payload words,
four wavefronts' workers, the bit words' edges, the largest table) and rows that do not decode, which E.encode_kafka_history refuses to
build: they are made by editing the arrays it returns.  Every case is a batch of one history of a few rows."""
import pytest

from maelstrom_amd import engine as E

from test_kafka import _h, _poll, _send
from test_kafka_check_gpu import FIELDS, _same
from test_kafka_classify_gpu import EDGE_HS, EDGES, _host_of, _names

pytestmark = pytest.mark.gpu

ROUTES = {"check": E.check_kafka_batch, "classify": E.classify_kafka_batch}


def _routed(route, hs, what, concurrency, n_host):
    """one call of the route's batch entry: every record the host's, exactly `n_host` histories handed over"""
    host = _host_of(hs)
    dev, handed = ROUTES[route](list(hs), concurrency)
    for i, h in enumerate(host):
        assert _same(dev[i], h), (what, route, i, {f: int(dev[i][f]) for f in FIELDS}, h, _names(h["error_count"]))
    assert handed == n_host, (what, route, handed, n_host)
    return host


@pytest.mark.parametrize("edge", list(EDGES))
def test_edges_through_the_clean_route(lib, edge):
    """the clean pass decides nothing it cannot prove: whatever the host finds a bit in, and whatever the classification hands over,
    is the host's here"""
    _, conc, _, handed = EDGES[edge]
    hs = EDGE_HS[edge]
    unclean = _host_of(hs)[0]["error_count"] != 0 or handed != 0
    _routed("check", hs, edge, conc, 1 if unclean else 0)


def _long_clean_poll():
    """300 consecutive pairs of one key in one poll — blocks of 255 and 45 messages, the second block's header at payload word 129,
    behind the 128 words a wavefront stages — and the same process's next poll, which continues at offset 300"""
    return _h(*_poll(1, {"2": [[o, o + 1] for o in range(300)]}), *_poll(1, {"2": [[300, 301], [301, 302]]}))


def _four_workers():
    """concurrency 64: processes 1, 9 and 17 are workers of one wavefront, 63 of another; each sends to and polls a key of its own,
    strictly upwards, the rows interleaved"""
    ops = []
    for step in range(3):
        for p, k in ((1, "1"), (9, "2"), (17, "3"), (63, "4")):
            ops += _send(p, k, 10 * step + 1, 2 * step) + _send(p, k, 10 * step + 2, 2 * step + 1)
            ops += _poll(p, {k: [[2 * step, 10 * step + 1], [2 * step + 1, 10 * step + 2]]})
    return _h(*ops)


def _clean_word_boundaries():
    """offsets 31 / 32 / 63 / 64 sent and polled in order (messages up to 65: a table of 96 entries in a batch of one)"""
    sends = sum((_send(0, "1", o + 1, o) for o in (31, 32, 63, 64)), [])
    return _h(*sends, *_poll(1, {"1": [[31, 32], [32, 33]]}), *_poll(1, {"1": [[63, 64], [64, 65]]}))


CLEAN = {
    # name: (ops, concurrency, histories handed over by {route})
    "a block header behind payload word 128": (_long_clean_poll(), 3, {"check": 0, "classify": 0}),
    "concurrency 64, workers 1 / 9 / 17 / 63": (_four_workers(), 64, {"check": 0, "classify": 0}),
    "offsets 31 / 32 / 63 / 64": (_clean_word_boundaries(), 3, {"check": 0, "classify": 0}),
    # tables of 2048 entries per key: the clean pass's largest (more than 64 KB of LDS).  It proves the history clean on either route,
    # so the classification, whose tables end at 1152, is never asked
    "offset 2046, the layout's last": (_h(*_send(0, "1", 5, 2046), *_poll(1, {"1": [[2046, 5]]})), 3, {"check": 0, "classify": 0}),
}
CLEAN_HS = {name: (E.encode_kafka_history(ops),) for name, (ops, _, _) in CLEAN.items()}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(CLEAN))
def test_clean_twins(lib, name, route):
    _, conc, handed = CLEAN[name]
    host = _routed(route, CLEAN_HS[name], name, conc, handed[route])
    assert host[0]["valid"] == 1 and host[0]["error_count"] == 0, (name, host[0])


def _edited(ops, edit):
    rows, pay = E.encode_kafka_history(ops)
    rows, pay = rows.copy(), pay.copy()
    return (edit(rows, pay),)


def _shorter_len(rows, pay):   # the :ok poll's len one word short of what its block's count asks for
    assert int(rows["time_len"][-1]) >> 48 == 3
    rows["time_len"][-1] = (int(rows["time_len"][-1]) & ((1 << 48) - 1)) | (2 << 48)
    return rows, pay


def _with_send_value(value):
    def edit(rows, pay):
        rows["value"][1] = value
        return rows, pay
    return edit


_POLL3 = _h(*_send(0, "1", 1, 0), *_poll(1, {"1": [[0, 1], [1, 2], [2, 3]]}))
UNDECODABLE = {
    "a poll block whose count runs past the row's len": _edited(_POLL3, _shorter_len),
    "value + len beyond the payload words given": _edited(_POLL3, lambda rows, pay: (rows, pay[:-1])),
    "an :ok send whose offset field is 0x7FF": _edited(_POLL3, _with_send_value(1 | (1 << 6) | (0x7FF << 17))),
    "an :ok send of key 8": _edited(_POLL3, _with_send_value(8 | (1 << 6) | (0 << 17))),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(UNDECODABLE))
def test_rows_that_do_not_decode_are_the_hosts(lib, name, route):
    host = _routed(route, UNDECODABLE[name], name, 3, 1)
    assert "malformed" in _names(host[0]["error_count"]), (name, host[0])
