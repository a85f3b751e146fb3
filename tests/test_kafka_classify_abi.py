"""The ctypes prototype of the kafka classification's batch entry (maelstrom_amd/_abi.py) beside the entry it mirrors:
msim_classify_kafka_batch takes what msim_check_kafka_batch takes; the header declares it, the library exports it, and it refuses null
arguments and a concurrency outside 1 .. 64 before it touches a device.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_classify_kafka_entry_is_declared_exported_and_prototyped(lib):
    with open(os.path.join(ROOT, "include", "maelsim.h")) as f:
        header = f.read()
    name = "msim_classify_kafka_batch"
    assert name in A.EXPORTS and re.search(r"^int %s\(" % name, header, re.M)
    assert hasattr(lib, name)
    assert lib.msim_classify_kafka_batch.argtypes == lib.msim_check_kafka_batch.argtypes and lib.msim_classify_kafka_batch.restype is C.c_int
    sig = lambda n: re.sub(r"\s+", " ", re.search(r"^int %s\(([^;]*)\);" % n, header, re.M | re.S).group(1))
    assert sig(name) == sig("msim_check_kafka_batch")
    assert callable(E.classify_kafka_batch) and callable(E.kafka_anomaly_census)


def test_classify_kafka_entry_refuses_null_and_zero_arguments(lib):
    rows = np.zeros(2, dtype=E.OP_DT); pay = np.zeros(1, dtype=np.uint32); off = np.zeros(2, dtype=np.uint64); out = np.zeros(1, dtype=E.CHECK_DT)
    good = [0, rows.ctypes.data, off.ctypes.data, pay.ctypes.data, off.ctypes.data, 1, 3, out.ctypes.data, None]
    assert lib.msim_classify_kafka_batch(0, None, None, None, None, 0, 0, None, None) == A.E_INVALID
    for i in (1, 2, 4, 7):                       # rows, row offsets, payload offsets, out
        args = list(good); args[i] = None
        assert lib.msim_classify_kafka_batch(*args) == A.E_INVALID, i
    args = list(good); args[5] = 0               # no histories
    assert lib.msim_classify_kafka_batch(*args) == A.E_INVALID
    for conc in (0, 65):                         # worker threads: 1 .. 64
        args = list(good); args[6] = conc
        assert lib.msim_classify_kafka_batch(*args) == A.E_INVALID, conc


def test_kafka_anomaly_census_counts_by_name():
    rec = np.zeros(4, dtype=E.CHECK_DT)
    rec["error_count"] = [0, 1 | 32, 64 | 128 | 256, 1]
    census = E.kafka_anomaly_census(rec)
    assert set(census) == set(A.KAFKA_ANOMALIES.values()) | {"clean"}
    assert census["clean"] == 1 and census["lost-write"] == 2 and census["int-poll-skip"] == 1 and census["duplicate"] == 1 and census["malformed"] == 0
