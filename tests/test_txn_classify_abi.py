"""The ctypes prototype of the list-append classification's batch entry (maelstrom_amd/_abi.py) beside the rw-register one it mirrors:
msim_classify_txn_batch takes what msim_classify_rw_batch takes; the header declares it, the library exports it, and it refuses null
arguments before it touches a device.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_classify_txn_entry_is_declared_exported_and_prototyped(lib):
    with open(os.path.join(ROOT, "include", "maelsim.h")) as f:
        header = f.read()
    name = "msim_classify_txn_batch"
    assert name in A.EXPORTS and re.search(r"^int %s\(" % name, header, re.M)
    assert hasattr(lib, name)
    assert lib.msim_classify_txn_batch.argtypes == lib.msim_classify_rw_batch.argtypes and lib.msim_classify_txn_batch.restype is C.c_int
    sig = lambda n: re.sub(r"\s+", " ", re.search(r"^int %s\(([^;]*)\);" % n, header, re.M | re.S).group(1))
    assert sig(name) == sig("msim_classify_rw_batch")
    assert callable(E.classify_txn_batch)


def test_classify_txn_entry_refuses_null_and_zero_arguments(lib):
    rows = np.zeros(2, dtype=E.OP_DT); pay = np.zeros(1, dtype=np.uint32); off = np.zeros(2, dtype=np.uint64); out = np.zeros(1, dtype=E.CHECK_DT)
    good = [0, rows.ctypes.data, off.ctypes.data, pay.ctypes.data, off.ctypes.data, 1, A.CM_STRICT_SERIALIZABLE, out.ctypes.data, None]
    assert lib.msim_classify_txn_batch(0, None, None, None, None, 0, 0, None, None) == A.E_INVALID
    for i in (1, 2, 4, 7):                       # rows, row offsets, payload offsets, out
        args = list(good); args[i] = None
        assert lib.msim_classify_txn_batch(*args) == A.E_INVALID, i
    args = list(good); args[5] = 0               # no histories
    assert lib.msim_classify_txn_batch(*args) == A.E_INVALID
    args = list(good); args[6] = A.CM_READ_UNCOMMITTED + 1   # no such consistency model
    assert lib.msim_classify_txn_batch(*args) == A.E_INVALID
