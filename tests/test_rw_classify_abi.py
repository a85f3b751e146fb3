"""The ctypes prototypes of the rw-register classification's entries (maelstrom_amd/_abi.py) beside those of the entries they extend:
msim_classify_rw_batch takes what msim_check_rw_batch takes, msim_set_check_classify what msim_set_dev_flags takes; the header
declares both and the library exports them.  Needs no device."""
import ctypes as C
import os
import re

from maelstrom_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_classify_entries_are_declared_exported_and_prototyped(lib):
    with open(os.path.join(ROOT, "include", "maelsim.h")) as f:
        header = f.read()
    for name in ("msim_classify_rw_batch", "msim_set_check_classify"):
        assert name in A.EXPORTS and re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(lib, name), name
    assert lib.msim_classify_rw_batch.argtypes == lib.msim_check_rw_batch.argtypes and lib.msim_classify_rw_batch.restype is C.c_int
    assert lib.msim_set_check_classify.argtypes == lib.msim_set_dev_flags.argtypes and lib.msim_set_check_classify.restype is C.c_int
    sig = lambda name: re.sub(r"\s+", " ", re.search(r"^int %s\(([^;]*)\);" % name, header, re.M | re.S).group(1))
    assert sig("msim_classify_rw_batch") == sig("msim_check_rw_batch")
    # no device is touched by either refusal
    assert lib.msim_set_check_classify(None, 1) == A.E_INVALID
    assert lib.msim_classify_rw_batch(0, None, None, None, None, 0, 0, None, None) == A.E_INVALID
