"""The read-only export of a replica's super-k-mer table (sshash_device_table_export, Dictionary.device_table) at the C ABI and in the
binding, as far as a machine without a GPU can tell: the symbol is declared beside sshash_device_table_histogram, exported and bound;
a NULL dictionary or a NULL info is SSHASH_ERR_ARGUMENT with a message and leaves the caller's words alone; a dictionary that is on
no device answers as the other two statistics calls do -- SSHASH_ERR_NO_DEVICE --, with or without a buffer. What needs a replica --
the copy, a capacity that is too small, a replica without a table -- is in tests/gpu_table_worker.py."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import ROOT

SYMBOL = "sshash_device_table_export"
ERR_ARGUMENT, ERR_NO_DEVICE = 1, 5
UNTOUCHED = 0x5A5A5A5A5A5A5A5A


def _info():
    return (C.c_uint64 * 8)(*([UNTOUCHED] * 8))


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    assert re.search(r"sshash_status\s+" + SYMBOL + r"\s*\(const sshash_dict\*\s*d,\s*int device,\s*uint64_t info\[8\],\s*void\*\s*out,\s*uint64_t capacity_bytes\);", header)
    assert header.index("sshash_device_table_histogram(") < header.index(SYMBOL + "(") < header.index("sshash_lookup_packed_device(")
    assert hasattr(C.CDLL(sshash_amd.library_path()), SYMBOL) and SYMBOL in B.C_ABI_SYMBOLS
    fn = getattr(B._load(), SYMBOL)
    assert fn.restype is C.c_int and len(fn.argtypes) == 5
    assert callable(sshash_amd.Dictionary.device_table)
    assert SYMBOL in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define\s+SSHASH_ERR_NO_DEVICE\s+5\b|SSHASH_ERR_NO_DEVICE\s*=\s*5\b", header)


def test_null_arguments_are_argument_errors(case_skew_regular):
    lib = B._load()
    lib.sshash_last_error.restype = C.c_char_p
    info = _info()
    assert lib.sshash_device_table_export(None, 0, C.byref(info), None, 0) == ERR_ARGUMENT
    assert lib.sshash_last_error() and list(info) == [UNTOUCHED] * 8
    assert lib.sshash_device_table_export(case_skew_regular.dict._h, 0, None, None, 0) == ERR_ARGUMENT
    assert lib.sshash_last_error()
    words = np.full(16, 7, dtype=np.uint32)
    assert lib.sshash_device_table_export(None, 0, C.byref(info), words.ctypes.data_as(C.c_void_p), words.nbytes) == ERR_ARGUMENT
    assert (words == 7).all() and list(info) == [UNTOUCHED] * 8


@pytest.mark.parametrize("device", [0, 3, -1])
def test_a_dictionary_on_no_device_answers_as_the_histogram_does(case_skew_regular, device):
    lib = B._load()
    lib.sshash_last_error.restype = C.c_char_p
    d = case_skew_regular.dict
    histogram = (C.c_uint64 * 32)()
    assert lib.sshash_device_table_histogram(d._h, device, C.byref(histogram)) == ERR_NO_DEVICE
    info, words = _info(), np.full(16, 7, dtype=np.uint32)
    assert lib.sshash_device_table_export(d._h, device, C.byref(info), None, 0) == ERR_NO_DEVICE
    assert b"not resident" in lib.sshash_last_error()
    assert lib.sshash_device_table_export(d._h, device, C.byref(info), words.ctypes.data_as(C.c_void_p), words.nbytes) == ERR_NO_DEVICE
    assert (words == 7).all()
    with pytest.raises(sshash_amd.SSHashError) as e:
        d.device_table(device)
    assert e.value.status == ERR_NO_DEVICE
