"""Long reads cut into segments (sshash_set_read_segments / sshash_get_read_segments) at the C ABI and in the binding, as far as a machine
without a GPU can tell: the symbols are declared, exported, bound and present in the facade; a new dictionary does not segment
(SSHASH_SEGMENTS_OFF, the device calls switched off) and 0 sets the default S; what is set is read back; 0 and SSHASH_SEGMENTS_OFF are accepted; a NULL dictionary, 2^30 + 1 and other
nonsense are SSHASH_ERR_ARGUMENT with a message, and leave the setting alone; the call needs no device; no segmented launch has been
counted on a dictionary that never ran one."""
from __future__ import annotations

import ctypes as C
import os
import re

import pytest

import sshash_amd
from sshash_amd import _binding as B
from conftest import ROOT

SYMBOLS = ("sshash_set_read_segments", "sshash_get_read_segments")
ERR_ARGUMENT = 1
OFF = 0xFFFFFFFFFFFFFFFF
DEFAULT_S = 256  # (include/sshash_amd.h says so, and RESULTS.md why)


def _get(d):
    kmers, device_calls, launches = C.c_uint64(7), C.c_int(7), C.c_uint64(7)
    assert B._load().sshash_get_read_segments(d._h, C.byref(kmers), C.byref(device_calls), C.byref(launches)) == 0
    return kmers.value, device_calls.value, launches.value


def test_symbols_are_declared_exported_bound_and_in_the_facade():
    header = open(os.path.join(ROOT, "include", "sshash_amd.h")).read()
    facade = open(os.path.join(ROOT, "include", "sshash_amd.hpp")).read()
    lib = C.CDLL(sshash_amd.library_path())
    bound = B._load()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in B.C_ABI_SYMBOLS
        assert getattr(bound, name).argtypes is not None and getattr(bound, name).restype is C.c_int
        assert name + "(" in facade, name
    assert re.search(r"#define\s+SSHASH_SEGMENTS_OFF\s+UINT64_MAX", header)
    for method in ("set_read_segments", "read_segments"):
        assert callable(getattr(sshash_amd.Dictionary, method)), method
        assert re.search(r"\b" + method + r"\s*\(", facade), method
    assert sshash_amd.SEGMENTS_OFF == OFF
    assert str(DEFAULT_S) in header[header.index("LONG READS"):header.index("sshash_set_read_segments(")]


def test_defaults_and_read_back(case_skew_regular, case_k63_canonical):
    """no device anywhere near: the setting is the dictionary's own"""
    lib = B._load()
    d = case_skew_regular.dict
    try:
        assert _get(d) == (OFF, 0, 0), "segmenting is opt-in"
        assert d.read_segments() == {"kmers": OFF, "device_calls": False, "segmented_launches": 0}
        for kmers, device_calls in ((7, 1), (1, 0), (1 << 30, 1), (OFF, 0), (OFF, 1), (4096, 0)):
            assert lib.sshash_set_read_segments(d._h, kmers, device_calls) == 0
            assert _get(d) == (kmers, device_calls, 0)
        assert lib.sshash_set_read_segments(d._h, 64, 5) == 0  # (any non-zero int switches the device calls on)
        assert _get(d) == (64, 1, 0)
        assert lib.sshash_set_read_segments(d._h, 0, 0) == 0   # 0: the default S
        assert _get(d) == (DEFAULT_S, 0, 0)
        # each output pointer may be NULL
        kmers = C.c_uint64(0)
        assert lib.sshash_get_read_segments(d._h, None, None, None) == 0
        assert lib.sshash_get_read_segments(d._h, C.byref(kmers), None, None) == 0 and kmers.value == DEFAULT_S
        # the Python method
        d.set_read_segments(7, device_calls=True)
        assert d.read_segments() == {"kmers": 7, "device_calls": True, "segmented_launches": 0}
        d.set_read_segments(sshash_amd.SEGMENTS_OFF)
        assert d.read_segments()["kmers"] == OFF and not d.read_segments()["device_calls"]
        d.set_read_segments()
        assert d.read_segments() == {"kmers": DEFAULT_S, "device_calls": False, "segmented_launches": 0}
        # a setting belongs to its dictionary
        d.set_read_segments(2, device_calls=True)
        assert _get(case_k63_canonical.dict) == (OFF, 0, 0)
    finally:
        d.set_read_segments(sshash_amd.SEGMENTS_OFF)  # (the fixture is shared)


@pytest.mark.parametrize("bad", [(1 << 30) + 1, 1 << 31, 1 << 40, OFF - 1, 1 << 63])
def test_nonsense_is_an_argument_error(case_skew_regular, bad):
    lib = B._load()
    d = case_skew_regular.dict
    lib.sshash_last_error.restype = C.c_char_p
    try:
        assert lib.sshash_set_read_segments(d._h, 9, 1) == 0
        assert lib.sshash_set_read_segments(d._h, bad, 0) == ERR_ARGUMENT
        message = lib.sshash_last_error()
        assert message and b"kmers_per_segment" in message
        assert _get(d) == (9, 1, 0), "a refused call changed the setting"
        with pytest.raises(sshash_amd.SSHashError) as e:
            d.set_read_segments(bad)
        assert e.value.status == ERR_ARGUMENT
    finally:
        d.set_read_segments(sshash_amd.SEGMENTS_OFF)


def test_a_null_dictionary_is_an_argument_error():
    lib = B._load()
    lib.sshash_last_error.restype = C.c_char_p
    assert lib.sshash_set_read_segments(None, 0, 0) == ERR_ARGUMENT
    assert lib.sshash_last_error()
    assert lib.sshash_set_read_segments(None, OFF, 1) == ERR_ARGUMENT
    kmers = C.c_uint64(5)
    assert lib.sshash_get_read_segments(None, C.byref(kmers), None, None) == ERR_ARGUMENT and kmers.value == 5
    assert lib.sshash_last_error()


def test_segment_arithmetic_under_the_sanitizers():
    """the host code that sizes a segmented launch (csrc/segments.hpp: the bound, the scratch layout) as a stand-alone program of its
    own, built with -fsanitize=address,undefined and run on the CPU: `make sanitize`"""
    import subprocess

    p = subprocess.run(["make", "-C", os.path.join(ROOT, "sshash_amd", "csrc"), "sanitize"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "EVERYTHING OK!" in p.stdout
