"""CPU-only: the per-replicate entries of the C ABI -- pyvb_lds_get_status, pyvb_lds_set_active, pyvb_lds_get_active
(include/pyvb_hip.h) -- are declared, exported, bound by pyvb_amd._capi, and refuse NULL before any HIP call."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pyvb_lds_get_status", "pyvb_lds_set_active", "pyvb_lds_get_active")


def test_the_three_entries_are_declared_exported_and_bound():
    from pyvb_amd import _capi
    hdr = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(pyvb_lds\* h, " % name, hdr), name
        assert hasattr(lib, name), "libpyvb_hip.so does not export %s" % name
        assert name in _capi.SIGNATURES, "pyvb_amd._capi does not bind %s" % name
    assert _capi.SIGNATURES["pyvb_lds_get_status"][1][1] is _capi._ip
    assert _capi.SIGNATURES["pyvb_lds_set_active"][1][1]._type_ is ctypes.c_ubyte
    for name, bit in (("PYVB_FAIL_STATES", _capi.FAIL_STATES), ("PYVB_FAIL_COLUMNS", _capi.FAIL_COLUMNS), ("PYVB_FAIL_NOISE", _capi.FAIL_NOISE)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == bit


def test_null_is_refused_without_a_gpu():
    from pyvb_amd import _capi
    one, byte = ctypes.c_int(0), ctypes.c_ubyte(1)
    for name, arg in (("pyvb_lds_get_status", ctypes.byref(one)), ("pyvb_lds_set_active", ctypes.byref(byte)),
                      ("pyvb_lds_get_active", ctypes.byref(byte))):
        fn = getattr(_capi.lib, name)
        rc = fn(None, ctypes.cast(arg, fn.argtypes[1]))
        assert rc == _capi.E_ARG, name
        assert b"handle is NULL" in _capi.lib.pyvb_last_error(), name


def test_the_batch_front_end_has_the_methods():
    from pyvb_amd.lds import LDSBatch
    for name in ("status", "set_active", "active"):
        assert callable(getattr(LDSBatch, name))
    assert LDSBatch.describe_status(_bits()) == "X_t, columns of A / C, Wishart Q / R"


def _bits():
    from pyvb_amd import _capi
    return _capi.FAIL_STATES | _capi.FAIL_COLUMNS | _capi.FAIL_NOISE
