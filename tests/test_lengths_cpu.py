"""CPU: the parts of per-replicate chain lengths that need no device -- the two C ABI entries exist everywhere they must, the
argument checks and the refusals of pyvb_lds_create_lengths come before any HIP call, and lds.pad_series pads as documented."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from pyvb_amd import _capi, lds, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_lds_create_lengths", "pyvb_lds_get_lengths")


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/pyvb_hip.h"
        assert name in _capi.SIGNATURES, name + " is not bound in _capi.SIGNATURES"
        assert getattr(_capi.lib, name).argtypes == _capi.SIGNATURES[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= exported
    assert _capi.lib.pyvb_version() >= 101


def _create(N, T, D, K, noise, lengths):
    h = ctypes.c_void_p()
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = _capi.lib.pyvb_lds_create_lengths(ctypes.byref(h), 0, N, T, D, K, noise, ln.ctypes.data_as(_capi._ip))
    assert not h.value
    return rc, _capi.lib.pyvb_last_error().decode()


@pytest.mark.parametrize("lengths,bad", [([10, 1, 5], 1), ([10, 5, 11], 2), ([0, 1, 11], 0)])
def test_lengths_out_of_range_are_argument_errors(lengths, bad):
    rc, msg = _create(3, 10, 4, 5, _capi.NOISE_DIAGONAL_GAMMA, lengths)
    assert rc == _capi.E_ARG, (rc, msg)
    assert "replicate %d" % bad in msg and "HIP" not in msg, msg


@pytest.mark.parametrize("D,K,noise", [(4, 5, _capi.NOISE_WISHART), (65, 5, _capi.NOISE_DIAGONAL_GAMMA), (4, 65, _capi.NOISE_GAMMA)])
def test_unequal_lengths_are_refused_where_they_are_not_served(D, K, noise):
    rc, msg = _create(3, 10, D, K, noise, [10, 4, 10])
    assert rc == _capi.E_UNSUPPORTED, (rc, msg)
    assert ("Wishart" in msg) if noise == _capi.NOISE_WISHART else ("64" in msg), msg
    assert "HIP" not in msg, msg


def test_get_lengths_refuses_null():
    assert _capi.lib.pyvb_lds_get_lengths(None, None) == _capi.E_ARG


def test_pad_series():
    D, K = 3, 4
    Ts = [5, 12, 2, 9]
    series = [(synth.simulate_lds(T, D, K, 1, seed=40 + T)["Y"][0], synth.initial_state(T, D, K, 1, seed=T)) for T in Ts]
    Y, st0, lengths = lds.pad_series(series)
    assert lengths.dtype == np.int32 and list(lengths) == Ts
    assert Y.shape == (4, 12, K) and st0["X"].shape == (4, 12, D)
    assert st0["A_mean"].shape == (4, D, D) and st0["A_colvar"].shape == (4, D, D)
    assert st0["C_mean"].shape == (4, K, D) and st0["C_colvar"].shape == (4, D, K)
    assert st0["Q_b"].shape == (4, D) and st0["R_b"].shape == (4, K)
    for n, ((y, st), T) in enumerate(zip(series, Ts)):          # only the live rows are specified
        assert np.array_equal(Y[n, :T], y)
        assert np.array_equal(st0["X"][n, :T], st["X"][0])
        for k in ("A_mean", "A_colvar", "C_mean", "C_colvar", "Q_b", "R_b"):
            assert np.array_equal(st0[k][n], st[k][0]), k
    with pytest.raises(AssertionError):
        lds.pad_series([(np.zeros((5, K)), synth.initial_state(6, D, K, 1))])
    with pytest.raises(ValueError):
        lds.pad_series([])
