"""The band-join entry points on CPU: both libraries export smj_dev_band_join
and smj_dev_band_join_count, and the binding carries them up to
Library.dev_band_join / dev_band_join_count / band_join.  No device call is
made (tests/test_gpu_band_join.py runs them).  The expected-value
construction of the GPU tests (band_ref.numpy_band) is checked here against
the plain definition."""
import ctypes
import os

import numpy as np
import pytest

from band_ref import I64_MAX, I64_MIN, double_loop, numpy_band

NAMES = ("smj_dev_band_join", "smj_dev_band_join_count")


@pytest.fixture(scope="module")
def smj_mod():
    import smj
    for w in (8, 16):
        if not os.path.exists(smj.lib_path(w)):
            smj.build()
            break
    return smj


@pytest.mark.parametrize("width", [8, 16])
def test_libraries_export_band_join(smj_mod, width):
    lib = ctypes.CDLL(smj_mod.lib_path(width))
    missing = [s for s in NAMES if not hasattr(lib, s)]
    assert not missing, missing


def test_names_are_listed(smj_mod):
    assert set(NAMES) <= set(smj_mod.DEVICE_SYMBOLS)


@pytest.mark.parametrize("width", [8, 16])
def test_binding_has_band_join(smj_mod, width):
    L = smj_mod.Library(width)
    # (ws, R, nR, S, nS, lo, hi, r_out, s_out, r_key_out, s_key_out, cap, stream)
    f = L.lib.smj_dev_band_join
    assert f.restype is ctypes.c_uint64
    assert len(f.argtypes) == 13
    assert f.argtypes[5] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int64
    # (ws, R, nR, S, nS, lo, hi, count, stream)
    g = L.lib.smj_dev_band_join_count
    assert g.restype is None
    assert len(g.argtypes) == 9
    for method in ("dev_band_join", "dev_band_join_count", "band_join"):
        assert callable(getattr(L, method)), method


BANDS = [(0, 0), (-3, 3), (1, 5), (-7, -2), (2, 1), (I64_MIN, I64_MAX),
         (I64_MIN, 2), (-2, I64_MAX)]
# key domains: around zero, and within 30 of either end of int64
DOMAINS = {"mid": (-15, 15), "top": (I64_MAX - 30, I64_MAX), "bottom": (I64_MIN, I64_MIN + 30)}


@pytest.mark.parametrize("domain", list(DOMAINS))
@pytest.mark.parametrize("band", BANDS, ids=[f"band{i}" for i in range(len(BANDS))])
def test_numpy_construction_against_double_loop(domain, band):
    a, b = DOMAINS[domain]
    rng = np.random.default_rng(7)
    Rk = np.sort(rng.integers(a, b, 40, dtype=np.int64, endpoint=True))
    Sk = np.sort(rng.integers(a, b, 50, dtype=np.int64, endpoint=True))
    lo, hi = band
    r_idx, s_idx = numpy_band(Rk, Sk, lo, hi)
    exp = double_loop(Rk, Sk, lo, hi)
    assert exp == list(zip(r_idx.tolist(), s_idx.tolist()))
    if band == (2, 1):
        assert exp == []
    if band == (I64_MIN, I64_MAX):
        assert len(exp) == 40 * 50
