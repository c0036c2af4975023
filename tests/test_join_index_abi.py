"""The join-index entry points on CPU: both libraries export
smj_dev_join_pairs and smj_dev_semi_join, and the binding carries them up to
Library.dev_join_pairs / dev_semi_join / join_index.  No device call is made
(tests/test_gpu_join_index.py runs them)."""
import ctypes
import os

import pytest

NAMES = ("smj_dev_join_pairs", "smj_dev_semi_join")


@pytest.fixture(scope="module")
def smj_mod():
    import smj
    for w in (8, 16):
        if not os.path.exists(smj.lib_path(w)):
            smj.build()
            break
    return smj


@pytest.mark.parametrize("width", [8, 16])
def test_libraries_export_join_index(smj_mod, width):
    lib = ctypes.CDLL(smj_mod.lib_path(width))
    missing = [s for s in NAMES if not hasattr(lib, s)]
    assert not missing, missing


def test_names_are_listed(smj_mod):
    assert set(NAMES) <= set(smj_mod.DEVICE_SYMBOLS)


@pytest.mark.parametrize("width", [8, 16])
def test_binding_has_join_index(smj_mod, width):
    L = smj_mod.Library(width)
    for name in NAMES:
        f = getattr(L.lib, name)
        assert f.restype is ctypes.c_uint64, name
    # (ws, R, nR, S, nS, r_out, s_out, key_out, cap, stream)
    assert len(L.lib.smj_dev_join_pairs.argtypes) == 10
    # (ws, R, nR, S, nS, out, cap, anti, stream)
    assert len(L.lib.smj_dev_semi_join.argtypes) == 9
    assert L.lib.smj_dev_semi_join.argtypes[7] is ctypes.c_int
    for method in ("dev_join_pairs", "dev_semi_join", "join_index"):
        assert callable(getattr(L, method)), method
