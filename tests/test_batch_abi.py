"""CPU checks of elp_solve_batch's boundary: the symbol is exported and its
argument errors come back before any GPU call (no GPU here)."""
import ctypes


def _lib():
    import torch
    if torch.cuda.is_available():  # (a GPU box: torch starts the HIP runtime first, as tests/test_abi.py)
        torch.cuda.init()
    from easylp_amd._lib import load
    return load()


def test_library_exports_solve_batch():
    from easylp_amd._lib import EXPORTS
    assert "elp_solve_batch" in EXPORTS
    assert hasattr(_lib(), "elp_solve_batch")


def test_negative_count():
    lib = _lib()
    st = (ctypes.c_int32 * 1)(-5)
    nb = ctypes.c_int64(-7)
    assert lib.elp_solve_batch(None, -1, st, ctypes.byref(nb)) == -1
    assert b"elp_solve_batch" in lib.elp_last_error() and b"count" in lib.elp_last_error()
    assert st[0] == -5


def test_null_handles():
    lib = _lib()
    st = (ctypes.c_int32 * 1)(-5)
    assert lib.elp_solve_batch(None, 1, st, None) == -1
    assert b"NULL" in lib.elp_last_error()
    hs = (ctypes.c_void_p * 1)(None)
    assert lib.elp_solve_batch(hs, 1, None, None) == -1
    assert lib.elp_solve_batch(hs, 1, st, None) == -1  # (a NULL member)
    assert b"member 0" in lib.elp_last_error()
    assert st[0] == -5


def test_empty_batch():
    lib = _lib()
    nb = ctypes.c_int64(-7)
    assert lib.elp_solve_batch(None, 0, None, ctypes.byref(nb)) == 0
    assert nb.value == 0
    assert lib.elp_solve_batch(None, 0, None, None) == 0
