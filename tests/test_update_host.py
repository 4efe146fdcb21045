"""In-place value updates (vbc.h vbc_update_values, VBC_CREATE_UPDATABLE): everything that needs no GPU --
the ABI, the error paths that are decided before a device is touched, and update_from_csc's pattern check."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from sparsematrixvbcs_amd import _lib as L

HEADER = L.PKG_DIR.parent / "include" / "vbc.h"


def test_abi_symbol_header_list_and_exports_agree():
    text = HEADER.read_text()
    assert re.search(r"VBC_API\s+int\s+vbc_update_values\s*\(", text)
    assert re.search(r"#define\s+VBC_CREATE_UPDATABLE\s+0x20u", text)
    assert "vbc_update_values" in L.ABI_SYMBOLS
    assert L.VBC_CREATE_UPDATABLE == 0x20
    exported = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], check=True, capture_output=True,
                              text=True).stdout
    assert re.search(r"\bT vbc_update_values$", exported, re.M)
    assert L.lib().vbc_version() >= 30300
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", text).group(1)) == L.lib().vbc_version()


def test_null_handle_is_an_argument_error():
    v = np.ones(4)
    st = L.lib().vbc_update_values(None, v.ctypes.data, 4, L.VBC_F64, L.VBC_MEM_HOST, None)
    assert st == L.VBC_INVALID_ARG
    assert "NULL handle" in L.last_error()
    with pytest.raises(L.ArgumentError):
        L.check(st)


def moved_entry(A):
    """A with one stored entry moved to a position that was empty (same nnz, another pattern)."""
    T = A.tocoo()
    stored = np.zeros(A.shape, bool)
    stored[T.row, T.col] = True
    fi, fj = (int(t) for t in np.argwhere(~stored)[0])
    row, col = T.row.copy(), T.col.copy()
    row[0], col[0] = fi, fj
    B = sp.csc_matrix((T.data, (row, col)), shape=A.shape)
    B.sort_indices()
    assert B.nnz == A.nnz
    return B


@pytest.mark.parametrize("kind", ["1d", "2d"])
def test_update_from_csc_checks_the_pattern(golden, kind):
    A = golden["HB__west0132"]["A"]
    rng = np.random.default_rng(5)
    A2 = A.copy()
    A2.data = rng.uniform(-1, 1, A.nnz)

    def make(M, like=None):
        if kind == "1d":
            return V.SparseMatrix1DVBC[4](M, like.Phi if like is not None else V.StrictChunker(4))
        if like is not None:
            return V.SparseMatrixVBC[4, 4](M, like.Pi, like.Phi)
        return V.SparseMatrixVBC[4, 4](M, V.AlternatingPacker(V.StrictChunker(4), V.StrictChunker(4)))

    B = make(A)
    with pytest.raises(L.ArgumentError):  # not updatable: no silent re-create
        B.update_values(B.val.copy())
    with pytest.raises(L.ArgumentError):
        B.update_from_csc(A2)
    B.updatable = True
    old = B.val.copy()
    with pytest.raises(L.ArgumentError, match="sparsity pattern changed"):
        B.update_from_csc(moved_entry(A))
    assert np.array_equal(B.val, old)
    assert B.update_from_csc(A2) is B
    F = make(A2, like=B)
    assert np.array_equal(B.val, F.val) and B.val.dtype == F.val.dtype
    assert not np.array_equal(B.val, old)
    with pytest.raises(L.DimensionMismatch):
        B.update_values(np.zeros(int(B.ofs[-1]) - 2))
    assert np.array_equal(B.val, F.val)


def test_csc_update_values_replaces_nzval(golden):
    A = golden["HB__west0132"]["A"]
    Cm = V.SparseMatrixCSC(A)
    with pytest.raises(L.ArgumentError):
        Cm.update_values(Cm.nzval.copy())
    Cm.updatable = True
    new = np.arange(A.nnz, dtype=np.float64)
    Cm.update_values(new)
    assert np.array_equal(Cm.nzval, new) and Cm.nzval is Cm.val
    with pytest.raises(L.DimensionMismatch):
        Cm.update_values(new[:-1])
    Ci = V.SparseMatrixCSC(sp.csc_matrix(A != 0))
    Ci.updatable = True
    with pytest.raises(L.UnsupportedDtype):
        Ci.update_values(new)
