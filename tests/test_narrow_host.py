"""Narrow value storage (vbc.h VBC_CREATE_NARROW_VALUES), the parts that need no GPU: the refusals of the C ABI
(decided before any device work), the Python rules of `B.narrow`, and the header."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from sparsematrixvbcs_amd import _lib as L

HEADER = L.PKG_DIR.parent / "include" / "vbc.h"
NARROW = L.VBC_CREATE_NARROW_VALUES


def mat1d(dtype=np.float32):
    B = V.synthetic.vbr_1dvbc(60, 12, 90, np.arange(12) % 4 + 1, W=4, seed=3)
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, B.val.astype(dtype))


def mat2d(dtype=np.float32):
    A = sp.random(40, 30, density=0.1, random_state=2, format="csc", dtype=np.float64).astype(dtype)
    return V.SparseMatrixVBC[4, 4](A, V.AlternatingPacker(V.StrictChunker(4), V.StrictChunker(4)))


def create_1d_ex(B, val_dt, compute_dt, flags):
    t = L.vbc_types(val_dt, 64, compute_dt, 0)
    h = C.c_void_p()
    st = L.lib().vbc1d_create_ex(C.byref(h), B.m, B.n, B.W, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                 B.idx.ctypes.data, B.ofs.ctypes.data, B.val.ctypes.data, len(B.val), C.byref(t), 0, flags)
    return st, h


def create_2d_ex(B, val_dt, compute_dt, flags):
    t = L.vbc_types(val_dt, 64, compute_dt, 0)
    h = C.c_void_p()
    st = L.lib().vbc2d_create_ex(C.byref(h), B.m, B.n, B.U, B.W, len(B.Pi), B.Pi.spl.ctypes.data, len(B.Phi),
                                 B.Phi.spl.ctypes.data, B.pos.ctypes.data, B.idx.ctypes.data, B.ofs.ctypes.data,
                                 B.val.ctypes.data, len(B.val), C.byref(t), 0, flags)
    return st, h


def create_csc_ex(Cm, val_dt, compute_dt, flags):
    t = L.vbc_types(val_dt, 64, compute_dt, 0)
    h = C.c_void_p()
    st = L.lib().vbc_csc_create_ex(C.byref(h), Cm.m, Cm.n, Cm.colptr.ctypes.data, Cm.rowval.ctypes.data,
                                   Cm.nzval.ctypes.data, C.byref(t), 0, flags)
    return st, h


def refused(st, h):
    assert st == L.VBC_INVALID_ARG
    assert not h.value  # no handle
    msg = L.last_error()
    assert msg and "VBC_CREATE_NARROW_VALUES" in msg
    return True


@pytest.mark.parametrize("val_dt,compute_dt,np_dt", [(L.VBC_F64, L.VBC_F64, np.float64), (L.VBC_F32, L.VBC_F32, np.float32),
                                                     (L.VBC_F64, L.VBC_F32, np.float64), (L.VBC_I32, L.VBC_F64, np.int32),
                                                     (L.VBC_BOOL, L.VBC_F64, np.bool_)])
def test_refused_for_any_other_eltype_pair(val_dt, compute_dt, np_dt):
    f = L.VBC_CREATE_TRANSPOSED | NARROW
    assert refused(*create_1d_ex(mat1d(np_dt), val_dt, compute_dt, f))
    if np_dt in (np.float64, np.float32):
        assert refused(*create_2d_ex(mat2d(np_dt), val_dt, compute_dt, f))
        A = sp.random(40, 30, density=0.1, random_state=4, format="csc", dtype=np.float64).astype(np_dt)
        assert refused(*create_csc_ex(V.SparseMatrixCSC(A), val_dt, compute_dt, f))


def test_refused_on_the_creates_without_types():
    f = L.VBC_CREATE_TRANSPOSED | NARROW
    for dt, np_dt in ((L.VBC_F64, np.float64), (L.VBC_F32, np.float32)):
        B = mat1d(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc1d_create(C.byref(h), B.m, B.n, B.W, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                  B.idx.ctypes.data, B.ofs.ctypes.data, B.val.ctypes.data, len(B.val), dt, 0, f)
        assert refused(st, h)
        B2 = mat2d(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc2d_create(C.byref(h), B2.m, B2.n, B2.U, B2.W, len(B2.Pi), B2.Pi.spl.ctypes.data, len(B2.Phi),
                                  B2.Phi.spl.ctypes.data, B2.pos.ctypes.data, B2.idx.ctypes.data, B2.ofs.ctypes.data,
                                  B2.val.ctypes.data, len(B2.val), dt, 0, f)
        assert refused(st, h)
        A = sp.random(40, 30, density=0.1, random_state=4, format="csc", dtype=np.float64).astype(np_dt)
        Cm = V.SparseMatrixCSC(A)
        h = C.c_void_p()
        st = L.lib().vbc_csc_create(C.byref(h), Cm.m, Cm.n, Cm.colptr.ctypes.data, Cm.rowval.ctypes.data,
                                    Cm.nzval.ctypes.data, dt, 0, f)
        assert refused(st, h)


def test_refused_together_with_updatable():
    f = L.VBC_CREATE_TRANSPOSED | NARROW | L.VBC_CREATE_UPDATABLE
    assert refused(*create_1d_ex(mat1d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_2d_ex(mat2d(), L.VBC_F32, L.VBC_F64, f))
    A = sp.random(40, 30, density=0.1, random_state=4, format="csc", dtype=np.float64).astype(np.float32)
    assert refused(*create_csc_ex(V.SparseMatrixCSC(A), L.VBC_F32, L.VBC_F64, f))


@pytest.mark.parametrize("upd", [0, L.VBC_CREATE_UPDATABLE_SHARDS])
def test_refused_on_the_sharded_creates(upd):
    f = L.VBC_CREATE_TRANSPOSED | NARROW | upd
    t = L.vbc_types(L.VBC_F32, 64, L.VBC_F64, 0)
    devs = (C.c_int * 2)(0, 0)
    B = mat1d()
    h = C.c_void_p()
    st = L.lib().vbc1d_create_sharded(C.byref(h), B.m, B.n, B.W, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                      B.idx.ctypes.data, B.ofs.ctypes.data, B.val.ctypes.data, len(B.val), C.byref(t),
                                      2, devs, L.VBC_SPLIT_STRIPES, f)
    assert refused(st, h)
    B2 = mat2d()
    h = C.c_void_p()
    st = L.lib().vbc2d_create_sharded(C.byref(h), B2.m, B2.n, B2.U, B2.W, len(B2.Pi), B2.Pi.spl.ctypes.data, len(B2.Phi),
                                      B2.Phi.spl.ctypes.data, B2.pos.ctypes.data, B2.idx.ctypes.data, B2.ofs.ctypes.data,
                                      B2.val.ctypes.data, len(B2.val), C.byref(t), 2, devs, L.VBC_SPLIT_STRIPES, f)
    assert refused(st, h)


class Recorder:
    """Stands in for the device create: records the flags handle() passes."""

    def __init__(self, B):
        self.flags = []
        B._create = self.create

    def create(self, out, device, flags, compute):
        self.flags.append((flags, compute))
        return L.VBC_OK


def test_python_narrow_is_passed_for_f32_values_in_f64_only():
    for dtype, compute, want in ((np.float32, L.VBC_F64, True), (np.float32, L.VBC_F32, False),
                                 (np.float32, None, False), (np.float64, L.VBC_F64, False),
                                 (np.float64, L.VBC_F32, False)):
        for B in (mat1d(dtype), mat2d(dtype)):
            B.narrow = True
            rec = Recorder(B)
            B.handle(0, True, compute=compute)
            B.handle(0, False, compute=compute)
            assert len(rec.flags) == 2
            for flags, _ in rec.flags:
                assert bool(flags & NARROW) == want, (dtype, compute)
            B._handles.h.clear()  # nothing was created
    Bi = V.SparseMatrix1DVBC[4](sp.csc_matrix(np.eye(8, dtype=np.int32)), V.StrictChunker(4))
    Bi.narrow = True
    rec = Recorder(Bi)
    Bi.handle(0, True)
    Bi.handle(0, True, compute=L.VBC_F64)
    assert all(not (flags & NARROW) for flags, _ in rec.flags)
    Bi._handles.h.clear()
    B = mat1d()
    rec = Recorder(B)  # without the attribute: never
    B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags[0][0] & NARROW
    B._handles.h.clear()
    B = mat1d()
    B.narrow = True
    rec = Recorder(B)  # the matrix-core panel layouts store no slotted bucket
    B.handle(0, True, multi=True, compute=L.VBC_F64)
    assert not rec.flags[0][0] & NARROW
    B._handles.h.clear()


def test_python_narrow_with_updatable_is_an_argument_error():
    for B in (mat1d(), mat1d(np.float64), mat2d()):
        B.narrow = True
        B.updatable = True
        rec = Recorder(B)
        with pytest.raises(L.ArgumentError):
            B.handle(0, True, compute=L.VBC_F64)
        assert not rec.flags


def test_python_multi_gpu_classes_refuse_narrow():
    B = mat1d()
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0], narrow=True)
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2, narrow=True)
    B.narrow = True
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0])
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2)


def test_header_flag_version_and_exports():
    text = HEADER.read_text()
    assert re.search(r"#define\s+VBC_CREATE_NARROW_VALUES\s+0x80u\b", text)
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", text).group(1)) == 30400
    assert L.lib().vbc_version() == 30400
    assert NARROW == 0x80
    exported = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], check=True, capture_output=True,
                              text=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if " T " in ln}
    assert {n for n in names if n.startswith("vbc")} == set(L.ABI_SYMBOLS)  # no new symbol
