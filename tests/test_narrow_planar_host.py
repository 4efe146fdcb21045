"""Narrow planar storage (vbc.h VBC_CREATE_NARROW_PLANAR, 0x100, valid only with VBC_CREATE_NARROW_VALUES), the
parts that need no GPU: the refusals of the C ABI (decided before any device work), the Python rules of
`B.narrow = "planar"`, what the flag does to the arena image the planner builds (vbcx_plan_image under the device
facts recorded in tests/golden/plan_images.json), and the planner under AddressSanitizer / UBSan as a program of
its own (tests/host/narrow_planar_asan.cpp)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from sparsematrixvbcs_amd import _lib as L
from tests.test_narrow_host import Recorder, create_1d_ex, create_2d_ex, create_csc_ex, mat1d, mat2d
from tests.test_plan_host import GOLDEN, facts_from, plan_image

HEADER = L.PKG_DIR.parent / "include" / "vbc.h"
NARROW, PLANAR = L.VBC_CREATE_NARROW_VALUES, L.VBC_CREATE_NARROW_PLANAR
BOTH = NARROW | PLANAR
T, F = L.VBC_CREATE_TRANSPOSED, L.VBC_CREATE_FORWARD
# The chunk-planar layout of spmv_planar / spmv_planar_fwd at any size: no fused small split, no split product, no
# lane streams, no lane pairs.
PLAIN = {"VBC_SLOT_PLANAR": "1", "VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_PAIR": "0",
         "VBC_PLANAR_LANES": "0", "VBC_SLOTS": "1"}


def refused(st, h):
    assert st == L.VBC_INVALID_ARG
    assert not h.value  # *out left NULL
    msg = L.last_error()
    assert msg and "VBC_CREATE_NARROW_" in msg
    return True


def csc(np_dt):
    A = sp.random(40, 30, density=0.1, random_state=4, format="csc", dtype=np.float64).astype(np_dt)
    return V.SparseMatrixCSC(A)


def test_flag_and_header():
    assert PLANAR == 0x100
    text = HEADER.read_text()
    assert re.search(r"#define\s+VBC_CREATE_NARROW_PLANAR\s+0x100u\b", text)
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", text).group(1)) == 30400
    assert int(re.search(r"#define\s+VBC_INFO_SIZE\s+(\d+)", text).group(1)) == L.VBC_INFO_SIZE == 152
    assert L.lib().vbc_version() == 30400


def test_refused_without_narrow_values():
    f = T | PLANAR  # 0x100 alone
    assert refused(*create_1d_ex(mat1d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_2d_ex(mat2d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_csc_ex(csc(np.float32), L.VBC_F32, L.VBC_F64, f))


@pytest.mark.parametrize("val_dt,compute_dt,np_dt", [(L.VBC_F64, L.VBC_F64, np.float64), (L.VBC_F32, L.VBC_F32, np.float32),
                                                     (L.VBC_F64, L.VBC_F32, np.float64), (L.VBC_I32, L.VBC_F64, np.int32),
                                                     (L.VBC_BOOL, L.VBC_F64, np.bool_)])
def test_refused_for_any_other_eltype_pair(val_dt, compute_dt, np_dt):
    f = T | BOTH
    assert refused(*create_1d_ex(mat1d(np_dt), val_dt, compute_dt, f))
    if np_dt in (np.float64, np.float32):
        assert refused(*create_2d_ex(mat2d(np_dt), val_dt, compute_dt, f))
        assert refused(*create_csc_ex(csc(np_dt), val_dt, compute_dt, f))


@pytest.mark.parametrize("bits", [PLANAR, BOTH])
def test_refused_on_the_creates_without_types(bits):
    f = T | bits
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
        Cm = csc(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc_csc_create(C.byref(h), Cm.m, Cm.n, Cm.colptr.ctypes.data, Cm.rowval.ctypes.data,
                                    Cm.nzval.ctypes.data, dt, 0, f)
        assert refused(st, h)


def test_refused_together_with_updatable():
    f = T | BOTH | L.VBC_CREATE_UPDATABLE  # 0x20
    assert refused(*create_1d_ex(mat1d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_2d_ex(mat2d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_csc_ex(csc(np.float32), L.VBC_F32, L.VBC_F64, f))


@pytest.mark.parametrize("bits", [PLANAR, BOTH])
@pytest.mark.parametrize("upd", [0, L.VBC_CREATE_UPDATABLE_SHARDS])
def test_refused_on_the_sharded_creates(bits, upd):
    f = T | bits | upd
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


def test_python_narrow_planar_passes_both_bits_and_true_only_0x80():
    for narrow, want in ((True, NARROW), ("planar", BOTH), (False, 0), (None, 0)):
        for B in (mat1d(), mat2d(), csc(np.float32)):
            B.narrow = narrow
            rec = Recorder(B)
            B.handle(0, True, compute=L.VBC_F64)
            assert rec.flags[0][0] & BOTH == want, (narrow, type(B))
            B._handles.h.clear()  # nothing was created
    for dtype, compute in ((np.float32, L.VBC_F32), (np.float32, None), (np.float64, L.VBC_F64)):
        B = mat1d(dtype)  # any other eltype pair: the attribute is ignored, as narrow = True is
        B.narrow = "planar"
        rec = Recorder(B)
        B.handle(0, True, compute=compute)
        assert not rec.flags[0][0] & BOTH
        B._handles.h.clear()
    B = mat1d()
    B.narrow = "planar"
    rec = Recorder(B)  # the matrix-core panel layouts store no planar bucket
    B.handle(0, True, multi=True, compute=L.VBC_F64)
    assert not rec.flags[0][0] & BOTH
    B._handles.h.clear()


@pytest.mark.parametrize("bad", ["slotted", "Planar", 1, 2, 0x180, 1.0, ("planar",)])
def test_python_bad_narrow_value_is_a_value_error(bad):
    B = mat1d()
    B.narrow = bad
    rec = Recorder(B)
    with pytest.raises(ValueError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_narrow_planar_with_updatable_is_an_argument_error():
    B = mat1d()
    B.narrow = "planar"
    B.updatable = True
    rec = Recorder(B)
    with pytest.raises(L.ArgumentError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_multi_gpu_classes_refuse_narrow_planar():
    B = mat1d()
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0], narrow="planar")
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2, narrow="planar")
    B.narrow = "planar"
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0])
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2)


# ---- the planner's image (no device) ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def facts():
    return facts_from(json.loads(GOLDEN.read_text())["facts"])


def uniform_bucket(w, rows=7, stripes=128, m=300, seed=5, dof=1, circulant=False):
    """`stripes` w-wide stripes of `rows` runs of `dof` consecutive rows each, float32 values.  With 128 stripes
    (two full chunks of 64) the planar B'x layout pads nothing.  circulant: m = stripes * dof and stripe l holds
    the nodes l, l + 17, l + 34, ... (mod stripes), so every node row lies in exactly `rows` stripes and the forward
    run layout (segments = nodes) pads nothing either."""
    rng = np.random.default_rng(seed + w)
    if circulant:
        assert m == stripes * dof
        idx = np.concatenate([np.sort((l + 17 * np.arange(rows)) % stripes) for l in range(stripes)])
    else:
        idx = np.concatenate([np.sort(rng.choice(m // dof, rows, replace=False)) for _ in range(stripes)])
    idx = (idx[:, None] * dof + np.arange(dof)[None, :]).reshape(-1)
    cnt = np.full(stripes, rows * dof, np.int64)
    spl = 1 + np.arange(stripes + 1, dtype=np.int64) * w
    pos = np.concatenate([[1], 1 + np.cumsum(cnt)]).astype(np.int64)
    ofs = np.concatenate([[1], 1 + np.cumsum(cnt * w)]).astype(np.int64)
    val = rng.uniform(-1, 1, int(ofs[-1]) - 1).astype(np.float32)
    return V.SparseMatrix1DVBC(8, m, stripes * w, V.SplitPartition(spl), pos, idx.astype(np.int64) + 1, ofs, val)


def image(B, flags, facts, val=None):
    """The image a Float64 create of the float32 matrix B would upload (val widened, as vbc1d_create_ex does)."""
    v = np.ascontiguousarray((B.val if val is None else val).astype(np.float64))
    return plan_image(B, v, L.VBC_F64, flags, facts)


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("w", [3, 4, 5, 6, 7, 8])
def test_image_shrinks_by_four_bytes_per_stored_value(w, facts, monkeypatch):
    set_env(monkeypatch, PLAIN)
    B = uniform_bucket(w)
    nval = int(B.ofs[-1]) - 1  # two full chunks, equal stripes: every stored slot of the planar bucket is a value
    wide, n80, n180 = image(B, T, facts), image(B, T | NARROW, facts), image(B, T | BOTH, facts)
    print("w", w, "nval", nval, "wide", wide.size, "0x80", n80.size, "0x180", n180.size)
    assert wide.size == n80.size and np.array_equal(wide, n80)  # the planar bucket stays wide under 0x80 alone
    regions = 8  # values, outputs, ranges (2), keys / bases / offsets, the fill list: each may move by < 16 B
    assert 4 * nval <= n80.size - n180.size <= 4 * nval + 16 * regions


@pytest.mark.parametrize("dof", [2, 3])
def test_forward_image_shrinks_by_four_bytes_per_stored_value(dof, facts, monkeypatch):
    """The forward planar bin (spmv_planar_fwd) of a node-blocked operator: dof x dof blocks, every node row in
    the same number of stripes."""
    set_env(monkeypatch, PLAIN)
    B = uniform_bucket(dof, rows=5, stripes=128, m=128 * dof, seed=9, dof=dof, circulant=True)
    nval = int(B.ofs[-1]) - 1
    wide, n80, n180 = image(B, F, facts), image(B, F | NARROW, facts), image(B, F | BOTH, facts)
    print("forward dof", dof, "nval", nval, "wide", wide.size, "0x80", n80.size, "0x180", n180.size)
    assert np.array_equal(wide, n80)
    assert 4 * nval <= n80.size - n180.size <= 4 * nval + 16 * 8


@pytest.mark.parametrize("w", [3, 6])
def test_two_value_arrays_differ_in_four_bytes_per_value(w, facts, monkeypatch):
    set_env(monkeypatch, PLAIN)
    B = uniform_bucket(w)
    nval = int(B.ofs[-1]) - 1
    rng = np.random.default_rng(77)
    v1 = rng.uniform(1, 2, len(B.val)).astype(np.float32)
    v2 = (v1 + 4).astype(np.float32)  # every value differs
    a, b = image(B, T | BOTH, facts, v1), image(B, T | BOTH, facts, v2)
    assert a.size == b.size
    diff = int((a != b).sum())
    print("w", w, "bytes that differ", diff, "4 * nval", 4 * nval)
    assert 0 < diff <= 4 * nval
    aw, bw = image(B, T | NARROW, facts, v1), image(B, T | NARROW, facts, v2)
    assert int((aw != bw).sum()) > diff  # (wide values: up to 8 bytes each)
    # the narrow slots hold the floats themselves
    words = a[:a.size // 4 * 4].view(np.float32)
    assert np.isin(v1[:nval], words).all()


@pytest.mark.parametrize("env", [{"VBC_PLANAR_PAIR": "2"}, {"VBC_PLANAR_LANES": "1"}, {"VBC_PLANAR_SPLIT": "4"}],
                         ids=["pair", "lanes", "split"])
def test_other_planar_kernels_keep_wide_values(env, facts, monkeypatch):
    set_env(monkeypatch, {**PLAIN, **env})
    B = uniform_bucket(3, rows=6, dof=3)  # 3-wide stripes with rows in runs of 3: the pair layout applies
    a, b = image(B, T | NARROW, facts), image(B, T | BOTH, facts)
    assert a.size == b.size and np.array_equal(a, b)
    monkeypatch.setenv("VBC_PLANAR_PAIR", "0")
    monkeypatch.setenv("VBC_PLANAR_LANES", "0")
    monkeypatch.setenv("VBC_PLANAR_SPLIT", "0")
    assert image(B, T | BOTH, facts).size < a.size  # (the same matrix in the plain layout does shrink)


def test_plan_image_refuses_planar_bit_alone(facts):
    B = uniform_bucket(3)
    v = np.ascontiguousarray(B.val.astype(np.float64))
    n = C.c_size_t()
    st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                 B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64, T | PLANAR,
                                 C.byref(facts), None, 0, C.byref(n))
    assert st == L.VBC_INVALID_ARG and "VBC_CREATE_NARROW_PLANAR" in L.last_error()


def test_sanitized_planner_program(tmp_path, facts, monkeypatch):
    """tests/host/narrow_planar_asan.cpp: the planner's host code under AddressSanitizer and UBSan, as a program of
    its own, plans one B'x and one forward narrow-planar case (handed over in files, the format of
    tests/host/plan_asan.cpp) and returns the images the library itself plans."""
    exe = tmp_path / "narrow_planar_asan"
    src = L.PKG_DIR.parent / "tests" / "host" / "narrow_planar_asan.cpp"
    r = subprocess.run(["make", "-C", str(L.PKG_DIR), "-j8", f"PLAN_ASAN={exe}", f"ASAN_BUILD={tmp_path / 'obj'}",
                        f"PLAN_ASAN_SRC={src}", "plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    set_env(monkeypatch, PLAIN)
    cases = {"bx": (uniform_bucket(5, rows=6, stripes=150, dof=2), T),  # a partial last chunk, row runs of 2
             "fwd": (uniform_bucket(3, rows=5, stripes=150, m=450, seed=9, dof=3, circulant=True), F)}
    for name, (B, flags) in cases.items():
        val = np.ascontiguousarray(B.val.astype(np.float64))
        head = np.array([B.m, B.n, 0, B.W, 0, len(B.Phi), len(B.idx), len(val), L.VBC_F64, flags, 8], np.int64)
        parts = [head.tobytes(), bytes(facts)]
        parts += [np.ascontiguousarray(a, np.int64).tobytes() for a in (B.Phi.spl, B.pos, B.idx, B.ofs)] + [val.tobytes()]
        (tmp_path / f"{name}.case").write_bytes(b"".join(parts))
        out = [tmp_path / f"{name}.180", tmp_path / f"{name}.80"]
        r = subprocess.run([str(exe), str(tmp_path / f"{name}.case"), str(out[0]), str(out[1])],
                           env={**os.environ, **PLAIN}, capture_output=True, text=True)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        i180, i80 = (np.frombuffer(p.read_bytes(), np.uint8) for p in out)
        assert np.array_equal(i180, image(B, flags | BOTH, facts)), name
        assert np.array_equal(i80, image(B, flags | NARROW, facts)), name
        assert i180.size + 4 * (int(B.ofs[-1]) - 1) <= i80.size, name
