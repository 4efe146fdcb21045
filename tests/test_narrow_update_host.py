"""In-place value updates of narrow handles (vbc.h VBC_CREATE_NARROW_UPDATABLE, 0x200, valid only with
VBC_CREATE_NARROW_VALUES), the parts that need no GPU: the header, the refusals of the C ABI (decided before any
device work), the Python rules of `B.updatable = "narrow"`, and the value map itself (vbc_host.h vbcx_value_map,
under the device facts recorded in tests/golden/plan_images.json).

Map round trip: image(val0) from vbcx_plan_image, the map from vbcx_value_map, the map applied to val1 in numpy
(per-chunk stored size, zero and skip entries, canon entries as 0 + v) must give vbcx_plan_image(val1) byte for
byte.  val1 holds -0.0 and zeros where val0 had values.  Each case also says which stored sizes its chunks must
have, so that it tests the layout it means to test.  The map's host code runs under AddressSanitizer / UBSan as a
program of its own (tests/host/value_map_asan.cpp)."""
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
NARROW, PLANAR, NUPD = L.VBC_CREATE_NARROW_VALUES, L.VBC_CREATE_NARROW_PLANAR, L.VBC_CREATE_NARROW_UPDATABLE
UPD = L.VBC_CREATE_UPDATABLE
T, F = L.VBC_CREATE_TRANSPOSED, L.VBC_CREATE_FORWARD

# The knob sets of tests/test_gpu_narrow_planar.py (the plain chunk-planar kernels at any size, planar rows from
# width 3) and tests/test_gpu_narrow.py (VBC_SLOTS=1: slotted buckets at any size); SLOTTED keeps every width slotted.
PLAIN = {"VBC_SLOT_PLANAR": "1", "VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_PAIR": "0",
         "VBC_PLANAR_LANES": "0", "VBC_SLOTS": "1"}
SLOTTED = {**PLAIN, "VBC_SLOT_PLANAR": "0", "VBC_SLOT_RUNS": "0"}
ORDERS = {"masked": {"VBC_SLOTS_SORT": "2", "VBC_PLANAR_MASK": "1"}, "sorted": {"VBC_SLOTS_SORT": "2", "VBC_PLANAR_MASK": "0"}}


def csc(np_dt=np.float32):
    A = sp.random(40, 30, density=0.1, random_state=4, format="csc", dtype=np.float64).astype(np_dt)
    return V.SparseMatrixCSC(A)


def refused(st, h):
    assert st == L.VBC_INVALID_ARG
    assert not h.value  # no handle
    msg = L.last_error()
    assert msg and "VBC_CREATE_NARROW_UPDATABLE" in msg, msg
    return True


# ---- header and refusals ------------------------------------------------------------------------------------------

def test_flag_and_header():
    assert NUPD == 0x200
    text = HEADER.read_text()
    assert re.search(r"#define\s+VBC_CREATE_NARROW_UPDATABLE\s+0x200u\b", text)
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", text).group(1)) == 30400
    assert L.lib().vbc_version() == 30400
    assert "vbcx_value_map" in L.ABI_SYMBOLS and hasattr(L.lib(), "vbcx_value_map")


@pytest.mark.parametrize("bits", [NUPD, NUPD | PLANAR])
def test_refused_without_narrow_values(bits):
    f = T | bits
    assert refused(*create_1d_ex(mat1d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_2d_ex(mat2d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_csc_ex(csc(), L.VBC_F32, L.VBC_F64, f))


@pytest.mark.parametrize("bits", [NARROW, NARROW | PLANAR])
def test_refused_together_with_updatable(bits):
    f = T | bits | NUPD | UPD  # 0x200 with 0x20
    assert refused(*create_1d_ex(mat1d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_2d_ex(mat2d(), L.VBC_F32, L.VBC_F64, f))
    assert refused(*create_csc_ex(csc(), L.VBC_F32, L.VBC_F64, f))


@pytest.mark.parametrize("val_dt,compute_dt,np_dt", [(L.VBC_F64, L.VBC_F64, np.float64), (L.VBC_F32, L.VBC_F32, np.float32),
                                                     (L.VBC_F64, L.VBC_F32, np.float64), (L.VBC_I32, L.VBC_F64, np.int32),
                                                     (L.VBC_BOOL, L.VBC_F64, np.bool_)])
def test_refused_for_any_other_eltype_pair(val_dt, compute_dt, np_dt):
    f = T | NARROW | NUPD
    assert refused(*create_1d_ex(mat1d(np_dt), val_dt, compute_dt, f))
    if np_dt in (np.float64, np.float32):
        assert refused(*create_2d_ex(mat2d(np_dt), val_dt, compute_dt, f))
        assert refused(*create_csc_ex(csc(np_dt), val_dt, compute_dt, f))


@pytest.mark.parametrize("bits", [NUPD, NARROW | NUPD, NARROW | PLANAR | NUPD])
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


@pytest.mark.parametrize("bits", [NARROW | NUPD, NARROW | PLANAR | NUPD])
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


# ---- the Python mirror --------------------------------------------------------------------------------------------

def test_python_narrow_updatable_flags():
    for narrow, want in ((True, NARROW | NUPD), ("planar", NARROW | PLANAR | NUPD)):
        for B in (mat1d(), mat2d(), csc()):
            B.narrow = narrow
            B.updatable = "narrow"
            rec = Recorder(B)
            B.handle(0, True, compute=L.VBC_F64)
            B.handle(0, False, compute=L.VBC_F64)
            assert rec.flags[0][0] == T | want, (narrow, type(B), hex(rec.flags[0][0]))
            assert rec.flags[1][0] == F | want
            assert rec.flags[0][0] == (T | (0xA0 ^ 0x20 | 0x200) | (want & PLANAR))
            B._handles.h.clear()  # nothing was created


def test_python_narrow_updatable_where_narrow_is_ignored_or_unset():
    cases = [(mat1d(np.float64), True, L.VBC_F64), (mat1d(), True, L.VBC_F32), (mat1d(), "planar", None),
             (mat2d(np.float64), "planar", L.VBC_F64), (mat1d(), False, L.VBC_F64), (mat1d(), None, L.VBC_F64)]
    for B, narrow, compute in cases:
        B.narrow = narrow
        B.updatable = "narrow"
        rec = Recorder(B)
        B.handle(0, True, compute=compute)
        assert rec.flags[0][0] == T | UPD, (narrow, compute, hex(rec.flags[0][0]))  # as B.updatable = True
        B._handles.h.clear()
    B = mat1d()
    B.updatable = "narrow"  # no B.narrow attribute at all
    rec = Recorder(B)
    B.handle(0, True, compute=L.VBC_F64)
    assert rec.flags[0][0] == T | UPD
    B._handles.h.clear()
    B = mat1d()
    B.narrow, B.updatable = True, "narrow"
    rec = Recorder(B)  # the matrix-core panel layouts store nothing narrow
    B.handle(0, True, multi=True, compute=L.VBC_F64)
    assert rec.flags[0][0] == L.VBC_CREATE_MULTI | UPD
    B._handles.h.clear()


@pytest.mark.parametrize("bad", ["x", "Narrow", 1, 2, 0x200, 1.0, ("narrow",)])
def test_python_bad_updatable_value_is_a_value_error(bad):
    for narrow in (False, True):
        B = mat1d()
        B.narrow = narrow
        B.updatable = bad
        rec = Recorder(B)
        with pytest.raises(ValueError) as e:
            B.handle(0, True, compute=L.VBC_F64)
        assert not isinstance(e.value, L.ArgumentError) and not rec.flags


def test_python_true_with_narrow_still_an_argument_error():
    for narrow in (True, "planar"):
        B = mat1d()
        B.narrow, B.updatable = narrow, True
        rec = Recorder(B)
        with pytest.raises(L.ArgumentError):
            B.handle(0, True, compute=L.VBC_F64)
        assert not rec.flags


def test_python_update_values_refuses_float64_before_any_library_call(monkeypatch):
    B = mat1d()
    B.narrow, B.updatable = True, "narrow"
    Recorder(B)
    B.handle(0, True, compute=L.VBC_F64)  # records a 0x200 handle (a NULL pointer: nothing was created)
    B.handle(0, True, compute=L.VBC_F32)  # and a plain updatable one
    assert sorted(f for _, f, _ in B._handles.h) == [T | UPD, T | NARROW | NUPD]

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library call " + name)
    monkeypatch.setattr(L, "lib", lambda: NoCalls())
    old = B.val.copy()
    with pytest.raises(L.UnsupportedDtype):
        B.update_values(np.ones(len(B.val), np.float64))
    with pytest.raises(L.UnsupportedDtype):
        B.update_values(np.ones(len(B.val), np.int32))
    assert np.array_equal(B.val, old)
    monkeypatch.undo()
    B._handles.h.clear()


def test_python_multi_gpu_classes_still_refuse_narrow():
    B = mat1d()
    B.narrow, B.updatable = True, "narrow"
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0])
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2)


# ---- the value map (no device) ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def facts():
    return facts_from(json.loads(GOLDEN.read_text())["facts"])


def ragged(widths, R, stripes=170, seed=1):
    """tests/test_gpu_narrow_planar.py's ragged shape -- `stripes` stripes over m = 300 rows whose rows come in
    aligned runs of R, the first 128 stripes with 1 .. 40 / R nodes each, the rest (the partial last chunk of the
    natural order) 1 or 2 -- with one width for all stripes or one per stripe.  float32 values, none of them zero."""
    w = np.broadcast_to(np.asarray(widths, np.int64), (stripes,))
    rng = np.random.default_rng(seed + 10 * int(w[0]) + R)
    m = 300
    nodes = m // R
    cnt = np.where(np.arange(stripes) < 128, rng.integers(1, max(1, 40 // R) + 1, stripes), rng.integers(1, 3, stripes))
    idx = np.concatenate([np.sort(rng.choice(nodes, c, replace=False)) for c in cnt])
    idx = (idx[:, None] * R + np.arange(R)[None, :]).reshape(-1)
    rows = cnt.astype(np.int64) * R
    spl = np.concatenate([[1], 1 + np.cumsum(w)]).astype(np.int64)
    pos = np.concatenate([[1], 1 + np.cumsum(rows)]).astype(np.int64)
    ofs = np.concatenate([[1], 1 + np.cumsum(rows * w)]).astype(np.int64)
    val = rng.uniform(0.25, 1, int(ofs[-1]) - 1).astype(np.float32) * rng.choice([-1, 1], int(ofs[-1]) - 1).astype(np.float32)
    return V.SparseMatrix1DVBC(8, m, int(w.sum()), V.SplitPartition(spl), pos, idx.astype(np.int64) + 1, ofs, val)


def mixed_widths():
    """Widths 2 and 3 alternating: under PLAIN the 2-wide bucket is slotted and the 3-wide one planar."""
    return ragged(np.where(np.arange(170) % 2 == 0, 2, 3), 2)


def mesh(dof=2):
    return V.synthetic.fe_grid_2d(13, dof=dof, dtype=np.float32, seed=11 + dof)


def small_mixed():  # tests/test_plan_host.py's `mixed` (the narrow_via_t_f64 case): widths 1 .. 4, m = 60
    return V.synthetic.vbr_1dvbc(60, 12, 90, np.arange(12) % 4 + 1, W=4, dtype=np.float32, seed=3)


def blocks_2d():
    return V.synthetic.vbr_2d(40, 30, 300, 4, 4, dtype=np.float32, seed=19)


# name: (matrix, flags without 0x200, knobs, the stored sizes its chunks must have -- 0: Float64, 4: Float32)
CASES = {
    "slotted_bx_w1": (lambda: ragged(1, 2), T | NARROW, SLOTTED, {4}),
    "slotted_bx_w2_keys16": (lambda: ragged(2, 2), T | NARROW, {**SLOTTED, "VBC_SLOT_KEYS16": "2"}, {4}),
    "slotted_bx_w8": (lambda: ragged(8, 2), T | NARROW, SLOTTED, {4}),
    "slotted_fwd": (lambda: ragged(2, 2), F | NARROW, SLOTTED, {4}),
    "planar_w3_run1_masked": (lambda: ragged(3, 2), T | NARROW | PLANAR, {**PLAIN, "VBC_SLOT_RUNS": "0", **ORDERS["masked"]}, {4}),
    "planar_w3_run2_sorted": (lambda: ragged(3, 2), T | NARROW | PLANAR, {**PLAIN, "VBC_SLOT_RUNS": "1", **ORDERS["sorted"]}, {4}),
    "planar_w4_run1_sorted": (lambda: ragged(4, 2), T | NARROW | PLANAR, {**PLAIN, "VBC_SLOT_RUNS": "0", **ORDERS["sorted"]}, {4}),
    "planar_w4_run2_masked": (lambda: ragged(4, 2), T | NARROW | PLANAR, {**PLAIN, "VBC_SLOT_RUNS": "1", **ORDERS["masked"]}, {4}),
    "planar_w3_under_0x80_stays_wide": (lambda: ragged(3, 2), T | NARROW, PLAIN, {0}),
    "planar_fwd": (mesh, F | NARROW | PLANAR, {k: v for k, v in PLAIN.items() if k != "VBC_SLOTS"}, {4}),
    "mixed_0x80": (mixed_widths, T | NARROW, PLAIN, {0, 4}),
    "mixed_0x180": (mixed_widths, T | NARROW | PLANAR, PLAIN, {4}),
    # (its 3- and 4-wide buckets are planar, so wide under 0x80 alone: a mixed handle too)
    "fwd_on_bt": (small_mixed, T | F | NARROW, {"VBC_SLOTS": "1", "VBC_FWD_T": "2"}, {0, 4}),
    "two_d": (blocks_2d, T | F | NARROW, SLOTTED, {4}),
}
CHUNK = np.dtype([("dst", "<u8"), ("map", "<u8"), ("n", "<u4"), ("vsz", "<u4")])


def value_map(B, val64, flags, facts):
    two_d = hasattr(B, "Pi")
    args = (B.m, B.n, B.U if two_d else 0, B.W, len(B.Pi) if two_d else 0, B.Pi.spl.ctypes.data if two_d else None,
            len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data, B.idx.ctypes.data, B.ofs.ctypes.data, val64.ctypes.data,
            len(val64), L.VBC_F64, flags, C.byref(facts))
    ne, nc = C.c_int64(), C.c_int64()
    L.check(L.lib().vbcx_value_map(*args, None, 0, C.byref(ne), None, 0, C.byref(nc)), "vbcx_value_map")
    mp = np.full(ne.value, 0x12345678, np.uint32)
    ch = np.zeros(nc.value, CHUNK)
    assert CHUNK.itemsize == C.sizeof(L.vbcx_map_chunk) == 24
    L.check(L.lib().vbcx_value_map(*args, mp.ctypes.data, mp.size, C.byref(ne), ch.ctypes.data, ch.size, C.byref(nc)),
            "vbcx_value_map")
    assert (ne.value, nc.value) == (mp.size, ch.size)
    return mp, ch


def apply_map(img, mp, chunks, val32):
    """What the update kernel does to the arena, in numpy: every chunk's quads from its entries."""
    buf = np.concatenate([img, np.zeros(16, np.uint8)])  # (room for a last quad's skip entries; both views share it)
    views = {8: buf[: buf.size // 8 * 8].view(np.float64), 4: buf[: buf.size // 4 * 4].view(np.float32)}
    for c in chunks:
        sz = int(c["vsz"]) or 8
        assert sz in (4, 8)
        dt = np.float32 if sz == 4 else np.float64
        cnt = int(c["n"]) * (16 // sz)
        assert int(c["dst"]) % (16 // sz) == 0 and int(c["map"]) % (16 // sz) == 0  # whole, aligned quads
        ents = mp[int(c["map"]): int(c["map"]) + cnt]
        assert ents.size == cnt
        write = ents != L.VBCX_MAP_SKIP
        real = write & (ents != L.VBCX_MAP_ZERO)
        vals = np.zeros(cnt, dt)
        v = val32[ents[real] & 0x7FFFFFFF].astype(dt)
        canon = (ents[real] & L.VBCX_MAP_CANON) != 0
        v[canon] = dt(0) + v[canon]
        vals[real] = v
        at = int(c["dst"]) + np.arange(cnt)
        assert (at[write] * sz + sz <= img.size).all()  # nothing is written outside the arena
        views[sz][at[write]] = vals[write]
    return buf[: img.size].copy()


def second_values(B):
    """val1: other values, -0.0 and +0.0 where val0 had values (val0 has no zero), one NaN-free special or two."""
    nval = int(B.ofs[-1]) - 1
    rng = np.random.default_rng(99)
    v = rng.uniform(-2, 2, len(B.val)).astype(np.float32)
    at = rng.permutation(nval)
    v[at[: nval // 8]] = -0.0
    v[at[nval // 8: nval // 4]] = 0.0
    v[at[nval // 4]] = np.finfo(np.float32).smallest_subnormal
    v[at[nval // 4 + 1]] = -np.finfo(np.float32).max
    v[nval:] = 0
    assert (B.val[:nval] != 0).all() and np.signbit(v[:nval][v[:nval] == 0]).any()
    return v


def images_and_map(name, facts, monkeypatch):
    make, flags, env, sizes = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = make()
    assert B.val.dtype == np.float32
    v0 = np.ascontiguousarray(B.val.astype(np.float64))
    v1 = second_values(B)
    img0 = plan_image(B, v0, L.VBC_F64, flags, facts)
    img1 = plan_image(B, np.ascontiguousarray(v1.astype(np.float64)), L.VBC_F64, flags, facts)
    mp, ch = value_map(B, v0, flags | NUPD, facts)
    return B, flags, sizes, v0, v1, img0, img1, mp, ch


@pytest.mark.parametrize("name", sorted(CASES))
def test_map_round_trip(name, facts, monkeypatch):
    B, flags, sizes, v0, v1, img0, img1, mp, ch = images_and_map(name, facts, monkeypatch)
    nval = int(B.ofs[-1]) - 1
    print(name, "image", img0.size, "entries", mp.size, "chunks", ch.size, "stored sizes", sorted(set(ch["vsz"].tolist())))
    assert set(ch["vsz"].tolist()) == sizes  # the layout the case means to test
    assert img0.size == img1.size and not np.array_equal(img0, img1)
    assert np.array_equal(apply_map(img0, mp, ch, v1), img1)
    assert np.array_equal(apply_map(img1, mp, ch, B.val), img0)  # and back
    real = mp[(mp != L.VBCX_MAP_SKIP) & (mp != L.VBCX_MAP_ZERO)] & 0x7FFFFFFF
    assert real.max() < nval and np.unique(real).size == nval  # every stored value of the matrix is somewhere
    assert (ch["n"] >= 1).all() and (ch["n"] <= 1024).all()
    if name == "fwd_on_bt":  # canon entries inside a narrow region, and -0.0 among the values they rewrite
        canon = np.zeros(mp.size, bool)
        for c in ch[ch["vsz"] == 4]:
            e = mp[int(c["map"]): int(c["map"]) + 4 * int(c["n"])]
            canon[int(c["map"]): int(c["map"]) + e.size] = (e < L.VBCX_MAP_SKIP) & ((e & L.VBCX_MAP_CANON) != 0)
        assert canon.any()
        assert np.signbit(v1[mp[canon] & 0x7FFFFFFF][v1[mp[canon] & 0x7FFFFFFF] == 0]).any()
    else:
        assert not ((mp < L.VBCX_MAP_SKIP) & ((mp & L.VBCX_MAP_CANON) != 0)).any()


@pytest.mark.parametrize("name", ["slotted_bx_w2_keys16", "planar_w3_run2_sorted", "mixed_0x80", "fwd_on_bt", "two_d"])
def test_flag_changes_no_layout_and_is_not_part_of_the_map_request(name, facts, monkeypatch):
    B, flags, sizes, v0, v1, img0, img1, mp, ch = images_and_map(name, facts, monkeypatch)
    assert np.array_equal(plan_image(B, v0, L.VBC_F64, flags | NUPD, facts), img0)  # the image under 0x200
    mp2, ch2 = value_map(B, v0, flags, facts)  # (the three UPDATABLE bits are ignored by vbcx_value_map)
    assert np.array_equal(mp, mp2) and np.array_equal(ch, ch2)
    wide_flags = flags & ~(NARROW | PLANAR)
    mpw, chw = value_map(B, v0, wide_flags, facts)  # the wide handle's map: Float64 chunks only
    assert set(chw["vsz"].tolist()) == {0}
    imgw = plan_image(B, v0, L.VBC_F64, wide_flags, facts)
    v1w = np.ascontiguousarray(v1.astype(np.float64))
    assert np.array_equal(apply_map(imgw, mpw, chw, v1), plan_image(B, v1w, L.VBC_F64, wide_flags, facts))


def test_plan_image_and_value_map_refusals(facts):
    B = ragged(2, 2)
    v = np.ascontiguousarray(B.val.astype(np.float64))
    n = C.c_size_t()
    st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                 B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64, T | NUPD,
                                 C.byref(facts), None, 0, C.byref(n))
    assert st == L.VBC_INVALID_ARG and "VBC_CREATE_NARROW_UPDATABLE" in L.last_error()
    ne, nc = C.c_int64(), C.c_int64()
    st = L.lib().vbcx_value_map(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64, T | PLANAR,
                                C.byref(facts), None, 0, C.byref(ne), None, 0, C.byref(nc))
    assert st == L.VBC_INVALID_ARG and "VBC_CREATE_NARROW_PLANAR" in L.last_error()
    st = L.lib().vbcx_value_map(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, 3, L.VBC_F64, T | NARROW,
                                C.byref(facts), None, 0, C.byref(ne), None, 0, C.byref(nc))
    assert st == L.VBC_INVALID_ARG and "val shorter" in L.last_error()


def off_quad():
    """One 1-wide slotted bucket whose stored values end off a 16-byte quad of floats in its last region."""
    B = ragged(1, 1, stripes=131, seed=4)
    return B


def test_sanitized_value_map_program(tmp_path, facts, monkeypatch):
    """tests/host/value_map_asan.cpp: the recording plans and the map's host code under AddressSanitizer and UBSan,
    as a program of its own, on the mixed handle and on a case whose last region ends off a quad boundary; it
    returns the map the library itself gives."""
    exe = tmp_path / "value_map_asan"
    src = L.PKG_DIR.parent / "tests" / "host" / "value_map_asan.cpp"
    r = subprocess.run(["make", "-C", str(L.PKG_DIR), "-j8", f"PLAN_ASAN={exe}", f"ASAN_BUILD={tmp_path / 'obj'}",
                        f"PLAN_ASAN_SRC={src}", "plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cases = {"mixed": (mixed_widths(), T | NARROW | NUPD, PLAIN), "off_quad": (off_quad(), T | NARROW | NUPD, SLOTTED)}
    for name, (B, flags, env) in cases.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        val = np.ascontiguousarray(B.val.astype(np.float64))
        mp, ch = value_map(B, val, flags, facts)
        if name == "off_quad":
            last = ch[-1]
            tail = mp[int(last["map"]): int(last["map"]) + 4 * int(last["n"])][-4:]
            assert last["vsz"] == 4 and (tail == L.VBCX_MAP_SKIP).any(), tail  # the region ends inside a quad
        else:
            assert set(ch["vsz"].tolist()) == {0, 4}
        head = np.array([B.m, B.n, 0, B.W, 0, len(B.Phi), len(B.idx), len(val), L.VBC_F64, flags, 8], np.int64)
        parts = [head.tobytes(), bytes(facts)]
        parts += [np.ascontiguousarray(a, np.int64).tobytes() for a in (B.Phi.spl, B.pos, B.idx, B.ofs)] + [val.tobytes()]
        (tmp_path / f"{name}.case").write_bytes(b"".join(parts))
        out = [tmp_path / f"{name}.map", tmp_path / f"{name}.chunks"]
        r = subprocess.run([str(exe), str(tmp_path / f"{name}.case"), str(out[0]), str(out[1])],
                           env={**os.environ, **env}, capture_output=True, text=True)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        assert np.array_equal(np.frombuffer(out[0].read_bytes(), np.uint32), mp), name
        assert np.array_equal(np.frombuffer(out[1].read_bytes(), CHUNK), ch), name
