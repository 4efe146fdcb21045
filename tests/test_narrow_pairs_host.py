"""Narrow lane-pair storage (vbc.h VBC_CREATE_NARROW_PAIRS, 0x400, valid only with VBC_CREATE_NARROW_VALUES |
VBC_CREATE_NARROW_PLANAR), the parts that need no GPU: the header, the refusals of the C ABI (decided before any
device work), the Python rules of `B.narrow = "pairs"`, what the flag does to the arena image the planner builds
(vbcx_plan_image under the device facts recorded in tests/golden/plan_images.json), the value map of a 0x780 handle
(vbcx_value_map; the method of tests/test_narrow_update_host.py), and the planner under AddressSanitizer / UBSan as
a program of its own (tests/host/narrow_pairs_asan.cpp).

The arrangement: a narrow run-row is the wide run-row's 288 values as floats, 16 B per lane and a 128-B tail
(WIDE_OF_NARROW below), so the pair value region of the 0x580 image is the 0x180 image's region narrowed and
permuted within each run-row, 4 * 288 bytes per run-row."""
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
from tests.test_gpu_narrow_planar import ragged
from tests.test_narrow_host import Recorder, create_1d_ex, create_2d_ex, create_csc_ex, mat1d, mat2d
from tests.test_narrow_update_host import CHUNK, apply_map, value_map
from tests.test_plan_host import GOLDEN, facts_from, plan_image

HEADER = L.PKG_DIR.parent / "include" / "vbc.h"
NARROW, PLANAR, NUPD = L.VBC_CREATE_NARROW_VALUES, L.VBC_CREATE_NARROW_PLANAR, L.VBC_CREATE_NARROW_UPDATABLE
PAIRS = 0x400
N180, N580 = NARROW | PLANAR, NARROW | PLANAR | PAIRS
T, F = L.VBC_CREATE_TRANSPOSED, L.VBC_CREATE_FORWARD
# the lane-pair layout of spmv_planar_pair at any size, and the lane-pair streams of spmv_pair_lanes
PAIR = {"VBC_PLANAR_PAIR": "2", "VBC_SLOTS": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0", "VBC_PLANAR_LANES": "0"}
PAIR_LANES = {"VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "1", "VBC_SLOTS": "1", "VBC_PLANAR_SPLIT": "0",
              "VBC_SMALL_FUSE": "0"}
LAYOUTS = {"pair": PAIR, "pair_masked": {**PAIR, "VBC_SLOTS_SORT": "2"}, "pair_keys16": {**PAIR, "VBC_SLOT_KEYS16": "2"},
           "pair_lanes": PAIR_LANES}


def refused(st, h):
    assert st == L.VBC_INVALID_ARG
    assert not h.value  # *out left NULL
    msg = L.last_error()
    assert msg and "VBC_CREATE_NARROW_" in msg, msg
    return True


def csc(np_dt=np.float32):
    A = sp.random(40, 30, density=0.1, random_state=4, format="csc", dtype=np.float64).astype(np_dt)
    return V.SparseMatrixCSC(A)


def all_ex_creates(flags, val_dt=L.VBC_F32, compute_dt=L.VBC_F64, np_dt=np.float32):
    yield create_1d_ex(mat1d(np_dt), val_dt, compute_dt, flags)
    if np_dt in (np.float64, np.float32):
        yield create_2d_ex(mat2d(np_dt), val_dt, compute_dt, flags)
        yield create_csc_ex(csc(np_dt), val_dt, compute_dt, flags)


# ---- header and refusals ------------------------------------------------------------------------------------------

def test_flag_and_header():
    assert L.VBC_CREATE_NARROW_PAIRS == PAIRS == 0x400
    text = HEADER.read_text()
    assert re.search(r"#define\s+VBC_CREATE_NARROW_PAIRS\s+0x400u\b", text)
    entry = text[text.index("#define VBC_CREATE_NARROW_PAIRS"): text.index("/* mul flags */")]
    for word in ("spmv_planar_pair", "spmv_pair_lanes", "bit 16 / 17", "VBC_CREATE_NARROW_UPDATABLE", "bit-identical"):
        assert word in entry, word
    assert "bit 16" in text[text.index("typedef struct vbc_info"):] and "bit 17" in text[text.index("typedef struct vbc_info"):]
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", text).group(1)) == 30400
    assert int(re.search(r"#define\s+VBC_INFO_SIZE\s+(\d+)", text).group(1)) == L.VBC_INFO_SIZE == 152
    assert C.sizeof(L.vbc_info) == 152
    assert L.lib().vbc_version() == 30400


@pytest.mark.parametrize("bits", [PAIRS, PAIRS | NARROW, PAIRS | PLANAR, PAIRS | NUPD, PAIRS | NARROW | NUPD,
                                  PAIRS | PLANAR | NUPD])
def test_refused_without_0x80_or_without_0x100(bits):
    for st, h in all_ex_creates(T | bits):
        assert refused(st, h)
        assert "VBC_CREATE_NARROW_PAIRS" in L.last_error() or "VBC_CREATE_NARROW_UPDATABLE" in L.last_error()


@pytest.mark.parametrize("bits", [N580, N580 | NUPD])
def test_refused_together_with_updatable(bits):
    for st, h in all_ex_creates(T | bits | L.VBC_CREATE_UPDATABLE):  # 0x20
        assert refused(st, h)


@pytest.mark.parametrize("val_dt,compute_dt,np_dt", [(L.VBC_F64, L.VBC_F64, np.float64), (L.VBC_F32, L.VBC_F32, np.float32),
                                                     (L.VBC_F64, L.VBC_F32, np.float64), (L.VBC_I32, L.VBC_F64, np.int32),
                                                     (L.VBC_BOOL, L.VBC_F64, np.bool_)])
@pytest.mark.parametrize("bits", [N580, N580 | NUPD])
def test_refused_for_any_other_eltype_pair(val_dt, compute_dt, np_dt, bits):
    for st, h in all_ex_creates(T | bits, val_dt, compute_dt, np_dt):
        assert refused(st, h)


@pytest.mark.parametrize("bits", [PAIRS, N580, N580 | NUPD])
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


@pytest.mark.parametrize("bits", [PAIRS, N580, N580 | NUPD])
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


# ---- the Python rule ------------------------------------------------------------------------------------------------

def test_python_narrow_pairs_flags():
    every = N580 | NUPD | L.VBC_CREATE_UPDATABLE
    for updatable, want in ((False, N580), ("narrow", N580 | NUPD)):
        for B in (mat1d(), mat2d(), csc(np.float32)):
            B.narrow = "pairs"
            B.updatable = updatable
            rec = Recorder(B)
            B.handle(0, True, compute=L.VBC_F64)
            assert rec.flags[0][0] & every == want, (updatable, type(B))
            B._handles.h.clear()  # nothing was created
    for narrow, want in ((True, NARROW), ("planar", N180)):  # the other values pass what they passed
        B = mat1d()
        B.narrow = narrow
        rec = Recorder(B)
        B.handle(0, True, compute=L.VBC_F64)
        assert rec.flags[0][0] & every == want
        B._handles.h.clear()
    for dtype, compute in ((np.float32, L.VBC_F32), (np.float32, None), (np.float64, L.VBC_F64)):
        B = mat1d(dtype)  # any other eltype pair: the attribute is ignored
        B.narrow = "pairs"
        rec = Recorder(B)
        B.handle(0, True, compute=compute)
        assert not rec.flags[0][0] & N580
        B._handles.h.clear()
    B = mat1d()
    B.narrow = "pairs"
    rec = Recorder(B)  # the matrix-core panel layouts store no pair bucket
    B.handle(0, True, multi=True, compute=L.VBC_F64)
    assert not rec.flags[0][0] & N580
    B._handles.h.clear()


@pytest.mark.parametrize("bad", ["pair", "Pairs", "lanes", 0x400, 0x580, ("pairs",)])
def test_python_any_other_string_is_still_a_value_error(bad):
    B = mat1d()
    B.narrow = bad
    rec = Recorder(B)
    with pytest.raises(ValueError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_pairs_with_updatable_true_is_an_argument_error():
    B = mat1d()
    B.narrow = "pairs"
    B.updatable = True
    rec = Recorder(B)
    with pytest.raises(L.ArgumentError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_multi_gpu_classes_refuse_narrow_pairs():
    B = mat1d()
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0], narrow="pairs")
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2, narrow="pairs")
    B.narrow = "pairs"
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0])
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2)


def test_julia_shim_mirrors_the_flag():
    text = (L.PKG_DIR / "julia" / "SparseMatrixVBCsHIP.jl").read_text()
    assert re.search(r"const VBC_CREATE_NARROW_PAIRS = Cuint\(0x400\)", text)
    assert ":pairs" in text


# ---- the planner's image (no device) ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def facts():
    return facts_from(json.loads(GOLDEN.read_text())["facts"])


def pair_matrix(seed=1):
    """tests/test_gpu_narrow_planar.py's ragged shape with 3-wide stripes and rows in runs of 3 (85 stripes: three pair
    chunks of 32 stripes, the last one partial), no value zero and all values distinct."""
    B = ragged(3, 3, stripes=85, seed=seed)
    nval = int(B.ofs[-1]) - 1
    val = (1 + np.arange(len(B.val), dtype=np.float32) / 8192) * np.where(np.arange(len(B.val)) % 3 == 0, -1, 1).astype(np.float32)
    assert np.unique(val[:nval]).size == nval
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, val)


def image(B, flags, facts, val=None):
    v = np.ascontiguousarray((B.val if val is None else val).astype(np.float64))
    return plan_image(B, v, L.VBC_F64, flags, facts)


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# The kept arrangement of a narrow run-row (vbc_planar.h pair_load, form 1): lane l's 16 B at element 4 l -- even lane
# of stripe slot s {r0c0, r0c1, r1c0, r1c1}, odd lane {r0c2, r1c2, r2c2, r2c0} -- and r2c1 at 256 + s.  WIDE_OF_NARROW
# maps each narrow element to the wide run-row's (A = 4 s + {r0c0, r0c1, r0c2, r1c2}, B = 128 + 2 s + {r1c0, r1c1},
# C = 192 + s: r2c2, D = 224 + 2 s + {r2c0, r2c1}).
_S = np.arange(32)
WIDE_OF_NARROW = np.zeros(288, np.int64)
for _k, _w in enumerate((4 * _S, 4 * _S + 1, 128 + 2 * _S, 129 + 2 * _S, 4 * _S + 2, 4 * _S + 3, 192 + _S, 224 + 2 * _S)):
    WIDE_OF_NARROW[8 * _S + _k] = _w
WIDE_OF_NARROW[256 + _S] = 225 + 2 * _S
assert np.array_equal(np.sort(WIDE_OF_NARROW), np.arange(288))


def al256(x):
    return (x + 255) // 256 * 256


def pair_region(i180, i580):
    """(offset, run-rows) of the one pair value region: both images are equal before it, the 0x180 image holds
    rows * 288 doubles there and the 0x580 image rows * 288 floats, and every later region (each on its own 256-B
    reservation) is byte-equal."""
    assert i580.size < i180.size
    first = int(np.flatnonzero(i180[: i580.size] != i580)[0])
    o = first // 256 * 256
    rows = [r for r in range(1, (i180.size - o) // 2304 + 1)
            if al256(r * 2304) - al256(r * 1152) == i180.size - i580.size
            and np.array_equal(i180[o + al256(r * 2304):], i580[o + al256(r * 1152):])]
    assert len(rows) == 1, rows
    return o, rows[0]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_image_differs_in_the_pair_value_region_only(layout, facts, monkeypatch):
    set_env(monkeypatch, LAYOUTS[layout])
    B = pair_matrix()
    nval = int(B.ofs[-1]) - 1
    wide, i180, i580 = image(B, T, facts), image(B, T | N180, facts), image(B, T | N580, facts)
    assert np.array_equal(wide, i180)  # 0x180 alone: the pair buckets stay wide (the documented behaviour)
    o, rows = pair_region(i180, i580)  # (asserts that every other region is byte-equal)
    print(layout, "sizes", i180.size, i580.size, "region at", o, "run-rows", rows, "nval", nval)
    assert np.array_equal(i180[:o], i580[:o])
    assert 288 * rows >= nval
    v64 = i180[o: o + rows * 2304].view(np.float64).reshape(rows, 288)
    v32 = i580[o: o + rows * 1152].view(np.float32).reshape(rows, 288)  # 4 * 288 bytes per run-row, no padding between
    # the narrow run-row is the wide one's values, each at the position the arrangement defines
    assert np.array_equal(v64[:, WIDE_OF_NARROW].astype(np.float32).view(np.uint32), v32.view(np.uint32))
    stored = v32[v32 != 0]
    assert stored.size == nval and np.array_equal(np.sort(stored), np.sort(B.val[:nval]))  # the inputs, each once
    if layout in ("pair", "pair_keys16"):  # natural order: slot s of run-row 0 is stripe s's first run
        for sl in (0, 1, 31):
            o1 = int(B.ofs[sl]) - 1
            run = B.val[o1: o1 + 9].reshape(3, 3)  # [row][column]
            row0 = v32[0]
            assert np.array_equal(row0[8 * sl: 8 * sl + 4], [run[0, 0], run[0, 1], run[1, 0], run[1, 1]])  # even lane
            assert np.array_equal(row0[8 * sl + 4: 8 * sl + 8], [run[0, 2], run[1, 2], run[2, 2], run[2, 0]])  # odd lane
            assert row0[256 + sl] == run[2, 1]  # the tail


def test_special_values_keep_their_bits(facts, monkeypatch):
    set_env(monkeypatch, PAIR)
    B = pair_matrix()
    fi = np.finfo(np.float32)
    v = B.val.copy()
    special = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x7F7FFFFF],
                       np.uint32).view(np.float32)  # NaNs with payloads, -0, +-Inf, subnormals, FLT_MAX
    v[10: 10 + special.size] = special
    assert np.isnan(v[10]) and v[17] == fi.max
    i180, i580 = image(B, T | N180, facts, v), image(B, T | N580, facts, v)
    o, rows = pair_region(i180, i580)
    v32 = i580[o: o + rows * 1152].view(np.uint32)
    for bits in special.view(np.uint32):
        assert (v32 == bits).sum() >= 1, hex(int(bits))
    nval = int(B.ofs[-1]) - 1
    assert np.array_equal(np.sort(v32[v32 != 0]), np.sort(v[:nval].view(np.uint32)))  # every input's bits, nothing else


def test_plan_image_and_value_map_refuse_the_bit_without_0x180(facts):
    B = pair_matrix()
    v = np.ascontiguousarray(B.val.astype(np.float64))
    n, ne, nc = C.c_size_t(), C.c_int64(), C.c_int64()
    for bits in (PAIRS, PAIRS | NARROW, PAIRS | PLANAR):
        st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                     B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64, T | bits,
                                     C.byref(facts), None, 0, C.byref(n))
        assert st == L.VBC_INVALID_ARG and "VBC_CREATE_NARROW_" in L.last_error()
        st = L.lib().vbcx_value_map(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                    B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64, T | bits,
                                    C.byref(facts), None, 0, C.byref(ne), None, 0, C.byref(nc))
        assert st == L.VBC_INVALID_ARG and "VBC_CREATE_NARROW_" in L.last_error()


# ---- the value map of a 0x780 handle ---------------------------------------------------------------------------------

def second_values(B):
    nval = int(B.ofs[-1]) - 1
    rng = np.random.default_rng(99)
    v = rng.uniform(-2, 2, len(B.val)).astype(np.float32)
    at = rng.permutation(nval)
    v[at[: nval // 8]] = -0.0
    v[at[nval // 8: nval // 4]] = 0.0
    v[at[nval // 4]] = np.finfo(np.float32).smallest_subnormal
    v[at[nval // 4 + 1]] = -np.finfo(np.float32).max
    v[nval:] = 0
    return v


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_map_round_trip(layout, facts, monkeypatch):
    """The map of the 0x780 handle, applied in numpy to a second float32 value array, gives vbcx_plan_image of that
    array byte for byte (and back): the recording plans' pair writers copied tags where the builders narrow, and
    the pair value regions are in the recorder's narrow list."""
    set_env(monkeypatch, LAYOUTS[layout])
    B = pair_matrix()
    nval = int(B.ofs[-1]) - 1
    v0 = np.ascontiguousarray(B.val.astype(np.float64))
    v1 = second_values(B)
    img0, img1 = image(B, T | N580, facts), image(B, T | N580, facts, v1)
    mp, ch = value_map(B, v0, T | N580 | NUPD, facts)
    print(layout, "image", img0.size, "entries", mp.size, "chunks", ch.size, "stored sizes", sorted(set(ch["vsz"].tolist())))
    assert set(ch["vsz"].tolist()) == {4}  # the one bucket is a narrow pair bucket
    assert img0.size == img1.size and not np.array_equal(img0, img1)
    assert np.array_equal(apply_map(img0, mp, ch, v1), img1)
    assert np.array_equal(apply_map(img1, mp, ch, B.val), img0)
    real = mp[(mp != L.VBCX_MAP_SKIP) & (mp != L.VBCX_MAP_ZERO)] & 0x7FFFFFFF
    assert real.max() < nval and np.unique(real).size == nval
    assert (ch["dst"] * 4 % 16 == 0).all()  # whole float quads: the regions start on 256-B reservations
    assert np.array_equal(image(B, T | N580 | NUPD, facts), img0)  # 0x200 changes no layout
    # under 0x180 | 0x200 the same bucket is wide: Float64 chunks
    mpw, chw = value_map(B, v0, T | N180 | NUPD, facts)
    assert set(chw["vsz"].tolist()) == {0}


# ---- the sanitized program ---------------------------------------------------------------------------------------------

def test_sanitized_planner_program(tmp_path, facts, monkeypatch):
    """tests/host/narrow_pairs_asan.cpp: the planner's and the value map's host code under AddressSanitizer and UBSan,
    as a program of its own (no preloaded runtime), plans a pair and a pair-lanes matrix with 0x580 and 0x780 and
    returns the image and the map the library itself gives."""
    exe = tmp_path / "narrow_pairs_asan"
    src = L.PKG_DIR.parent / "tests" / "host" / "narrow_pairs_asan.cpp"
    r = subprocess.run(["make", "-C", str(L.PKG_DIR), "-j8", f"PLAN_ASAN={exe}", f"ASAN_BUILD={tmp_path / 'obj'}",
                        f"PLAN_ASAN_SRC={src}", "plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    B = pair_matrix()
    val = np.ascontiguousarray(B.val.astype(np.float64))
    for name in ("pair_masked", "pair_keys16", "pair_lanes"):
        env = LAYOUTS[name]
        for k in ("VBC_SLOTS_SORT", "VBC_SLOT_KEYS16", "VBC_PLANAR_PAIR", "VBC_PLANAR_LANES", "VBC_LANES_PAIR"):
            monkeypatch.delenv(k, raising=False)
        set_env(monkeypatch, env)
        head = np.array([B.m, B.n, 0, B.W, 0, len(B.Phi), len(B.idx), len(val), L.VBC_F64, T, 8], np.int64)
        parts = [head.tobytes(), bytes(facts)]
        parts += [np.ascontiguousarray(a, np.int64).tobytes() for a in (B.Phi.spl, B.pos, B.idx, B.ofs)] + [val.tobytes()]
        (tmp_path / f"{name}.case").write_bytes(b"".join(parts))
        out = [tmp_path / f"{name}.{s}" for s in ("580", "map", "chunks")]
        clean = {k: v for k, v in os.environ.items() if not k.startswith("VBC_") and k != "LD_PRELOAD"}
        r = subprocess.run([str(exe), str(tmp_path / f"{name}.case")] + [str(p) for p in out], env={**clean, **env},
                           capture_output=True, text=True)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        i580 = image(B, T | N580, facts)
        assert i580.size < image(B, T | N180, facts).size, name
        assert np.array_equal(np.frombuffer(out[0].read_bytes(), np.uint8), i580), name
        mp, ch = value_map(B, val, T | N580 | NUPD, facts)
        assert np.array_equal(np.frombuffer(out[1].read_bytes(), np.uint32), mp), name
        assert np.array_equal(np.frombuffer(out[2].read_bytes(), CHUNK), ch), name
