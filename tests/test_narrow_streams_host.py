"""Narrow lane-stream storage (vbc.h VBC_CREATE_NARROW_STREAMS, 0x800, valid only with VBC_CREATE_NARROW_VALUES |
VBC_CREATE_NARROW_PLANAR | VBC_CREATE_NARROW_PAIRS), the parts that need no GPU: the header, the refusals of the C
ABI (decided before any device work), the Python rules of `B.narrow = "streams"`, what the flag does to the arena
image the planner builds (vbcx_plan_image under the device facts recorded in tests/golden/plan_images.json), the
value map of a 0xF80 handle (vbcx_value_map; the method of tests/test_narrow_update_host.py), and the planner under
AddressSanitizer / UBSan as a program of its own (tests/host/narrow_streams_asan.cpp).

The arrangement: a narrow stored row of a lane bucket is the wide row's 64 * w values as floats in the Float32
column-group arrangement (planar_off(4, w, lane, column): 16-B groups of four floats, the last group narrower), so the
lane value region of the 0xD80 image is the 0x580 image's region narrowed and permuted within each row, 4 * 64 * w
bytes per row.  (The second arrangement the issue of this work allowed -- a lane's whole run fetched as 16 + 16 + 4
B -- was not built.)"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_narrow_planar import ragged
from tests.test_narrow_host import Recorder, mat1d, mat2d
from tests.test_narrow_pairs_host import al256, all_ex_creates, csc, image, refused, second_values, set_env
from tests.test_narrow_update_host import CHUNK, apply_map, value_map
from tests.test_plan_host import GOLDEN, facts_from

HEADER = L.PKG_DIR.parent / "include" / "vbc.h"
NARROW, PLANAR, NUPD = L.VBC_CREATE_NARROW_VALUES, L.VBC_CREATE_NARROW_PLANAR, L.VBC_CREATE_NARROW_UPDATABLE
PAIRS, STREAMS = L.VBC_CREATE_NARROW_PAIRS, 0x800
N580, ND80 = NARROW | PLANAR | PAIRS, NARROW | PLANAR | PAIRS | STREAMS
T, F = L.VBC_CREATE_TRANSPOSED, L.VBC_CREATE_FORWARD
# 0x800 with each proper subset of {0x80, 0x100, 0x400}
INCOMPLETE = [STREAMS | s for s in (0, NARROW, PLANAR, PAIRS, NARROW | PLANAR, NARROW | PAIRS, PLANAR | PAIRS)]
# the plain lane streams of spmv_planar_lanes at any size; the forward ones
LANES = {"VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "0", "VBC_SLOTS": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0"}
FWD_LANES = {**LANES, "VBC_PLANAR_PAIR": "0"}
TARGETS = ("1", "256")


def names_streams():
    msg = L.last_error()
    assert "VBC_CREATE_NARROW_STREAMS" in msg, msg
    return True


# ---- header and refusals ------------------------------------------------------------------------------------------

def test_flag_and_header():
    assert L.VBC_CREATE_NARROW_STREAMS == STREAMS == 0x800
    text = HEADER.read_text()
    assert re.search(r"#define\s+VBC_CREATE_NARROW_STREAMS\s+0x800u\b", text)
    entry = text[text.index("#define VBC_CREATE_NARROW_STREAMS"): text.index("/* mul flags */")]
    entry = re.sub(r"\s+", " ", entry)
    for word in ("spmv_planar_lanes", "bit 18 / 19", "VBC_CREATE_NARROW_UPDATABLE", "bit-identical"):
        assert word in entry, word
    info = text[text.index("typedef struct vbc_info"):]
    assert "bit 18" in info and "bit 19" in info
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", text).group(1)) == 30400
    assert int(re.search(r"#define\s+VBC_INFO_SIZE\s+(\d+)", text).group(1)) == L.VBC_INFO_SIZE == 152
    assert C.sizeof(L.vbc_info) == 152
    assert L.lib().vbc_version() == 30400


@pytest.mark.parametrize("upd", [0, NUPD])
@pytest.mark.parametrize("bits", INCOMPLETE)
def test_refused_without_any_one_of_the_three(bits, upd):
    for st, h in all_ex_creates(T | bits | upd):
        assert refused(st, h) and names_streams()


@pytest.mark.parametrize("bits", [ND80, ND80 | NUPD])
def test_refused_together_with_updatable(bits):
    for st, h in all_ex_creates(T | bits | L.VBC_CREATE_UPDATABLE):  # 0x20
        assert refused(st, h) and names_streams()


@pytest.mark.parametrize("val_dt,compute_dt,np_dt", [(L.VBC_F64, L.VBC_F64, np.float64), (L.VBC_F32, L.VBC_F32, np.float32),
                                                     (L.VBC_F64, L.VBC_F32, np.float64), (L.VBC_I32, L.VBC_F64, np.int32),
                                                     (L.VBC_BOOL, L.VBC_F64, np.bool_)])
@pytest.mark.parametrize("bits", [ND80, ND80 | NUPD])
def test_refused_for_any_other_eltype_pair(val_dt, compute_dt, np_dt, bits):
    for st, h in all_ex_creates(T | bits, val_dt, compute_dt, np_dt):
        assert refused(st, h) and names_streams()


@pytest.mark.parametrize("bits", [STREAMS, ND80, ND80 | NUPD])
def test_refused_on_the_creates_without_types(bits):
    f = T | bits
    for dt, np_dt in ((L.VBC_F64, np.float64), (L.VBC_F32, np.float32)):
        B = mat1d(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc1d_create(C.byref(h), B.m, B.n, B.W, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                  B.idx.ctypes.data, B.ofs.ctypes.data, B.val.ctypes.data, len(B.val), dt, 0, f)
        assert refused(st, h) and names_streams()
        B2 = mat2d(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc2d_create(C.byref(h), B2.m, B2.n, B2.U, B2.W, len(B2.Pi), B2.Pi.spl.ctypes.data, len(B2.Phi),
                                  B2.Phi.spl.ctypes.data, B2.pos.ctypes.data, B2.idx.ctypes.data, B2.ofs.ctypes.data,
                                  B2.val.ctypes.data, len(B2.val), dt, 0, f)
        assert refused(st, h) and names_streams()
        Cm = csc(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc_csc_create(C.byref(h), Cm.m, Cm.n, Cm.colptr.ctypes.data, Cm.rowval.ctypes.data,
                                    Cm.nzval.ctypes.data, dt, 0, f)
        assert refused(st, h) and names_streams()


@pytest.mark.parametrize("bits", [STREAMS, ND80, ND80 | NUPD])
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
    assert refused(st, h) and names_streams()
    B2 = mat2d()
    h = C.c_void_p()
    st = L.lib().vbc2d_create_sharded(C.byref(h), B2.m, B2.n, B2.U, B2.W, len(B2.Pi), B2.Pi.spl.ctypes.data, len(B2.Phi),
                                      B2.Phi.spl.ctypes.data, B2.pos.ctypes.data, B2.idx.ctypes.data, B2.ofs.ctypes.data,
                                      B2.val.ctypes.data, len(B2.val), C.byref(t), 2, devs, L.VBC_SPLIT_STRIPES, f)
    assert refused(st, h) and names_streams()


# ---- the Python rule ------------------------------------------------------------------------------------------------

def test_python_narrow_streams_flags():
    every = ND80 | NUPD | L.VBC_CREATE_UPDATABLE
    for updatable, want in ((False, ND80), ("narrow", ND80 | NUPD)):
        assert want in (0xD80, 0xF80)
        for B in (mat1d(), mat2d(), csc(np.float32)):
            B.narrow = "streams"
            B.updatable = updatable
            rec = Recorder(B)
            B.handle(0, True, compute=L.VBC_F64)
            assert rec.flags[0][0] & every == want, (updatable, type(B))
            B._handles.h.clear()  # nothing was created
    for narrow, want in ((True, NARROW), ("planar", NARROW | PLANAR), ("pairs", N580)):  # the older values pass what they passed
        B = mat1d()
        B.narrow = narrow
        rec = Recorder(B)
        B.handle(0, True, compute=L.VBC_F64)
        assert rec.flags[0][0] & every == want
        B._handles.h.clear()
    for dtype, compute in ((np.float32, L.VBC_F32), (np.float32, None), (np.float64, L.VBC_F64)):
        B = mat1d(dtype)  # any other eltype pair: the attribute is ignored
        B.narrow = "streams"
        rec = Recorder(B)
        B.handle(0, True, compute=compute)
        assert not rec.flags[0][0] & ND80
        B._handles.h.clear()
    B = mat1d()
    B.narrow = "streams"
    rec = Recorder(B)  # the matrix-core panel layouts store no lane bucket
    B.handle(0, True, multi=True, compute=L.VBC_F64)
    assert not rec.flags[0][0] & ND80
    B._handles.h.clear()


@pytest.mark.parametrize("bad", ["stream", "Streams", "lanes", 0x800, 0xD80, ("streams",)])
def test_python_any_other_value_is_still_a_value_error(bad):
    B = mat1d()
    B.narrow = bad
    rec = Recorder(B)
    with pytest.raises(ValueError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_streams_with_updatable_true_is_an_argument_error():
    B = mat1d()
    B.narrow = "streams"
    B.updatable = True
    rec = Recorder(B)
    with pytest.raises(L.ArgumentError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_multi_gpu_classes_refuse_narrow_streams():
    B = mat1d()
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0], narrow="streams")
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2, narrow="streams")
    B.narrow = "streams"
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0])
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2)


def test_julia_shim_mirrors_the_flag():
    text = (L.PKG_DIR / "julia" / "SparseMatrixVBCsHIP.jl").read_text()
    assert re.search(r"const VBC_CREATE_NARROW_STREAMS = Cuint\(0x800\)", text)
    assert ":streams" in text


# ---- the planner's image (no device) ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def facts():
    return facts_from(json.loads(GOLDEN.read_text())["facts"])


def distinct(B):
    """B with no value zero and all values distinct (exact in float32)."""
    nval = int(B.ofs[-1]) - 1
    val = (1 + np.arange(len(B.val), dtype=np.float32) / 8192) * np.where(np.arange(len(B.val)) % 3 == 0, -1, 1).astype(np.float32)
    assert np.unique(val[:nval]).size == nval
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, val)


def forward_operand():
    """The forward-lanes operand of tests/test_gpu_narrow_streams.py: a 3-dof stiffness matrix of 300 nodes with one
    node zeroed (empty segments), distinct values."""
    A = V.synthetic.fe_stiffness_3d(900, 40000, 3, np.float32).tolil()
    A[30:33, :] = 0.0
    A[:, 30:33] = 0.0
    A = A.tocsc()
    A.eliminate_zeros()
    return distinct(V.SparseMatrix1DVBC[8](A.T.tocsc(), V.StrictChunker(8)))


# name -> (matrix, create direction, knobs, width of a stored row's lane slot = the kernel's W)
def case(name):
    if name == "bx_w3_r3":
        return distinct(ragged(3, 3, stripes=85)), T, LANES, 3
    if name == "bx_w5_r2":
        return distinct(ragged(5, 2, stripes=85)), T, LANES, 5
    assert name == "forward"
    return forward_operand(), F, FWD_LANES, 3  # (rows and columns exchanged: W = the R = 3 rows of a node)


CASES = ("bx_w3_r3", "bx_w5_r2", "forward")


def planar_off(esz, w, s, c):
    """vbc_planar.h planar_off: element offset of (slot s, column c) in a stored row of width w."""
    G = 16 // esz
    g = c // G
    vg = min(w - g * G, G)
    return 64 * g * G + s * vg + (c - g * G)


def row_maps(w):
    """Element offsets of (lane, column), lane-major, in a wide and in a narrow stored row of 64 * w values."""
    wide = np.array([planar_off(8, w, l, c) for l in range(64) for c in range(w)])
    narrow = np.array([planar_off(4, w, l, c) for l in range(64) for c in range(w)])
    assert np.array_equal(np.sort(wide), np.arange(64 * w)) and np.array_equal(np.sort(narrow), np.arange(64 * w))
    return wide, narrow


def lane_region(i580, iD80, w):
    """(offset, stored rows) of the one lane value region: both images are equal before it, the 0x580 image holds
    rows * 64 * w doubles there and the 0xD80 image rows * 64 * w floats, and every later region (each on its own
    256-B reservation) is byte-equal."""
    assert iD80.size < i580.size
    first = int(np.flatnonzero(i580[: iD80.size] != iD80)[0])
    o = first // 256 * 256
    wb, nb = 8 * 64 * w, 4 * 64 * w
    rows = [r for r in range(1, (i580.size - o) // wb + 1)
            if al256(r * wb) - al256(r * nb) == i580.size - iD80.size
            and np.array_equal(i580[o + al256(r * wb):], iD80[o + al256(r * nb):])]
    assert len(rows) == 1, rows
    return o, rows[0]


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", CASES)
def test_image_differs_in_the_lane_value_region_only(name, target, facts, monkeypatch):
    B, direction, env, w = case(name)
    set_env(monkeypatch, {**env, "VBC_TARGET_RANGES_L": target})
    nval = int(B.ofs[-1]) - 1
    wide, i580, iD80 = image(B, direction, facts), image(B, direction | N580, facts), image(B, direction | ND80, facts)
    assert np.array_equal(wide, i580)  # 0x580 alone: the lane streams stay wide (the documented behaviour)
    o, rows = lane_region(i580, iD80, w)  # (asserts that every other region is byte-equal)
    print(name, target, "sizes", i580.size, iD80.size, "region at", o, "rows", rows, "nval", nval)
    assert np.array_equal(i580[:o], iD80[:o])
    assert 64 * w * rows >= nval
    v64 = i580[o: o + rows * 512 * w].view(np.float64).reshape(rows, 64 * w)
    v32 = iD80[o: o + rows * 256 * w].view(np.float32).reshape(rows, 64 * w)  # 4 * 64 * w bytes per row, no padding between
    wide_at, narrow_at = row_maps(w)
    # row by row, the narrow row is the wide one's values, each at planar_off(4, w, lane, column)
    assert np.array_equal(v64[:, wide_at].astype(np.float32).view(np.uint32), v32[:, narrow_at].view(np.uint32))
    stored = v32[v32 != 0]
    assert stored.size == nval and np.array_equal(np.sort(stored), np.sort(B.val[:nval]))  # the inputs, each once
    assert np.count_nonzero(v64) == nval


def test_first_rows_of_a_single_tile(facts, monkeypatch):
    """One tile of all 85 stripes: the stream that starts at stripe 0 belongs to one lane, and the rows d = 0 .. 2 of
    stripe 0's first node run sit in stored rows 0 .. 2 at planar_off(4, 3, lane, c)."""
    B, direction, env, w = case("bx_w3_r3")
    set_env(monkeypatch, {**env, "VBC_TARGET_RANGES_L": "1"})
    i580, iD80 = image(B, direction | N580, facts), image(B, direction | ND80, facts)
    o, rows = lane_region(i580, iD80, w)
    v32 = iD80[o: o + rows * 256 * w].view(np.float32).reshape(rows, 64 * w)
    run = B.val[:9].reshape(3, 3)  # stripe 0's first node run, [row][column]
    lanes = [l for l in range(64) if v32[0, planar_off(4, 3, l, 0)] == run[0, 0]]
    assert len(lanes) == 1
    for d in range(3):
        for c in range(3):
            assert v32[d, planar_off(4, 3, lanes[0], c)] == run[d, c]
    assert 12 * lanes[0] == 4 * planar_off(4, 3, lanes[0], 0)  # a lane's 3 floats are one 12-B load


def test_special_values_keep_their_bits(facts, monkeypatch):
    B, direction, env, w = case("bx_w3_r3")
    set_env(monkeypatch, {**env, "VBC_TARGET_RANGES_L": "256"})
    fi = np.finfo(np.float32)
    v = B.val.copy()
    special = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x7F7FFFFF],
                       np.uint32).view(np.float32)  # NaNs with payloads, -0, +-Inf, subnormals, FLT_MAX
    v[10: 10 + special.size] = special
    assert np.isnan(v[10]) and v[17] == fi.max
    i580, iD80 = image(B, direction | N580, facts, v), image(B, direction | ND80, facts, v)
    o, rows = lane_region(i580, iD80, w)
    v32 = iD80[o: o + rows * 256 * w].view(np.uint32)
    for bits in special.view(np.uint32):
        assert (v32 == bits).sum() >= 1, hex(int(bits))
    nval = int(B.ofs[-1]) - 1
    assert np.array_equal(np.sort(v32[v32 != 0]), np.sort(v[:nval].view(np.uint32)))  # every input's bits, nothing else


def test_plan_image_and_value_map_refuse_the_incomplete_combinations(facts):
    B = case("bx_w3_r3")[0]
    v = np.ascontiguousarray(B.val.astype(np.float64))
    n, ne, nc = C.c_size_t(), C.c_int64(), C.c_int64()
    for bits in INCOMPLETE:
        st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                     B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64, T | bits,
                                     C.byref(facts), None, 0, C.byref(n))
        assert st == L.VBC_INVALID_ARG and names_streams(), hex(bits)
        st = L.lib().vbcx_value_map(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                    B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64, T | bits,
                                    C.byref(facts), None, 0, C.byref(ne), None, 0, C.byref(nc))
        assert st == L.VBC_INVALID_ARG and names_streams(), hex(bits)


# ---- the value map of a 0xF80 handle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_map_round_trip(name, facts, monkeypatch):
    """The map of the 0xF80 handle, applied in numpy to a second float32 value array, gives vbcx_plan_image of that
    array byte for byte (and back): the recording plans' lane writer copied tags where the builder narrows, and the
    lane value regions are in the recorder's narrow list."""
    B, direction, env, w = case(name)
    set_env(monkeypatch, {**env, "VBC_TARGET_RANGES_L": "8"})
    nval = int(B.ofs[-1]) - 1
    v0 = np.ascontiguousarray(B.val.astype(np.float64))
    v1 = second_values(B)
    img0, img1 = image(B, direction | ND80, facts), image(B, direction | ND80, facts, v1)
    mp, ch = value_map(B, v0, direction | ND80 | NUPD, facts)
    print(name, "image", img0.size, "entries", mp.size, "chunks", ch.size, "stored sizes", sorted(set(ch["vsz"].tolist())))
    assert set(ch["vsz"].tolist()) == {4}  # the one bucket is a narrow lane bucket
    assert img0.size == img1.size and not np.array_equal(img0, img1)
    assert np.array_equal(apply_map(img0, mp, ch, v1), img1)
    assert np.array_equal(apply_map(img1, mp, ch, B.val), img0)
    real = mp[(mp != L.VBCX_MAP_SKIP) & (mp != L.VBCX_MAP_ZERO)] & 0x7FFFFFFF
    assert real.max() < nval and np.unique(real).size == nval
    assert (ch["dst"] * 4 % 16 == 0).all()  # whole float quads: the regions start on 256-B reservations
    assert np.array_equal(image(B, direction | ND80 | NUPD, facts), img0)  # 0x200 changes no image byte
    # under 0x580 | 0x200 the same bucket is wide: Float64 chunks
    mpw, chw = value_map(B, v0, direction | N580 | NUPD, facts)
    assert set(chw["vsz"].tolist()) == {0}


# ---- the sanitized program ---------------------------------------------------------------------------------------------

def test_sanitized_planner_program(tmp_path, facts, monkeypatch):
    """tests/host/narrow_streams_asan.cpp: the planner's and the value map's host code under AddressSanitizer and UBSan,
    as a program of its own (no preloaded runtime), plans the B'x and the forward lane case with 0xD80 and 0xF80 and
    returns the image and the map the library itself gives."""
    exe = tmp_path / "narrow_streams_asan"
    src = L.PKG_DIR.parent / "tests" / "host" / "narrow_streams_asan.cpp"
    r = subprocess.run(["make", "-C", str(L.PKG_DIR), "-j8", f"PLAN_ASAN={exe}", f"ASAN_BUILD={tmp_path / 'obj'}",
                        f"PLAN_ASAN_SRC={src}", "plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("bx_w3_r3", "forward"):
        B, direction, env, w = case(name)
        env = {**env, "VBC_TARGET_RANGES_L": "8"}
        for k in ("VBC_PLANAR_PAIR", "VBC_TARGET_RANGES_L"):
            monkeypatch.delenv(k, raising=False)
        set_env(monkeypatch, env)
        val = np.ascontiguousarray(B.val.astype(np.float64))
        head = np.array([B.m, B.n, 0, B.W, 0, len(B.Phi), len(B.idx), len(val), L.VBC_F64, direction, 8], np.int64)
        parts = [head.tobytes(), bytes(facts)]
        parts += [np.ascontiguousarray(a, np.int64).tobytes() for a in (B.Phi.spl, B.pos, B.idx, B.ofs)] + [val.tobytes()]
        (tmp_path / f"{name}.case").write_bytes(b"".join(parts))
        out = [tmp_path / f"{name}.{s}" for s in ("d80", "map", "chunks")]
        clean = {k: v for k, v in os.environ.items() if not k.startswith("VBC_") and k != "LD_PRELOAD"}
        r = subprocess.run([str(exe), str(tmp_path / f"{name}.case")] + [str(p) for p in out], env={**clean, **env},
                           capture_output=True, text=True)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        iD80 = image(B, direction | ND80, facts)
        assert iD80.size < image(B, direction | N580, facts).size, name
        assert np.array_equal(np.frombuffer(out[0].read_bytes(), np.uint8), iD80), name
        mp, ch = value_map(B, val, direction | ND80 | NUPD, facts)
        assert np.array_equal(np.frombuffer(out[1].read_bytes(), np.uint32), mp), name
        assert np.array_equal(np.frombuffer(out[2].read_bytes(), CHUNK), ch), name
