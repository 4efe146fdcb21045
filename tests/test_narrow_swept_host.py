"""Narrow row-swept storage (vbc.h VBC_CREATE_NARROW_SWEPT, 0x1000, valid only with VBC_CREATE_NARROW_VALUES), the
parts that need no GPU: the header, the refusals of the C ABI (decided before any device work), the Python rules of
`B.narrow = "swept"`, what the flag does to the arena image the planner builds (vbcx_plan_image under the device facts
recorded in tests/golden/plan_images.json, with VBC_SWEEP=1), the value map of a 0x1280 handle (vbcx_value_map; the
method of tests/test_narrow_update_host.py), and the planner under AddressSanitizer / UBSan as a program of its own
(tests/host/narrow_swept_asan.cpp).

The arrangement: a narrow swept bucket's value region holds the wide one's steps * 64 * w values as floats in the
same order -- the row of lane l of step s at float offset (s * 64 + l) * w -- so the region of the 0x1080 image is the
0x80 image's region narrowed element by element, at the same linear index; padding slots are zero in both."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from sparsematrixvbcs_amd import _lib as L
from tests.test_narrow_host import Recorder, mat1d, mat2d
from tests.test_narrow_pairs_host import al256, all_ex_creates, csc, image, refused, second_values, set_env
from tests.test_narrow_streams_host import distinct
from tests.test_narrow_update_host import CHUNK, apply_map, value_map
from tests.test_plan_host import GOLDEN, facts_from

HEADER = L.PKG_DIR.parent / "include" / "vbc.h"
NARROW, PLANAR, NUPD = L.VBC_CREATE_NARROW_VALUES, L.VBC_CREATE_NARROW_PLANAR, L.VBC_CREATE_NARROW_UPDATABLE
PAIRS, STREAMS, SWEPT = L.VBC_CREATE_NARROW_PAIRS, L.VBC_CREATE_NARROW_STREAMS, 0x1000
N1080, N1D80 = NARROW | SWEPT, NARROW | PLANAR | PAIRS | STREAMS | SWEPT
T, F = L.VBC_CREATE_TRANSPOSED, L.VBC_CREATE_FORWARD
# 0x1000 without 0x80, with every combination of the bits between
WITHOUT_80 = [SWEPT | s for s in (0, PLANAR, PAIRS, STREAMS, PLANAR | PAIRS, PLANAR | PAIRS | STREAMS)]
# 0x1000 with 0x80 and any of the bits between (incomplete ladders included: 0x1000 needs none of them)
VALID = [N1080, N1080 | PLANAR, N1080 | PLANAR | PAIRS, N1D80]


def names_swept():
    msg = L.last_error()
    assert "VBC_CREATE_NARROW_SWEPT" in msg, msg
    return True


# ---- header and refusals ------------------------------------------------------------------------------------------

def test_flag_and_header():
    assert getattr(L, "VBC_CREATE_NARROW_SWEPT", None) == SWEPT == 0x1000
    text = HEADER.read_text()
    assert re.search(r"#define\s+VBC_CREATE_NARROW_SWEPT\s+0x1000u\b", text)
    entry = text[text.index("#define VBC_CREATE_NARROW_SWEPT"): text.index("/* mul flags */")]
    entry = re.sub(r"\s+", " ", entry)
    for word in ("spmv_sweep", "bit 20 / 21", "VBC_CREATE_NARROW_UPDATABLE", "bit-identical", "(s * 64 + l) * w",
                 "16-B aligned", "VBC_CREATE_NARROW_VALUES"):
        assert word in entry, word
    info = text[text.index("typedef struct vbc_info"):]
    assert "bit 20" in info and "bit 21" in info and "VBC_CREATE_NARROW_SWEPT" in info
    head = re.sub(r"\s+", " ", text[: text.index("#define VBC_VERSION")])
    assert "VBC_CREATE_NARROW_SWEPT: bits 20 / 21" in head  # the version comment
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", text).group(1)) == 30400
    assert int(re.search(r"#define\s+VBC_INFO_SIZE\s+(\d+)", text).group(1)) == L.VBC_INFO_SIZE == 152
    assert C.sizeof(L.vbc_info) == 152
    assert L.lib().vbc_version() == 30400


@pytest.mark.parametrize("upd", [0, NUPD])
@pytest.mark.parametrize("bits", WITHOUT_80)
def test_refused_without_narrow_values(bits, upd):
    for st, h in all_ex_creates(T | bits | upd):
        assert refused(st, h) and names_swept()


@pytest.mark.parametrize("bits", [N1080, N1080 | NUPD, N1D80, N1D80 | NUPD])
def test_refused_together_with_updatable(bits):
    for st, h in all_ex_creates(T | bits | L.VBC_CREATE_UPDATABLE):  # 0x20
        assert refused(st, h) and names_swept()


@pytest.mark.parametrize("val_dt,compute_dt,np_dt", [(L.VBC_F64, L.VBC_F64, np.float64), (L.VBC_F32, L.VBC_F32, np.float32),
                                                     (L.VBC_F64, L.VBC_F32, np.float64), (L.VBC_I32, L.VBC_F64, np.int32),
                                                     (L.VBC_BOOL, L.VBC_F64, np.bool_)])
@pytest.mark.parametrize("bits", [N1080, N1080 | NUPD, N1D80])
def test_refused_for_any_other_eltype_pair(val_dt, compute_dt, np_dt, bits):
    for st, h in all_ex_creates(T | bits, val_dt, compute_dt, np_dt):
        assert refused(st, h) and names_swept()


@pytest.mark.parametrize("bits", [SWEPT, N1080, N1080 | NUPD, N1D80])
def test_refused_on_the_creates_without_types(bits):
    f = T | bits
    for dt, np_dt in ((L.VBC_F64, np.float64), (L.VBC_F32, np.float32)):
        B = mat1d(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc1d_create(C.byref(h), B.m, B.n, B.W, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                  B.idx.ctypes.data, B.ofs.ctypes.data, B.val.ctypes.data, len(B.val), dt, 0, f)
        assert refused(st, h) and names_swept()
        B2 = mat2d(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc2d_create(C.byref(h), B2.m, B2.n, B2.U, B2.W, len(B2.Pi), B2.Pi.spl.ctypes.data, len(B2.Phi),
                                  B2.Phi.spl.ctypes.data, B2.pos.ctypes.data, B2.idx.ctypes.data, B2.ofs.ctypes.data,
                                  B2.val.ctypes.data, len(B2.val), dt, 0, f)
        assert refused(st, h) and names_swept()
        Cm = csc(np_dt)
        h = C.c_void_p()
        st = L.lib().vbc_csc_create(C.byref(h), Cm.m, Cm.n, Cm.colptr.ctypes.data, Cm.rowval.ctypes.data,
                                    Cm.nzval.ctypes.data, dt, 0, f)
        assert refused(st, h) and names_swept()


@pytest.mark.parametrize("bits", [SWEPT, N1080, N1080 | NUPD, N1D80])
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
    assert refused(st, h) and names_swept()
    B2 = mat2d()
    h = C.c_void_p()
    st = L.lib().vbc2d_create_sharded(C.byref(h), B2.m, B2.n, B2.U, B2.W, len(B2.Pi), B2.Pi.spl.ctypes.data, len(B2.Phi),
                                      B2.Phi.spl.ctypes.data, B2.pos.ctypes.data, B2.idx.ctypes.data, B2.ofs.ctypes.data,
                                      B2.val.ctypes.data, len(B2.val), C.byref(t), 2, devs, L.VBC_SPLIT_STRIPES, f)
    assert refused(st, h) and names_swept()


# ---- the Python rule ------------------------------------------------------------------------------------------------

def test_python_narrow_swept_flags():
    every = N1D80 | NUPD | L.VBC_CREATE_UPDATABLE
    for updatable, want in ((False, N1D80), ("narrow", N1D80 | NUPD)):
        assert want in (0x1D80, 0x1F80)
        for B in (mat1d(), mat2d(), csc(np.float32)):
            B.narrow = "swept"
            B.updatable = updatable
            rec = Recorder(B)
            B.handle(0, True, compute=L.VBC_F64)
            assert rec.flags[0][0] & every == want, (updatable, type(B))
            B._handles.h.clear()  # nothing was created
    for narrow, want in ((True, NARROW), ("planar", NARROW | PLANAR), ("pairs", NARROW | PLANAR | PAIRS),
                         ("streams", NARROW | PLANAR | PAIRS | STREAMS)):  # the older values pass what they passed
        B = mat1d()
        B.narrow = narrow
        rec = Recorder(B)
        B.handle(0, True, compute=L.VBC_F64)
        assert rec.flags[0][0] & every == want
        B._handles.h.clear()
    for dtype, compute in ((np.float32, L.VBC_F32), (np.float32, None), (np.float64, L.VBC_F64)):
        B = mat1d(dtype)  # any other eltype pair: the attribute is ignored
        B.narrow = "swept"
        rec = Recorder(B)
        B.handle(0, True, compute=compute)
        assert not rec.flags[0][0] & N1D80
        B._handles.h.clear()
    B = mat1d()
    B.narrow = "swept"
    rec = Recorder(B)  # the matrix-core panel layouts store no swept bucket
    B.handle(0, True, multi=True, compute=L.VBC_F64)
    assert not rec.flags[0][0] & N1D80
    B._handles.h.clear()


@pytest.mark.parametrize("bad", ["sweep", "Swept", "sweeps", 0x1000, 0x1080, ("swept",)])
def test_python_any_other_value_is_still_a_value_error(bad):
    B = mat1d()
    B.narrow = bad
    rec = Recorder(B)
    with pytest.raises(ValueError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_swept_with_updatable_true_is_an_argument_error():
    B = mat1d()
    B.narrow = "swept"
    B.updatable = True
    rec = Recorder(B)
    with pytest.raises(L.ArgumentError):
        B.handle(0, True, compute=L.VBC_F64)
    assert not rec.flags


def test_python_multi_gpu_classes_refuse_narrow_swept():
    B = mat1d()
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0], narrow="swept")
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2, narrow="swept")
    B.narrow = "swept"
    with pytest.raises(L.ArgumentError):
        V.distributed.MultiGPUSparseMatrix1DVBC(B, devices=[0, 0])
    with pytest.raises(L.ArgumentError):
        V.distributed.ShardedSparseMatrix1DVBC(B, 0, 2)


def test_julia_shim_mirrors_the_flag():
    text = (L.PKG_DIR / "julia" / "SparseMatrixVBCsHIP.jl").read_text()
    assert re.search(r"const VBC_CREATE_NARROW_SWEPT = Cuint\(0x1000\)", text)
    assert "narrow === :swept" in text


# ---- the planner's image (no device) ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def facts():
    return facts_from(json.loads(GOLDEN.read_text())["facts"])


# name -> (matrix, create direction, swept buckets): 60 stripes over m = 300 rows, ~700 stored rows; the mixed case
# has one bucket per width, and 8 KB tiles of 1024 / w stripes
def case(name):
    widths, direction = {"bx_w4": (4, T), "fwd_w4": (4, F), "bx_mixed": (np.arange(60) % 8 + 1, T),
                         "fwd_mixed": (np.arange(60) % 8 + 1, F)}[name]
    B = distinct(V.synthetic.vbr_1dvbc(300, 60, 700, widths, W=8, dtype=np.float32, seed=7))
    return B, direction, 1 if np.isscalar(widths) else 8


CASES = ("bx_w4", "fwd_w4", "bx_mixed", "fwd_mixed")
SWEEP = {"VBC_SWEEP": "1", "VBC_SWEEP_TILE": "8"}


def swept_regions(wide, narrow, pa=0, pb=0):
    """[(offset in `wide`, offset in `narrow`, values)] of the value regions in which the two images differ: the walk
    takes equal bytes up to the first difference, which lies in a region that starts on a 256-B reservation, holds a
    multiple of 64 doubles in `wide` and as many floats in `narrow`, each float the double narrowed at the same
    index, with zero alignment padding behind it in both, and is followed by equal bytes again (the next
    reservation).  The walk must use up both images, so every byte is either equal or inside such a region; a
    candidate length after which the rest of the walk fails is dropped for the next shorter one.  None: no such walk."""
    n = min(wide.size - pa, narrow.size - pb)
    d = np.flatnonzero(wide[pa: pa + n] != narrow[pb: pb + n])
    if d.size == 0:
        return [] if wide.size - pa == narrow.size - pb else None
    o = int(d[0]) // 256 * 256
    oa, ob = pa + o, pb + o
    fits = []
    for nv in range(64, (wide.size - oa) // 8 + 1, 64):
        na, nb = oa + al256(nv * 8), ob + al256(nv * 4)
        if na > wide.size or nb > narrow.size:
            break
        v64 = wide[oa: oa + nv * 8].view(np.float64)
        v32 = narrow[ob: ob + nv * 4].view(np.float32)
        if not np.array_equal(v64[-64:].astype(np.float32).view(np.uint32), v32[-64:].view(np.uint32)):
            break  # (the candidates grow by 64 values: the earlier ones were compared already)
        if not wide[oa + nv * 8: na].any() and not narrow[ob + nv * 4: nb].any():
            fits.append(nv)
    for nv in reversed(fits):  # the longest first: a region is never reported in pieces
        rest = swept_regions(wide, narrow, oa + al256(nv * 8), ob + al256(nv * 4))
        if rest is not None:
            return [(oa, ob, nv)] + rest
    return None


@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("name", CASES)
def test_image_differs_in_one_value_region_per_swept_bucket(name, pack, facts, monkeypatch):
    B, direction, buckets = case(name)
    set_env(monkeypatch, {**SWEEP, "VBC_SWEEP_PACK": pack})
    nval = int(B.ofs[-1]) - 1
    wide, i80, i1080 = image(B, direction, facts), image(B, direction | NARROW, facts), image(B, direction | N1080, facts)
    assert np.array_equal(wide, i80)  # 0x80 alone: the swept buckets stay wide (no slotted bucket here)
    regs = swept_regions(i80, i1080)  # (every byte outside the regions is equal)
    assert regs is not None
    print(name, pack, "sizes", i80.size, i1080.size, "regions", regs, "nval", nval)
    assert len(regs) == buckets
    stored32, stored64 = [], []
    for oa, ob, nv in regs:
        assert ob % 16 == 0
        v64 = i80[oa: oa + nv * 8].view(np.float64)
        v32 = i1080[ob: ob + nv * 4].view(np.float32)
        # row by row -- lane l of step s, column c at (s * 64 + l) * w + c in both -- the floats are the doubles narrowed
        assert np.array_equal(v64.astype(np.float32).view(np.uint32), v32.view(np.uint32))
        assert np.array_equal(v64 == 0, v32 == 0)  # padding slots are zero, in the same places
        stored32.append(v32[v32 != 0])
        stored64.append(v64[v64 != 0])
    stored32 = np.concatenate(stored32)
    assert stored32.size == nval and np.array_equal(np.sort(stored32), np.sort(B.val[:nval]))  # the inputs, each once
    assert np.concatenate(stored64).size == nval
    assert i80.size - i1080.size >= 4 * nval - 256 * buckets
    # the bits between change nothing here (no planar bucket): 0x1D80 gives the 0x1080 image
    assert np.array_equal(image(B, direction | N1D80, facts), i1080)


def test_rows_keep_step_lane_column(facts, monkeypatch):
    """One width-4 bucket, one tile: the first region value rows are the stripes' first rows in ascending x row, lane
    l of step 0 at floats 4 l .. 4 l + 3, as in the wide image."""
    B, direction, _ = case("bx_w4")
    set_env(monkeypatch, {**SWEEP, "VBC_SWEEP_PACK": "0"})
    i80, i1080 = image(B, direction | NARROW, facts), image(B, direction | N1080, facts)
    (oa, ob, nv), = swept_regions(i80, i1080)
    v32 = i1080[ob: ob + nv * 4].view(np.float32).reshape(-1, 64, 4)
    v64 = i80[oa: oa + nv * 8].view(np.float64).reshape(-1, 64, 4)
    # the input rows: stripe l's row r is val[ofs[l] - 1 + 4 r : + 4]
    rows = {tuple(B.val[o - 1 + 4 * r: o + 3 + 4 * r]) for l, o in enumerate(B.ofs[:-1]) for r in range(B.pos[l + 1] - B.pos[l])}
    live = v32[..., 0] != 0
    assert live.sum() == len(rows) == int(B.pos[-1]) - 1
    for s, l in zip(*np.nonzero(live)):
        assert tuple(v32[s, l]) in rows and tuple(v64[s, l].astype(np.float32)) == tuple(v32[s, l])
    assert live[:-1].all() or not live[-1].all()  # only a tile's last step is padded


def test_special_values_keep_their_bits(facts, monkeypatch):
    B, direction, _ = case("bx_mixed")
    set_env(monkeypatch, {**SWEEP, "VBC_SWEEP_PACK": "1"})
    fi = np.finfo(np.float32)
    v = B.val.copy()
    special = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x7F7FFFFF],
                       np.uint32).view(np.float32)  # NaNs with payloads, -0, +-Inf, subnormals, FLT_MAX
    v[10: 10 + special.size] = special
    assert np.isnan(v[10]) and v[17] == fi.max
    i80, i1080 = image(B, direction | NARROW, facts, v), image(B, direction | N1080, facts, v)
    assert i1080.size < i80.size
    nval = int(B.ofs[-1]) - 1
    # the layout does not depend on the values: the regions are those of the distinct values
    regs = swept_regions(image(B, direction | NARROW, facts), image(B, direction | N1080, facts))
    v32 = np.concatenate([i1080[ob: ob + nv * 4].view(np.uint32) for _, ob, nv in regs])
    for bits in special.view(np.uint32):
        assert (v32 == bits).sum() >= 1, hex(int(bits))
    assert np.array_equal(np.sort(v32[v32 != 0]), np.sort(v[:nval].view(np.uint32)))  # every input's bits, nothing else


def test_plan_image_and_value_map_refuse_the_same_combinations(facts):
    B = case("bx_w4")[0]
    v = np.ascontiguousarray(B.val.astype(np.float64))
    v32 = np.ascontiguousarray(B.val)
    n, ne, nc = C.c_size_t(), C.c_int64(), C.c_int64()
    for bits, dt, vv in [(b, L.VBC_F64, v) for b in WITHOUT_80] + [(N1080, L.VBC_F32, v32), (N1D80, L.VBC_F32, v32)]:
        st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                     B.idx.ctypes.data, B.ofs.ctypes.data, vv.ctypes.data, len(vv), dt, T | bits,
                                     C.byref(facts), None, 0, C.byref(n))
        assert st == L.VBC_INVALID_ARG and names_swept(), hex(bits)
        st = L.lib().vbcx_value_map(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                    B.idx.ctypes.data, B.ofs.ctypes.data, vv.ctypes.data, len(vv), dt, T | bits,
                                    C.byref(facts), None, 0, C.byref(ne), None, 0, C.byref(nc))
        assert st == L.VBC_INVALID_ARG and names_swept(), hex(bits)
    st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                 B.idx.ctypes.data, B.ofs.ctypes.data, v.ctypes.data, len(v), L.VBC_F64,
                                 T | N1080 | L.VBC_CREATE_UPDATABLE, C.byref(facts), None, 0, C.byref(n))
    assert st == L.VBC_INVALID_ARG  # (as for every flag set: the image has no updatable form)


# ---- the value map of a 0x1280 handle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("name", CASES)
def test_map_round_trip(name, pack, facts, monkeypatch):
    """The map of the 0x1280 handle, applied in numpy to a second float32 value array, gives vbcx_plan_image of that
    array byte for byte (and back): the recording plans' swept writer copied tags where the builder narrows, and the
    swept value regions are in the recorder's narrow list."""
    B, direction, buckets = case(name)
    set_env(monkeypatch, {**SWEEP, "VBC_SWEEP_PACK": pack})
    nval = int(B.ofs[-1]) - 1
    v0 = np.ascontiguousarray(B.val.astype(np.float64))
    v1 = second_values(B)
    img0, img1 = image(B, direction | N1080, facts), image(B, direction | N1080, facts, v1)
    mp, ch = value_map(B, v0, direction | N1080 | NUPD, facts)
    print(name, "image", img0.size, "entries", mp.size, "chunks", ch.size, "stored sizes", sorted(set(ch["vsz"].tolist())))
    assert set(ch["vsz"].tolist()) == {4}  # every bucket is a narrow swept bucket
    assert img0.size == img1.size and not np.array_equal(img0, img1)
    assert np.array_equal(apply_map(img0, mp, ch, v1), img1)
    assert np.array_equal(apply_map(img1, mp, ch, B.val), img0)
    real = mp[(mp != L.VBCX_MAP_SKIP) & (mp != L.VBCX_MAP_ZERO)] & 0x7FFFFFFF
    assert real.max() < nval and np.unique(real).size == nval
    assert (ch["dst"] * 4 % 16 == 0).all()  # whole float quads: the regions start on 256-B reservations
    assert np.array_equal(image(B, direction | N1080 | NUPD, facts), img0)  # 0x200 changes no image byte
    # under 0x80 | 0x200 the same buckets are wide: Float64 chunks
    mpw, chw = value_map(B, v0, direction | NARROW | NUPD, facts)
    assert set(chw["vsz"].tolist()) == {0}


# ---- the sanitized program ---------------------------------------------------------------------------------------------

def test_sanitized_planner_program(tmp_path, facts, monkeypatch):
    """tests/host/narrow_swept_asan.cpp: the planner's and the value map's host code under AddressSanitizer and UBSan,
    as a program of its own (no preloaded runtime), plans the B'x and the forward swept case with 0x1080 and 0x1280 and
    returns the image and the map the library itself gives."""
    exe = tmp_path / "narrow_swept_asan"
    src = L.PKG_DIR.parent / "tests" / "host" / "narrow_swept_asan.cpp"
    r = subprocess.run(["make", "-C", str(L.PKG_DIR), "-j8", f"PLAN_ASAN={exe}", f"ASAN_BUILD={tmp_path / 'obj'}",
                        f"PLAN_ASAN_SRC={src}", "plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = {**SWEEP, "VBC_SWEEP_PACK": "1"}
    set_env(monkeypatch, env)
    for name in ("bx_mixed", "fwd_w4"):
        B, direction, _ = case(name)
        val = np.ascontiguousarray(B.val.astype(np.float64))
        head = np.array([B.m, B.n, 0, B.W, 0, len(B.Phi), len(B.idx), len(val), L.VBC_F64, direction, 8], np.int64)
        parts = [head.tobytes(), bytes(facts)]
        parts += [np.ascontiguousarray(a, np.int64).tobytes() for a in (B.Phi.spl, B.pos, B.idx, B.ofs)] + [val.tobytes()]
        (tmp_path / f"{name}.case").write_bytes(b"".join(parts))
        out = [tmp_path / f"{name}.{s}" for s in ("1080", "map", "chunks")]
        clean = {k: v for k, v in os.environ.items() if not k.startswith("VBC_") and k != "LD_PRELOAD"}
        r = subprocess.run([str(exe), str(tmp_path / f"{name}.case")] + [str(p) for p in out], env={**clean, **env},
                           capture_output=True, text=True)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        i1080 = image(B, direction | N1080, facts)
        assert i1080.size < image(B, direction | NARROW, facts).size, name
        assert np.array_equal(np.frombuffer(out[0].read_bytes(), np.uint8), i1080), name
        mp, ch = value_map(B, val, direction | N1080 | NUPD, facts)
        assert np.array_equal(np.frombuffer(out[1].read_bytes(), np.uint32), mp), name
        assert np.array_equal(np.frombuffer(out[2].read_bytes(), CHUNK), ch), name
