"""The layout planner on the host (vbc_host.h vbcx_plan_image): no GPU needed.

Golden comparison: the arena image of every case of CASES, planned under the device facts recorded in
tests/golden/plan_images.json, has the SHA-256 recorded there.  The digests were taken on an MI355X from the
arena the library uploaded before the planner was split from the device part of a create, so they pin the
planner to that layout byte for byte; tests/test_gpu_plan.py checks that the recorded facts are the device's.

Recording property: planned with val all zero and with val holding the tag i + 1 in element i, the images have
one length and differ only inside value slots -- what VBC_CREATE_UPDATABLE's value map is built from.

Host-only property: the objects of the planner's translation units (csrc/vbc_plan*.hip) leave no HIP runtime
function and no getenv undefined, i.e. they call none.
"""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from sparsematrixvbcs_amd import _lib as L

GOLDEN = Path(__file__).parent / "golden" / "plan_images.json"
T, F, M, SERIAL, MF, NARROW = (L.VBC_CREATE_TRANSPOSED, L.VBC_CREATE_FORWARD, L.VBC_CREATE_MULTI, L.VBC_CREATE_SERIAL,
                               L.VBC_CREATE_MULTI_FORWARD, L.VBC_CREATE_NARROW_VALUES)
F64, F32 = np.float64, np.float32

# No fused small split, no split product, no lane streams: the bucket layouts a large matrix would get.
PLAIN = {"VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_LANES": "0"}


def mixed(dt, seed=3):
    return V.synthetic.vbr_1dvbc(60, 12, 90, np.arange(12) % 4 + 1, W=4, dtype=dt, seed=seed)


def uniform(dt, w, m=300, L_=150, q=4000):
    return V.synthetic.vbr_1dvbc(m, L_, q, w, W=8, dtype=dt, seed=5)


def ragged(dt, w):  # stripe lengths from 0 to ~60 rows: the natural order pads far beyond VBC_SLOTS_PAD
    B = V.synthetic.vbr_1dvbc(400, 200, 3000, w, W=8, dtype=dt, seed=11)
    keep = np.concatenate([np.arange(B.pos[l] - 1, B.pos[l] - 1 + (B.pos[l + 1] - B.pos[l]) * (l % 7) // 6)
                           for l in range(len(B.Phi))]).astype(np.int64)
    cnt = np.array([(B.pos[l + 1] - B.pos[l]) * (l % 7) // 6 for l in range(len(B.Phi))], np.int64)
    pos = np.concatenate([[1], 1 + np.cumsum(cnt)]).astype(np.int64)
    ofs = np.concatenate([[1], 1 + np.cumsum(cnt * w)]).astype(np.int64)
    val = np.arange(1, int(ofs[-1]), dtype=dt) / 7
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, pos, B.idx[keep], ofs, val)


def mesh(dt, dof=3, N=14):
    return V.synthetic.fe_grid_2d(N, dof=dof, W=8, dtype=dt, seed=7)


def dominant(dt):  # 700 3-wide stripes and a few 1- and 2-wide ones: one width holds > 80 % of the chunks
    w = np.full(720, 3)
    w[::60] = 1
    w[30::90] = 2
    return V.synthetic.vbr_1dvbc(500, 720, 9000, w, W=8, dtype=dt, seed=13)


def pieces(dt):  # 2-wide stripes and a few 4-wide ones (column pieces: each runs as two 2-wide stripes)
    w = np.full(100, 2)
    w[::10] = 4
    return V.synthetic.vbr_1dvbc(200, 100, 1500, w, W=8, dtype=dt, seed=17)


def blocks(dt, u=4, w=4):
    return V.synthetic.vbr_2d(40, 30, 300, u, w, dtype=dt, seed=19)


def integers(_):
    B = mixed(F64)
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, (B.val * 100).astype(np.int64))


# name: (matrix, eltype, flags, environment)
CASES = {
    "merge_f64": (mixed, F64, T | F, {"VBC_SLOTS": "0", "VBC_FWD_T": "0"}),
    "merge_f32": (mixed, F32, T | F, {"VBC_SLOTS": "0", "VBC_FWD_T": "0"}),
    "slots_key32_f64": (lambda dt: uniform(dt, 2), F64, T | F, {"VBC_SLOTS": "1", "VBC_SLOT_KEYS16": "0", **PLAIN}),
    "slots_key16_f32": (lambda dt: uniform(dt, 2), F32, T | F, {"VBC_SLOTS": "1", "VBC_SLOT_KEYS16": "2", **PLAIN}),
    "slots_key16_nodedup_f64": (lambda dt: uniform(dt, 1), F64, T | F,
                                {"VBC_SLOTS": "1", "VBC_SLOT_KEYS16": "2", "VBC_SLOT_DEDUP": "0", **PLAIN}),
    "slots_sorted_f32": (lambda dt: ragged(dt, 2), F32, T, {"VBC_SLOTS": "1", "VBC_SLOTS_SORT": "2", **PLAIN}),
    "planar_f64": (lambda dt: mesh(dt, 3), F64, T, {"VBC_PLANAR_PAIR": "0", **PLAIN}),
    "planar_f32": (lambda dt: uniform(dt, 5), F32, T, {"VBC_SLOTS": "1", **PLAIN}),
    "planar_pair_f64": (lambda dt: mesh(dt, 3), F64, T, {"VBC_PLANAR_PAIR": "2", **PLAIN}),
    "planar_masked_f64": (lambda dt: ragged(dt, 5), F64, T, {"VBC_SLOTS": "1", "VBC_PLANAR_MASK": "1", **PLAIN}),
    "planar_masked_pair_f64": (lambda dt: mesh(dt, 3, 9), F64, T,
                               {"VBC_SLOTS": "1", "VBC_PLANAR_MASK": "1", "VBC_PLANAR_PAIR": "2", "VBC_SLOTS_SORT": "2",
                                **PLAIN}),
    "planar_sorted_f32": (lambda dt: ragged(dt, 5), F32, T, {"VBC_SLOTS": "1", "VBC_PLANAR_MASK": "0", **PLAIN}),
    "planar_split_f64": (lambda dt: mesh(dt, 3), F64, T, {"VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "4"}),
    "lanes_f64": (lambda dt: mesh(dt, 3), F64, T, {"VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_LANES": "1"}),
    "lanes_f32": (lambda dt: mesh(dt, 3), F32, T, {"VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_LANES": "1"}),
    "lanes_pair_f64": (lambda dt: mesh(dt, 3), F64, T, {"VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0",
                                                       "VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "1"}),
    "sweep_packed_f64": (lambda dt: uniform(dt, 4, 3000, 200, 3000), F64, T | F, {"VBC_SWEEP": "1", "VBC_SWEEP_PACK": "1"}),
    "sweep_unpacked_f32": (lambda dt: uniform(dt, 4, 3000, 200, 3000), F32, T | F, {"VBC_SWEEP": "1", "VBC_SWEEP_PACK": "0"}),
    "fused_f64": (mixed, F64, T, {}),
    "fused_f32": (mixed, F32, T, {}),
    "fused_mesh_f64": (lambda dt: mesh(dt, 3, 9), F64, T, {"VBC_SMALL_FUSE": "2"}),
    "fused_side_f64": (dominant, F64, T, {"VBC_SIDE_FUSE": "1"}),
    "fused_noside_f32": (dominant, F32, T, {"VBC_SIDE_FUSE": "0"}),
    "fused_ksplit_f64": (lambda dt: ragged(dt, 3), F64, T, {"VBC_SMALL_FUSE": "2", "VBC_KSPLIT": "0.5"}),
    "pieces_f64": (pieces, F64, T, {}),
    "pieces_off_f32": (pieces, F32, T, {"VBC_COLSPLIT": "0"}),
    "fwd_runs_f64": (lambda dt: mesh(dt, 3), F64, F, {"VBC_FWD_T": "0", "VBC_PLANAR_PAIR": "0", "VBC_PLANAR_LANES": "0"}),
    "fwd_runs_f32": (lambda dt: mesh(dt, 2), F32, F, {"VBC_FWD_T": "0", "VBC_PLANAR_LANES": "0"}),
    "fwd_lanes_f64": (lambda dt: mesh(dt, 3), F64, F, {"VBC_FWD_T": "0", "VBC_PLANAR_PAIR": "0", "VBC_PLANAR_LANES": "1"}),
    "fwd_pair_f64": (lambda dt: mesh(dt, 3), F64, F, {"VBC_FWD_T": "0", "VBC_PLANAR_PAIR": "2", "VBC_PLANAR_LANES": "0",
                                                     "VBC_PLANAR_SPLIT": "0"}),
    "fwd_buckets_f32": (mixed, F32, F, {"VBC_FWD_T": "0"}),
    "fwd_via_t_f64": (mixed, F64, T | F, {"VBC_FWD_T": "2"}),
    "fwd_via_t_f32": (mixed, F32, F, {"VBC_FWD_T": "2"}),
    "panel_f32": (lambda dt: blocks(dt, 8, 8), F32, M, {"VBC_PANEL_TILES": "0"}),
    "panel_f64": (lambda dt: blocks(dt, 4, 4), F64, M, {"VBC_PANEL_TILES": "0"}),
    "tiles_f32": (lambda dt: blocks(dt, 4, 4), F32, M, {"VBC_PANEL_TILES": "1"}),
    "tiles_1d_f64": (lambda dt: mesh(dt, 3), F64, M, {"VBC_PANEL_TILES": "1"}),
    "fwd_panel_f32": (lambda dt: blocks(dt, 4, 4), F32, MF | M, {}),
    "fwd_panel_1d_f64": (mixed, F64, MF, {}),
    "serial_f64": (mixed, F64, T | F | SERIAL, {}),
    "serial_mesh_f32": (lambda dt: mesh(dt, 3), F32, T | SERIAL, {}),
    "narrow_f64": (lambda dt: uniform(F32, 2), F64, T | F | NARROW, {"VBC_SLOTS": "1", **PLAIN}),
    "narrow_via_t_f64": (lambda dt: mixed(F32), F64, T | F | NARROW, {"VBC_SLOTS": "1", "VBC_FWD_T": "2"}),
    "int64": (integers, np.int64, T | F, {}),
}
RECORDING = ("fused_f64", "fwd_via_t_f32", "fwd_panel_f32")


def facts_from(d):
    f = L.vbcx_facts()
    f.cus = d["cus"]
    for name, _ in L.vbcx_facts._fields_[1:]:
        arr = np.frombuffer(getattr(f, name), dtype=np.int32)
        arr[:] = np.asarray(d[name], np.int32).reshape(-1)
    return f


def facts_dict(f):
    d = {"cus": int(f.cus)}
    for name, _ in L.vbcx_facts._fields_[1:]:
        d[name] = np.ctypeslib.as_array(getattr(f, name)).tolist()
    return d


def matrix_of(name):
    make, dt, flags, env = CASES[name]
    B = make(dt)
    val = np.ascontiguousarray(B.val.astype(dt))  # (narrow: Float32 values widened to the Float64 the handle computes in)
    return B, val, L.dtype_code(np.dtype(dt)), flags, env


def plan_image(B, val, code, flags, facts):
    two_d = hasattr(B, "Pi")
    args = (B.m, B.n, B.U if two_d else 0, B.W, len(B.Pi) if two_d else 0, B.Pi.spl.ctypes.data if two_d else None,
            len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data, B.idx.ctypes.data, B.ofs.ctypes.data, val.ctypes.data,
            len(val), code, flags, C.byref(facts))
    n = C.c_size_t()
    L.check(L.lib().vbcx_plan_image(*args, None, 0, C.byref(n)), "vbcx_plan_image")
    img = np.zeros(n.value, np.uint8)
    L.check(L.lib().vbcx_plan_image(*args, img.ctypes.data, img.size, C.byref(n)), "vbcx_plan_image")
    assert n.value == img.size
    return img


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_is_the_recorded_one(name, golden, monkeypatch):
    B, val, code, flags, env = matrix_of(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    img = plan_image(B, val, code, flags, facts_from(golden["facts"]))
    rec = golden["images"][name]
    assert img.size == rec["bytes"]
    assert hashlib.sha256(img.tobytes()).hexdigest() == rec["sha256"]


def test_size_query_and_short_buffer(golden):
    B, val, code, flags, _ = matrix_of("merge_f64")
    facts = facts_from(golden["facts"])
    img = plan_image(B, val, code, flags, facts)
    n = C.c_size_t()
    short = np.zeros(img.size - 1, np.uint8)
    st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                 B.idx.ctypes.data, B.ofs.ctypes.data, val.ctypes.data, len(val), code, flags,
                                 C.byref(facts), short.ctypes.data, short.size, C.byref(n))
    assert st == L.VBC_INVALID_ARG and n.value == img.size
    # the checks are the creates': a val shorter than ofs says is refused the same way
    st = L.lib().vbcx_plan_image(B.m, B.n, 0, B.W, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                 B.idx.ctypes.data, B.ofs.ctypes.data, val.ctypes.data, 3, code, flags,
                                 C.byref(facts), None, 0, C.byref(n))
    assert st == L.VBC_INVALID_ARG and "val shorter" in L.last_error()


@pytest.mark.parametrize("name", RECORDING)
def test_tagged_and_zero_images_differ_in_value_slots_only(name, golden, monkeypatch):
    B, val, code, flags, env = matrix_of(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    facts = facts_from(golden["facts"])
    esz = val.dtype.itemsize
    nval = len(val)
    tags = np.arange(1, nval + 1, dtype=np.uint64 if esz == 8 else np.uint32).view(val.dtype)  # create_updatable's
    zero = plan_image(B, np.zeros_like(val), code, flags, facts)
    tagged = plan_image(B, tags, code, flags, facts)
    assert zero.size == tagged.size == golden["images"][name]["bytes"]
    words = slice(0, zero.size // esz * esz)
    wt = tagged[words].view(np.uint64 if esz == 8 else np.uint32)
    wz = zero[words].view(wt.dtype)
    assert np.array_equal(tagged[words.stop:], zero[words.stop:])
    diff = wt != wz
    assert diff.any()
    assert (wz[diff] == 0).all()
    assert ((wt[diff] >= 1) & (wt[diff] <= nval)).all()
    assert np.unique(wt[diff]).size == int(B.ofs[-1]) - 1  # every stored value of the matrix is somewhere


PLANNER_OBJECTS = ("vbc_plan.o", "vbc_plan_bins.o", "vbc_plan_panel.o")


def undefined_symbols(obj):
    path = L.PKG_DIR / "build" / obj
    assert path.exists(), f"{path}: the library's build leaves its objects there"
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-u", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [line.split()[-1] for line in r.stdout.splitlines() if line.strip()]


def test_planner_objects_call_no_hip_and_read_no_environment():
    """vbc_plan.h's promise, enforced: the planner's translation units reference no HIP runtime function (hipMalloc,
    hipMemcpy, ...: `hip` and an upper-case letter; the compiler's own __hip* registration symbols are not calls of
    the planner's) and no getenv.  The device part's object does reference one, so the listing can see them."""
    runtime = re.compile(r"hip[A-Z]")
    for obj in PLANNER_OBJECTS:
        syms = undefined_symbols(obj)
        assert syms, obj  # (it calls at least the C++ runtime: an empty listing would be a listing that failed)
        assert [s for s in syms if runtime.match(s)] == [], obj
        assert [s for s in syms if s in ("getenv", "secure_getenv")] == [], obj
    assert [s for s in undefined_symbols("vbc_device.o") if runtime.match(s)]


SANITIZED = ("fused_f64", "slots_key16_f32", "fwd_panel_f32")


def test_sanitized_planner_program(tmp_path, golden):
    """tests/host/plan_asan.cpp: the planner's host code under AddressSanitizer and UBSan, as a program of its own,
    plans three cases of the table (handed over in files) and returns the recorded images."""
    exe = tmp_path / "plan_asan"
    r = subprocess.run(["make", "-C", str(L.PKG_DIR), "-j8", f"PLAN_ASAN={exe}", f"ASAN_BUILD={tmp_path / 'obj'}",
                        "plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    facts = facts_from(golden["facts"])
    for name in SANITIZED:
        B, val, code, flags, env = matrix_of(name)
        two_d = hasattr(B, "Pi")
        head = np.array([B.m, B.n, B.U if two_d else 0, B.W, len(B.Pi) if two_d else 0, len(B.Phi), len(B.idx), len(val),
                         code, flags, val.dtype.itemsize], np.int64)
        parts = [head.tobytes(), bytes(facts)] + ([B.Pi.spl.tobytes()] if two_d else [])
        parts += [np.ascontiguousarray(a, np.int64).tobytes() for a in (B.Phi.spl, B.pos, B.idx, B.ofs)] + [val.tobytes()]
        (tmp_path / f"{name}.case").write_bytes(b"".join(parts))
        r = subprocess.run([str(exe), str(tmp_path / f"{name}.case"), str(tmp_path / f"{name}.img")],
                           env={**os.environ, **env}, capture_output=True, text=True)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        img = (tmp_path / f"{name}.img").read_bytes()
        assert hashlib.sha256(img).hexdigest() == golden["images"][name]["sha256"], name
