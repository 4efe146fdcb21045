"""In-place value updates of narrow handles on the GPU (vbc.h VBC_CREATE_NARROW_UPDATABLE, `B.updatable = "narrow"`
together with `B.narrow`): a float32 matrix on a Float64 handle whose narrow buckets store Float32, rewritten in
place by vbc_update_values from float32 values.

Criterion: created with val0 and updated to val1 (from a device tensor, and in a second instance from a numpy
array), every product is bit-identical to that of a fresh NON-updatable narrow handle created with val1 and to the
wide handle of val1, at (alpha, beta) = (1, 0) and (-0.5, 2); against the oracle (val1.astype(float64)) the
tolerance of tests/test_gpu_parity.py holds.  val1 holds -0.0 and zeros where val0 had values.  The shapes and knob
sets are those of tests/test_narrow_update_host.py's map round trip (about 170 stripes, m = 300), and every case
first checks through vbc_info that it got the layout it means to test."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_parity import TOL64, dev, rel
from tests.test_narrow_update_host import (CHUNK, ORDERS, PLAIN, SLOTTED, blocks_2d, mesh, mixed_widths, ragged,
                                           second_values, small_mixed)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
AB = ((1.0, 0.0), (-0.5, 2.0))
NUPD = L.VBC_CREATE_NARROW_UPDATABLE
ALL_KNOBS = sorted(set(PLAIN) | set(SLOTTED) | {"VBC_SLOTS_SORT", "VBC_PLANAR_MASK", "VBC_SLOT_KEYS16", "VBC_FWD_T"})


def csc_node_blocked():
    """A 3-dof stiffness operand: vbc_csc_create_ex groups a node's columns into one 3-wide stripe (planar bucket)."""
    A = V.synthetic.fe_stiffness_3d(900, 20000, 3, np.float32).tocsc()
    A.sort_indices()
    return V.SparseMatrixCSC(A)


def values_of(B):
    return B.nzval if isinstance(B, V.SparseMatrixCSC) else B.val


def clone(B, val, narrow, updatable):
    """A new matrix object (its own handles: the knobs are read when a handle is created) with B's pattern."""
    if isinstance(B, V.SparseMatrixCSC):
        N = V.SparseMatrixCSC(sp.csc_matrix((val[: len(B.nzval)], B.rowval - 1, B.colptr - 1), shape=(B.m, B.n)))
    elif isinstance(B, V.SparseMatrixVBC):
        N = V.SparseMatrixVBC(B.U, B.W, B.m, B.n, B.Pi, B.Phi, B.pos, B.idx, B.ofs, val.copy())
    else:
        N = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, val.copy())
    if narrow:
        N.narrow = narrow
    if updatable:
        N.updatable = updatable
    return N


def two_value_sets(B):
    """val0 (no zero among the stored values) and val1 (tests/test_narrow_update_host.py second_values)."""
    if not isinstance(B, V.SparseMatrixCSC):
        return B.val.copy(), second_values(B)
    rng = np.random.default_rng(21)  # nzval has no tail pad and the stand-in's values may hold zeros: its own val0
    n = len(B.nzval)

    class Shape:
        val = (rng.uniform(0.25, 1, n) * rng.choice([-1, 1], n)).astype(np.float32)
        ofs = np.array([n + 1])
    return Shape.val, second_values(Shape)


def info64(B, trans):
    return B.info(trans=trans, compute=L.VBC_F64)


def product(B, trans, x, y0, alpha, beta):
    y = dev(y0.copy())
    V.mul_(y, V.adjoint(B) if trans else B, dev(x), alpha, beta)
    return y.cpu().numpy()


def bitwise(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def oracle_product(B, val, trans, x, y0, alpha, beta):
    v = val.astype(np.float64)
    if isinstance(B, V.SparseMatrixCSC):
        A = sp.csc_matrix((v[: len(B.nzval)], B.rowval - 1, B.colptr - 1), shape=(B.m, B.n))
        return alpha * O.trspmv(A, x, np.zeros(B.n)) + beta * y0
    if isinstance(B, V.SparseMatrixVBC):
        R = O.RefVBC(B.m, B.n, B.U, B.W, B.Pi.spl, B.Phi.spl, B.pos, B.idx, B.ofs, v)
    else:
        R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, v)
    return O.mul(R, x, y0.copy(), alpha, beta, trans=trans, ref_semantics=False)


def slotted_t(i):
    assert i["narrow_t"] and not i["narrow_planar_t"] and i["planar_bins"] == 0 and i["slot_bins"] >= 1, i


def slotted_f(i):
    assert i["narrow_f"] and not i["narrow_planar_f"] and not i["planar_mask"] & 256, i


def planar_t(run):
    def check(i):
        assert i["narrow_planar_t"] and i["planar_bins"] >= 1 and i["planar_run"] == run, i
        assert i["planar_split"] == 1 and i["planar_pair"] == 0 and not i["planar_mask"] & ((1 << 2) | (1 << 5)), i
    return check


def planar_f(i):
    assert i["narrow_planar_f"] and i["fwd_run"] == 2 and not i["planar_mask"] & (8 | 16 | 2048), i


def mixed_t(i):  # 0x80 alone: the 2-wide bucket narrow, the planar 3-wide bucket wide
    assert i["narrow_t"] and not i["narrow_planar_t"] and i["planar_bins"] >= 1 and i["slot_bins"] > i["planar_bins"], i


def via_bt(i):
    assert i["planar_mask"] & 256 and i["narrow_f"], i


def csc_t(i):
    assert i["narrow_planar_t"] and i["planar_bins"] == 1 and i["planar_run"] == 3 and i["L"] * 3 == i["n"], i


def two_d(i):
    assert i["K"] > 0 and i["narrow_t"], i


# name: (matrix, B.narrow, knobs, trans, layout check)
CASES = {
    "slotted_bx_w2_keys16": (lambda: ragged(2, 2), True, {**SLOTTED, "VBC_SLOT_KEYS16": "2"}, True, slotted_t),
    "slotted_fwd": (lambda: ragged(2, 2), True, SLOTTED, False, slotted_f),
    "planar_bx_w3": (lambda: ragged(3, 2), "planar", {**PLAIN, "VBC_SLOT_RUNS": "0", **ORDERS["masked"]}, True, planar_t(1)),
    "planar_bx_w4": (lambda: ragged(4, 2), "planar", {**PLAIN, "VBC_SLOT_RUNS": "1", **ORDERS["sorted"]}, True, planar_t(2)),
    "planar_fwd": (mesh, "planar", {k: v for k, v in PLAIN.items() if k != "VBC_SLOTS"}, False, planar_f),
    "mixed": (mixed_widths, True, PLAIN, True, mixed_t),
    "fwd_on_bt": (small_mixed, True, {"VBC_SLOTS": "1", "VBC_FWD_T": "2"}, False, via_bt),
    "csc": (csc_node_blocked, "planar", PLAIN, True, csc_t),
    "two_d": (blocks_2d, True, SLOTTED, True, two_d),
}


@pytest.fixture
def knobs(monkeypatch):
    def use(env):
        for k in ALL_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    yield use
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)


def setup(name, knobs):
    make, narrow, env, trans, check = CASES[name]
    knobs(env)
    B = make()
    v0, v1 = two_value_sets(B)
    assert v0.dtype == v1.dtype == np.float32
    return B, narrow, trans, check, v0, v1


def vectors(B, trans, seed=3):
    rng = np.random.default_rng(seed)
    nx, ny = (B.m, B.n) if trans else (B.n, B.m)
    return rng.uniform(-1, 1, nx), rng.uniform(-1, 1, ny)


@pytest.mark.parametrize("device_val", [True, False], ids=["device_val", "host_val"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_update_against_a_fresh_create(name, device_val, knobs):
    B, narrow, trans, check, v0, v1 = setup(name, knobs)
    Bu = clone(B, v0, narrow, "narrow")
    check(info64(Bu, trans))
    assert all(f & NUPD and not f & L.VBC_CREATE_UPDATABLE for _, f, _ in Bu._handles.h)
    x, y0 = vectors(B, trans)
    old = clone(B, v0, narrow, False)
    assert bitwise(product(Bu, trans, x, y0, 1.0, 0.0), product(old, trans, x, y0, 1.0, 0.0))  # 0x200 changes no product
    Bu.update_values(dev(v1) if device_val else v1)
    fresh, wide = clone(B, v1, narrow, False), clone(B, v1, False, False)
    for alpha, beta in AB:
        got = product(Bu, trans, x, y0, alpha, beta)
        assert bitwise(got, product(fresh, trans, x, y0, alpha, beta)), (alpha, beta)
        assert bitwise(got, product(wide, trans, x, y0, alpha, beta)), (alpha, beta)
        err = rel(got, oracle_product(B, v1, trans, x, y0, alpha, beta))
        print(name, "alpha", alpha, "beta", beta, "rel err", err)
        assert err <= TOL64, (alpha, beta)
    assert np.array_equal(values_of(Bu)[: len(v1)].view(np.uint32), v1.view(np.uint32))  # the host copy, -0.0 included
    for M in (Bu, old, fresh, wide):
        M.release()


def map_counts(B, flags):
    """(entries, chunks) of the value map under this device's facts and the current knobs."""
    facts = L.vbcx_facts()
    L.check(L.lib().vbcx_device_facts(0, C.byref(facts)), "facts")
    val = np.ascontiguousarray(B.val.astype(np.float64))
    two = hasattr(B, "Pi")
    ne, nc = C.c_int64(), C.c_int64()
    L.check(L.lib().vbcx_value_map(B.m, B.n, B.U if two else 0, B.W, len(B.Pi) if two else 0,
                                   B.Pi.spl.ctypes.data if two else None, len(B.Phi), B.Phi.spl.ctypes.data,
                                   B.pos.ctypes.data, B.idx.ctypes.data, B.ofs.ctypes.data, val.ctypes.data, len(val),
                                   L.VBC_F64, flags, C.byref(facts), None, 0, C.byref(ne), None, 0, C.byref(nc)), "map")
    return ne.value, nc.value


@pytest.mark.parametrize("name", ["slotted_bx_w2_keys16", "planar_bx_w3", "planar_fwd", "mixed", "fwd_on_bt", "two_d"])
def test_info_is_the_narrow_handles_but_for_the_map(name, knobs):
    B, narrow, trans, check, v0, _ = setup(name, knobs)
    Bu, Bn = clone(B, v0, narrow, "narrow"), clone(B, v0, narrow, False)
    a, b = info64(Bu, trans), info64(Bn, trans)
    check(a)
    for k in a:
        if k != "device_bytes":
            assert a[k] == b[k], (k, a[k], b[k])
    (flags,) = [f for _, f, _ in Bu._handles.h]
    entries, chunks = map_counts(B, flags)
    nval = int(B.ofs[-1]) - 1
    extra = a["device_bytes"] - b["device_bytes"]
    print(name, "device_bytes", a["device_bytes"], b["device_bytes"], "entries", entries, "chunks", chunks, "nval", nval)
    assert entries >= nval
    # 4 bytes per stored slot and the chunk table (24 bytes each), each rounded up to 256 bytes (the table at least 256)
    assert extra == (4 * entries + 255) // 256 * 256 + max(C.sizeof(L.vbcx_map_chunk) * chunks, 256)
    assert CHUNK.itemsize == C.sizeof(L.vbcx_map_chunk)
    Bu.release()
    Bn.release()


@pytest.mark.parametrize("name", ["mixed", "planar_fwd"])
def test_graph_replay_sees_new_values(name, knobs):
    B, narrow, trans, check, v0, v1 = setup(name, knobs)
    Bu = clone(B, v0, narrow, "narrow")
    check(info64(Bu, trans))
    xn, y0 = vectors(B, trans)
    want0 = product(clone(B, v0, narrow, False), trans, xn, y0, 1.0, 0.0)
    want1 = product(clone(B, v1, narrow, False), trans, xn, y0, 1.0, 0.0)
    x = dev(xn)
    op = V.adjoint(Bu) if trans else Bu
    s = torch.cuda.Stream()
    y = torch.full((len(y0),), float("nan"), dtype=torch.float64, device=DEV)
    d1 = dev(v1)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        V.mul_(y, op, x)  # eager once, outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        V.mul_(y, op, x)
    g.replay()
    torch.cuda.synchronize()
    assert bitwise(y.cpu().numpy(), want0)
    Bu.update_values(d1)
    torch.cuda.synchronize()
    g.replay()  # no re-capture
    torch.cuda.synchronize()
    assert bitwise(y.cpu().numpy(), want1)
    Bu.release()


def test_refused_float64_and_short_val_keep_the_old_values(knobs):
    B, narrow, trans, check, v0, v1 = setup("mixed", knobs)
    Bu = clone(B, v0, narrow, "narrow")
    check(info64(Bu, trans))
    x, y0 = vectors(B, trans)
    before = product(Bu, trans, x, y0, 1.0, 0.0)
    (h,) = Bu._handles.h.values()
    v64, d64 = v1.astype(np.float64), dev(v1.astype(np.float64))
    for ptr, mem in ((v64.ctypes.data, L.VBC_MEM_HOST), (d64.data_ptr(), L.VBC_MEM_DEVICE)):
        st = L.lib().vbc_update_values(h, ptr, len(v64), L.VBC_F64, mem, None)
        assert st == L.VBC_UNSUPPORTED_DTYPE and "VBC_CREATE_NARROW_UPDATABLE" in L.last_error()
    i32 = np.ones(len(v1), np.int32)
    assert L.lib().vbc_update_values(h, i32.ctypes.data, len(i32), L.VBC_I32, L.VBC_MEM_HOST, None) == L.VBC_UNSUPPORTED_DTYPE
    torch.cuda.synchronize()
    assert bitwise(product(Bu, trans, x, y0, 1.0, 0.0), before)
    short = v1[: int(B.ofs[-1]) - 2].copy()
    st = L.lib().vbc_update_values(h, short.ctypes.data, len(short), L.VBC_F32, L.VBC_MEM_HOST, None)
    assert st == L.VBC_DIM_MISMATCH
    assert bitwise(product(Bu, trans, x, y0, 1.0, 0.0), before)
    with pytest.raises(L.UnsupportedDtype):  # the Python mirror, before any handle is touched
        Bu.update_values(d64)
    with pytest.raises(L.DimensionMismatch):
        Bu.update_values(dev(short))
    assert bitwise(product(Bu, trans, x, y0, 1.0, 0.0), before)
    # a narrow handle without the flag refuses the update, and 0x200 is what makes the difference
    Bn = clone(B, v0, narrow, False)
    st = L.lib().vbc_update_values(Bn.handle(0, trans, compute=L.VBC_F64), v1.ctypes.data, len(v1), L.VBC_F32,
                                   L.VBC_MEM_HOST, None)
    assert st == L.VBC_INVALID_ARG
    Bu.release()
    Bn.release()


@pytest.mark.parametrize("name", ["planar_bx_w3", "fwd_on_bt"])
def test_two_updates_in_a_row_return_the_original_product(name, knobs):
    B, narrow, trans, check, v0, v1 = setup(name, knobs)
    Bu = clone(B, v0, narrow, "narrow")
    check(info64(Bu, trans))
    x, y0 = vectors(B, trans)
    first = [product(Bu, trans, x, y0, a, b) for a, b in AB]
    Bu.update_values(dev(v1))
    mid = product(Bu, trans, x, y0, 1.0, 0.0)
    assert not bitwise(mid, first[0])
    Bu.update_values(v0)  # back, from the host
    for (a, b), want in zip(AB, first):
        assert bitwise(product(Bu, trans, x, y0, a, b), want), (a, b)
    Bu.release()
