"""In-place value updates of sharded handles on the GPU (vbc.h VBC_CREATE_UPDATABLE_SHARDS,
vbc_sharded_update_values; csrc/vbc_pack.hip).

Criterion (that of tests/test_gpu_update.py): after update_values(v2) every product of the updatable sharded
object is np.array_equal to that of a fresh sharded object built WITHOUT the flag from v2 -- same devices, split
and flags -- and before the update to the fresh unflagged one built from v1.  v1 / v2 are small integers with
different zero patterns; both directions; alpha, beta = (1, 0) and (0.5, -2.0) (an integer handle takes integer
alpha and beta only: (3, -2) there).

The partial-output direction (stripes: B x, rows: B'x) on devices = [0] * N adds the shards' partial sums shard
after shard on one stream.  Every roundtrip first builds two fresh unflagged handles with equal values and
compares their products: where they agree bitwise (on an MI355X they did in every case of this file -- the
comparison is made each time and printed), that direction is compared bitwise like the others; where they do
not, it is compared within TOL64 of tests/test_gpu_parity.py instead.  Disjoint outputs must always agree bitwise.

With one GPU every path runs as devices = [0] * N (no communicator, or one rank); the ncclSend / ncclRecv of the
slices runs in test_distinct_devices only, which needs two GPUs.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from sparsematrixvbcs_amd import _lib as L
from sparsematrixvbcs_amd import distributed as D
from tests.test_gpu_parity import TOL64, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def with_values(B, val):
    if hasattr(B, "Pi"):
        return V.SparseMatrixVBC(B.U, B.W, B.m, B.n, B.Pi, B.Phi, B.pos, B.idx, B.ofs, val.copy())
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, val.copy())


def two_value_sets(B, seed=1):
    """v1, v2: small integers (exact in every eltype), each zero on its own tenth of the entries."""
    rng = np.random.default_rng(seed)
    n, dt = len(B.val), B.val.dtype
    if dt == np.bool_:
        v1 = rng.random(n) < 0.5
        return v1, ~v1
    v1 = rng.integers(1, 9, n) * rng.choice([-1, 1], n)
    v2 = rng.integers(1, 9, n) * rng.choice([-1, 1], n)
    z = rng.permutation(n)
    v1[z[: n // 10]] = 0
    v2[z[n // 10: 2 * (n // 10)]] = 0
    assert ((v1 == 0) & (v2 != 0)).any() or n < 10
    return v1.astype(dt), v2.astype(dt)


def sharded(B, val, devices, split, updatable=False, **kw):
    return D.MultiGPUSparseMatrix(with_values(B, val), devices=devices, split=split, updatable=updatable, **kw)


def products(S, ydtype=np.float64, seed=17):
    """[(trans, y)] for B'x and B x, each with the default and a general alpha / beta."""
    rng = np.random.default_rng(seed)
    ydtype = np.dtype(ydtype)
    out = []
    for trans in (True, False):
        nx, ny = (S.m, S.n) if trans else (S.n, S.m)
        for alpha, beta in ((1.0, 0.0), (0.5, -2.0) if ydtype.kind == "f" else (3.0, -2.0)):
            if ydtype.kind == "f":
                x, y0 = rng.uniform(-1, 1, nx).astype(ydtype), rng.uniform(-1, 1, ny).astype(ydtype)
            else:
                x, y0 = rng.integers(-8, 9, nx).astype(ydtype), rng.integers(-8, 9, ny).astype(ydtype)
            y = dev(y0)
            V.mul_(y, S.T if trans else S, dev(x), alpha, beta)
            out.append((trans, y.cpu().numpy()))
    return out


def agree(got, want, exact):
    for (trans, a), (_, b), ex in zip(got, want, exact):
        if ex:
            assert np.array_equal(a, b), ("trans" if trans else "fwd", np.flatnonzero(a != b)[:5])
        else:
            assert rel(a, b) <= TOL64, ("trans" if trans else "fwd", rel(a, b))


def roundtrip(B, devices, split, values=None, ydtype=np.float64, convert=None, **kw):
    """The criterion of the module docstring; returns the updated object (holding v2) and the fresh v1 / v2 products."""
    v1, v2 = values if values is not None else two_value_sets(B)
    c = convert or (lambda v: v)  # what a fresh handle is built from when the update passes another eltype
    F1a, F1b, F2 = (sharded(B, c(v), devices, split, **kw) for v in (v1, v1, v2))
    p1, p1b, p2 = (products(F, ydtype) for F in (F1a, F1b, F2))
    exact = [np.array_equal(a, b) for (_, a), (_, b) in zip(p1, p1b)]
    for (trans, _), ex in zip(p1, exact):
        if (split == "stripes") == trans:
            assert ex, "a disjoint output differs between two equal handles"
    print("bitwise between equal fresh handles:", [(t, e) for (t, _), e in zip(p1, exact)])
    Su = sharded(B, c(v1), devices, split, updatable=True, **kw)
    assert Su.updatable and Su.shards() == F1a.shards() and Su.x_spans() == F1a.x_spans()  # no cut or span moves
    agree(products(Su, ydtype), p1, exact)
    Su.update_values(dev(v2))
    agree(products(Su, ydtype), p2, exact)
    Su.update_values(v1)  # and back, from a host val
    agree(products(Su, ydtype), p1, exact)
    Su.update_values(v2)
    agree(products(Su, ydtype), p2, exact)
    for F in (F1a, F1b, F2):
        F.release()
    return Su, p1, p2


@pytest.fixture(scope="module")
def mat():
    rng = np.random.default_rng(11)  # the matrix of tests/test_gpu_multigpu.py: several width buckets per shard
    return V.synthetic.vbr_1dvbc(9000, 2500, 60000, rng.integers(1, 9, 2500), W=8, seed=12)


@pytest.mark.parametrize("split", ["stripes", "rows"])
@pytest.mark.parametrize("devices", [[0], [0, 0, 0], [0] * 7])
def test_mixed_widths(mat, split, devices):
    B = mat
    Su, _, _ = roundtrip(B, devices, split)
    N = len(devices)
    cuts = D.stripe_split(B, N) if split == "stripes" else D.row_split(B, N)
    ranges = [(lo, hi) for lo, hi, _ in Su.shards()]
    if split == "stripes":
        assert ranges == [(int(B.Phi.spl[a] - 1), int(B.Phi.spl[b] - 1)) for a, b in zip(cuts[:-1], cuts[1:])]
    else:
        assert ranges == [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    F = sharded(B, two_value_sets(B)[0], devices, split)  # Su's create-time values (nnz_hint is create-time)
    for g in range(N):  # each shard keeps its own map, and nothing else about it changes
        iu, i0 = Su.shard_info(g), F.shard_info(g)
        assert iu["device_bytes"] > i0["device_bytes"], g
        assert {k: v for k, v in iu.items() if k != "device_bytes"} == {k: v for k, v in i0.items() if k != "device_bytes"}
    F.release()
    Su.release()


@pytest.mark.parametrize("split", ["stripes", "rows"])
def test_more_shards_than_stripes(split):
    """3 stripes on 8 shards: empty shards, zero-length slices, zero chunks."""
    A = np.zeros((40, 6))
    A[::3, 1] = 1.0
    A[5, 4] = 2.0
    A[7, 0] = A[8, 0] = 3.0
    B = V.SparseMatrix1DVBC[4](sp.csc_matrix(A), V.EquiChunker(2))
    assert len(B.Phi) == 3
    Su, _, _ = roundtrip(B, [0] * 8, split)
    if split == "stripes":
        assert sum(lo == hi for lo, hi, _ in Su.shards()) >= 5
    Su.release()


def test_node_aligned_row_cuts():
    """The ldoor stand-in (3 x 3 node blocks: runs of 3 rows), row split over 4 shards, both directions."""
    B = V.SparseMatrix1DVBC[8](V.synthetic.standin("GHS_psdef/ldoor", scale=0.005).T.tocsc(), V.StrictChunker(8))
    assert D.row_runs(B) == 3
    Su, _, _ = roundtrip(B, [0] * 4, "rows")
    assert all(lo % 3 == 0 for lo, _, _ in Su.shards())
    Su.release()


def vbc2d(seed, dtype=np.float64):
    A = sp.random(700, 520, density=0.02, random_state=seed, format="csc", dtype=np.float64)
    A.data = np.random.default_rng(seed).uniform(-1, 1, A.nnz)
    return V.SparseMatrixVBC[4, 4](A.astype(dtype), V.AlternatingPacker(V.OverlapChunker(0.9, 4), V.OverlapChunker(0.9, 4)))


@pytest.mark.parametrize("split", ["stripes", "rows"])
def test_2d(split):
    B = vbc2d(3)
    Su, _, _ = roundtrip(B, [0, 0, 0], split)
    assert Su.is2d
    Su.release()


def test_fp32_values_into_fp64_handle(mat):
    """A 4-byte pack: fp32 values (not integers) converted by the shards' update kernels."""
    B = mat
    rng = np.random.default_rng(4)
    v1 = rng.uniform(-1, 1, len(B.val)).astype(np.float32)
    v2 = rng.uniform(-1, 1, len(B.val)).astype(np.float32)
    Su, _, _ = roundtrip(B, [0, 0, 0], "rows", values=(v1, v2), convert=lambda v: v.astype(np.float64))
    Su.release()


@pytest.mark.parametrize("kind", ["i32", "bool"])
def test_integer_handles(mat, kind):
    """An Int32 matrix on the exact integer path (4-byte pack) and a Bool one (1-byte pack); then Int64 values
    into the Int32 matrix's handle: a wider val_dtype than at create, so the staging grows."""
    dt = np.int32 if kind == "i32" else np.bool_
    B = with_values(mat, np.ones(len(mat.val), dt))
    Su, p1, _ = roundtrip(B, [0, 0, 0], "rows", ydtype=np.int64)
    with pytest.raises(L.UnsupportedDtype):  # through the C entry itself
        v = np.ones(len(B.val))
        L.check(L.lib().vbc_sharded_update_values(Su._h, v.ctypes.data, len(v), L.VBC_F64, L.VBC_MEM_HOST, None))
    with pytest.raises(L.UnsupportedDtype):
        Su.update_values(dev(np.ones(len(B.val))))
    if kind == "i32":
        v1, _ = two_value_sets(B)
        Su.update_values(dev(v1.astype(np.int64)))
        agree(products(Su, np.int64), p1, [True] * 4)
    Su.release()


def test_stream_order_without_synchronisation(mat):
    B = mat
    v1, v2 = two_value_sets(B)
    devices, split = [0, 0, 0], "rows"
    x = np.random.default_rng(5).uniform(-1, 1, B.n)
    want = []
    for v in (v1, v2):
        F = sharded(B, v, devices, split)
        y = torch.full((B.m,), float("nan"), dtype=torch.float64, device=DEV)
        V.mul_(y, F, dev(x))  # B x: the row split's disjoint output
        want.append(y.cpu().numpy())
        F.release()
    Su = sharded(B, v1, devices, split, updatable=True)
    xd, d2 = dev(x), dev(v2)
    y1 = torch.full((B.m,), float("nan"), dtype=torch.float64, device=DEV)
    y2 = torch.full((B.m,), float("nan"), dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        V.mul_(y1, Su, xd)
        Su.update_values(d2)
        V.mul_(y2, Su, xd)
    torch.cuda.synchronize()
    assert np.array_equal(y1.cpu().numpy(), want[0]) and np.array_equal(y2.cpu().numpy(), want[1])
    Su.release()


def test_errors(mat):
    B = mat
    v1, v2 = two_value_sets(B)
    plain = sharded(B, v1, [0, 0], "rows")
    with pytest.raises(L.ArgumentError):
        plain.update_values(v2)
    st = L.lib().vbc_sharded_update_values(plain._h, v2.ctypes.data, len(v2), L.VBC_F64, L.VBC_MEM_HOST, None)
    assert st == L.VBC_INVALID_ARG and "VBC_CREATE_UPDATABLE_SHARDS" in L.last_error()
    plain.release()
    Su = sharded(B, v1, [0, 0], "rows", updatable=True)
    before = products(Su)
    short = np.ones(int(B.ofs[-1]) - 2)
    for mem, p in ((L.VBC_MEM_HOST, short.ctypes.data), (L.VBC_MEM_DEVICE, dev(short).data_ptr())):
        assert L.lib().vbc_sharded_update_values(Su._h, p, len(short), L.VBC_F64, mem, None) == L.VBC_DIM_MISMATCH
    with pytest.raises(L.DimensionMismatch):
        Su.update_values(dev(short))
    with pytest.raises(L.DimensionMismatch):
        Su.update_values(short)
    assert L.lib().vbc_sharded_update_values(Su._h, v2.ctypes.data, len(v2), 99, L.VBC_MEM_HOST, None) \
        == L.VBC_UNSUPPORTED_DTYPE
    torch.cuda.synchronize()
    agree(products(Su), before, [True] * 4)  # the same object, nothing written: bitwise
    Su.release()
    # the single-GPU creates refuse the sharded flag
    out = C.c_void_p()
    st = L.lib().vbc1d_create(C.byref(out), B.m, B.n, B.W, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                              B.idx.ctypes.data, B.ofs.ctypes.data, B.val.ctypes.data, len(B.val), L.VBC_F64, 0,
                              L.VBC_CREATE_TRANSPOSED | L.VBC_CREATE_UPDATABLE_SHARDS)
    assert st == L.VBC_INVALID_ARG and not out.value
    t = L.vbc_types(L.VBC_F64, 64, L.VBC_F64, 0)
    st = L.lib().vbc1d_create_ex(C.byref(out), B.m, B.n, B.W, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data,
                                 B.idx.ctypes.data, B.ofs.ctypes.data, B.val.ctypes.data, len(B.val), C.byref(t), 0,
                                 L.VBC_CREATE_TRANSPOSED | L.VBC_CREATE_UPDATABLE_SHARDS)
    assert st == L.VBC_INVALID_ARG and not out.value


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2,
                    reason="needs two GPUs (ncclSend / ncclRecv of the value slices between distinct devices)")
@pytest.mark.parametrize("split", ["stripes", "rows"])
def test_distinct_devices(mat, split):
    Su, _, _ = roundtrip(mat, [0, 1], split)
    Su.release()


@pytest.mark.parametrize("split", ["stripes", "rows"])
def test_distributed_class_world1(mat, split):
    """ShardedSparseMatrix1DVBC, world 1, libvbc as the rank's product: update_values(dev(v2)) equals a fresh
    object built from v2 (the collective-free halves of both products)."""
    B = mat
    v1, v2 = two_value_sets(B)

    def both(S):
        rng = np.random.default_rng(8)
        xt, xf = dev(rng.uniform(-1, 1, B.m)), dev(rng.uniform(-1, 1, B.n))
        yt = torch.full((B.n,), float("nan"), dtype=torch.float64, device=DEV)
        yf = torch.full((B.m,), float("nan"), dtype=torch.float64, device=DEV)
        S.local_mul_t(yt, xt)
        S.local_mul(yf, xf)
        return yt.cpu().numpy(), yf.cpu().numpy()

    Su = D.ShardedSparseMatrix1DVBC(with_values(B, v1), 0, 1, split=split, updatable=True)
    assert all(np.array_equal(a, b) for a, b in zip(both(Su), both(D.ShardedSparseMatrix1DVBC(with_values(B, v1), 0, 1, split=split))))
    Su.update_values(dev(v2))
    want = both(D.ShardedSparseMatrix1DVBC(with_values(B, v2), 0, 1, split=split))
    assert all(np.array_equal(a, b) for a, b in zip(both(Su), want))
    nv = int(B.ofs[-1]) - 1
    assert np.array_equal(Su.local.val[:nv], v2[:nv])
    assert any(f & L.VBC_CREATE_UPDATABLE for _, f, _ in Su.local._handles.h)
