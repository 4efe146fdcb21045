"""Row-major multi-RHS B'X fused over the slotted layout (spmm_slots, csrc/vbc_slots_mm.h; vbc.h planar_mask bit 22).

A slot folds its stripe serially in stored row order and spmm_slots keeps one accumulator per right-hand side, so
every column of the fused product is, bit for bit, the single-vector product of that column on the same handle:
the comparisons with the per-column products below are np.array_equal on the raw bits, no tolerance.  The oracle
comparisons use integer inputs (every partial sum exact, tests/test_gpu_operand_views.py), again without tolerance.

Two facts of the layout as the planner builds it, which decide what bit 22 covers:
  * the only narrow-row form (one lane holding two segments, run_slots_narrow) is the Float32 w = 2 bucket -- the
    Float32 FE grid itself -- and spmm_slots has that form too, so the Float32 FE grid fuses;
  * a SparseMatrixCSC handle keeps one segment per lane slot (its w = 1 narrow forms were never kept), so its
    slotted buckets are of the plain form spmm_slots covers and the handle fuses like any other: the test of the
    CSC handle asserts bit 22 from the forms vbc_info reports, and the product bitwise against per-column.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
BIT = 1 << 22
NRHS = (2, 3, 4, 5, 8, 9, 13)
AB = ((1.0, 0.0), (-0.5, 2.0))
KINDS = {"f32": (np.float32, np.float32, False), "f64": (np.float64, np.float64, False),
         "narrow": (np.float32, np.float64, True)}  # value dtype, vector dtype, B.narrow


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def with_values(B, val, narrow=False, updatable=False):
    """A new matrix object (its own handles: the knobs are read when a handle is created) with B's pattern."""
    M = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, np.array(val))
    if narrow:
        M.narrow = narrow
    if updatable:
        M.updatable = updatable
    _LIVE.append(M)
    return M


_LIVE = []


@pytest.fixture(autouse=True)
def release_handles():
    yield
    for M in _LIVE:
        M.release()
    _LIVE.clear()


@pytest.fixture
def forced(monkeypatch):
    for k in ("VBC_MM_SLOTS", "VBC_SLOT_KEYS16", "VBC_SLOTS_SORT", "VBC_SLOT_DEDUP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VBC_SLOTS", "1")
    return monkeypatch


def random_values(B, vdt, seed=5):
    """Non-integer values of either sign (the summation order shows in the last bits), the tail pad kept zero."""
    rng = np.random.default_rng(seed)
    val = np.zeros(len(B.val), vdt)
    nv = int(B.ofs[-1]) - 1
    val[:nv] = rng.uniform(0.25, 1, nv) * rng.choice([-1, 1], nv)
    return val


def integer_values(B, vdt, seed=1):
    """Integers in [-8, 8], a tenth of them zero (test_gpu_operand_views.integer_values)."""
    rng = np.random.default_rng(seed)
    val = np.zeros(len(B.val), vdt)
    nv = int(B.ofs[-1]) - 1
    v = rng.integers(1, 9, nv) * rng.choice([-1, 1], nv)
    v[rng.permutation(nv)[: nv // 10]] = 0
    val[:nv] = v
    return val


@functools.lru_cache(maxsize=None)
def pattern(name):
    if name == "fe37":
        return V.synthetic.fe_grid_2d(37, dof=2)
    if name == "fe120":  # several ranges, several chunks per range, a partial last chunk
        return V.synthetic.fe_grid_2d(120, dof=2)
    if name == "vbr":  # mixed widths 1..8, unequal stripe lengths: padding rows in every chunk
        return V.synthetic.vbr_1dvbc(400, 300, 1400, np.arange(300) % 8 + 1, W=8, seed=7)
    if name == "vbr12":  # widths 1 and 2 only: slotted in Float64 without a planar bucket
        return V.synthetic.vbr_1dvbc(400, 300, 1400, np.arange(300) % 2 + 1, W=8, seed=8)
    raise KeyError(name)


def info(M, kind):
    return M.info(trans=True, compute=L.dtype_code(np.dtype(KINDS[kind][1])))


def assert_slotted(inf):
    assert inf["slot_bins"] > 0 and inf["planar_bins"] == 0 and inf["sweep_bins"] == 0, inf


def view2d(rows, nrhs, ld, off, dt, fill):
    """(buffer, rows x nrhs row-major view with leading dimension ld at element offset off); 16 elements of `fill`
    on either side and in the gap columns."""
    buf = torch.full((16 + off + rows * ld + 16,), fill, dtype=dt, device=DEV)
    return buf, buf[16 + off: 16 + off + rows * ld].view(rows, ld)[:, :nrhs]


def bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def per_column(M, X, Y0, alpha, beta):
    """nrhs single-vector products mul_(y, M', x, alpha, beta) on contiguous vectors: the reference of every test."""
    Y = torch.empty_like(Y0)
    for j in range(X.shape[1]):
        y = Y0[:, j].contiguous()
        V.mul_(y, V.adjoint(M), X[:, j].contiguous(), alpha, beta)
        Y[:, j] = y
    return Y


def fused(M, X, Y0, alpha, beta, ld_extra=0, xoff=0, yoff=0):
    """The engine="vector" product on row-major views; returns the window of Y, and checks that nothing else of
    the Y allocation and nothing of the X allocation changed and that the NaN around X reached no output."""
    n, k = Y0.shape
    xbuf, Xv = view2d(X.shape[0], k, k + ld_extra, xoff, X.dtype, float("nan"))
    Xv.copy_(X)
    xbefore = bits(xbuf)
    ybuf, Yv = view2d(n, k, k + ld_extra, yoff, Y0.dtype, float("nan"))
    if beta != 0:
        Yv.copy_(Y0)
    canary = bits(ybuf).copy()
    V.mulmat_(Yv, V.adjoint(M), Xv, alpha, beta, engine="vector")
    got = Yv.clone()
    after = bits(ybuf).copy()
    win = torch.zeros_like(ybuf, dtype=torch.bool)
    win[16 + yoff: 16 + yoff + n * (k + ld_extra)].view(n, k + ld_extra)[:, :k] = True
    out = ~win.cpu().numpy()
    assert np.array_equal(after[out], canary[out]), "stray write outside the live columns of Y"
    assert np.array_equal(bits(xbuf), xbefore), "X changed"
    return got


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def operands(M, vdt, k=max(NRHS), seed=11):
    rng = np.random.default_rng(seed)
    return dev(rng.uniform(-1, 1, (M.m, k)).astype(vdt)), dev(rng.uniform(-1, 1, (M.n, k)).astype(vdt))


# ---------------------------------------------------------------------------------------------------------------
# 1. path taken
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bit22_set_on_forced_slotted_fe_grid(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    inf = info(M, kind)
    assert_slotted(inf)
    assert inf["planar_mask"] & BIT, inf
    assert bool(inf["planar_mask"] & (1 << 12)) == narrow, inf


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bit22_clear_with_knob_off(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_MM_SLOTS", "0")
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    inf = info(M, kind)
    assert_slotted(inf)
    assert not inf["planar_mask"] & BIT, inf


def test_bit22_clear_on_runtime_width(forced):
    B = V.synthetic.vbr_1dvbc(900, 300, 1800, 16, W=16, seed=16)  # 16-wide stripes: a runtime-width bucket
    M = with_values(B, random_values(B, np.float64))
    assert not info(M, "f64")["planar_mask"] & BIT


def test_bit22_clear_on_planar_bucket(monkeypatch):
    monkeypatch.delenv("VBC_SLOTS", raising=False)
    B = V.synthetic.fe_stiffness_3d_1dvbc(3 * 4000, 3 * 4000 * 40, 3)  # the ldoor-like stand-in at small scale
    inf = B.info(trans=True)
    _LIVE.append(B)
    assert inf["planar_bins"] > 0, inf
    assert not inf["planar_mask"] & BIT, inf


def test_bit22_clear_on_int64(forced):
    B = pattern("fe37")
    M = with_values(B, integer_values(B, np.int64))
    assert not M.info(trans=True, compute=L.VBC_I64)["planar_mask"] & BIT


def test_csc_handle(forced):
    """A SparseMatrixCSC (TrSpMV!) handle: its buckets keep one segment per lane slot, the form spmm_slots covers
    (module docstring), so bit 22 is set exactly when the layout is slotted without planar / swept buckets, and the
    fused product equals the per-column one bit for bit."""
    rng = np.random.default_rng(3)
    A = sp.random(500, 700, density=0.02, format="csc", random_state=4, data_rvs=lambda n: rng.uniform(0.25, 1, n))
    A.sort_indices()
    M = V.SparseMatrixCSC(A)
    _LIVE.append(M)
    inf = M.info(trans=True)
    assert inf["slot_bins"] > 0, inf
    want = inf["planar_bins"] == 0 and inf["sweep_bins"] == 0
    assert bool(inf["planar_mask"] & BIT) == want, inf
    X, Y0 = operands(M, np.float64, 5)
    for alpha, beta in AB:
        assert same(fused(M, X, Y0, alpha, beta, 1), per_column(M, X, Y0, alpha, beta))


# ---------------------------------------------------------------------------------------------------------------
# 2. bitwise against column by column
# ---------------------------------------------------------------------------------------------------------------

def sweep(M, vdt, lds=(0, 1, 5), offs=((0, 0), (1, 0), (0, 1), (1, 1))):
    X, Y0 = operands(M, vdt)
    for alpha, beta in AB:
        ref = per_column(M, X, Y0, alpha, beta)
        for k in NRHS:
            for ld in lds:
                for xo, yo in offs:
                    got = fused(M, X[:, :k], Y0[:, :k], alpha, beta, ld, xo, yo)
                    assert same(got, ref[:, :k]), (k, ld, xo, yo, alpha, beta)
    return ref


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["fe120", "vbr", "vbr12"])
def test_bitwise_against_columns(forced, name, kind):
    vdt, xdt, narrow = KINDS[kind]
    B = pattern(name)
    forced.setenv("VBC_SLOT_PLANAR", "0")  # every width bucket in the plain slotted form
    M = with_values(B, random_values(B, vdt), narrow)
    inf = info(M, kind)
    assert_slotted(inf)
    assert inf["planar_mask"] & BIT, inf
    ref = sweep(M, xdt)
    if narrow:  # the narrow handle against the wide one (the same float32 values, widened exactly)
        W = with_values(B, random_values(B, vdt))
        X, Y0 = operands(W, xdt)
        assert same(ref, per_column(W, X, Y0, *AB[-1]))


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("keys", ["0", "1", "2"])
def test_bitwise_keys_orders_dedup(forced, kind, keys):
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_SLOT_KEYS16", keys)
    forced.setenv("VBC_SLOT_PLANAR", "0")
    for name in ("fe120", "vbr"):
        B = pattern(name)
        for sort in ("0", "2"):  # affine and table-mapped outputs
            for dedup in ("0", "1"):
                forced.setenv("VBC_SLOTS_SORT", sort)
                forced.setenv("VBC_SLOT_DEDUP", dedup)
                M = with_values(B, random_values(B, vdt), narrow)
                inf = info(M, kind)
                assert_slotted(inf)
                assert inf["planar_mask"] & BIT, inf
                sweep(M, xdt, lds=(1,), offs=((0, 0), (1, 1)))
                M.release()


# ---------------------------------------------------------------------------------------------------------------
# 3. against the oracle (integer inputs: exact)
# ---------------------------------------------------------------------------------------------------------------

def oracle_product(B, val, X, Y0, alpha, beta):
    R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, np.asarray(val, np.float64))
    Y = np.asfortranarray(Y0.astype(np.float64))
    return O.mulmat_t(R, X.astype(np.float64), Y, alpha, beta)


def check_oracle(M, B, val, kind, k=9):
    xdt = KINDS[kind][1]
    rng = np.random.default_rng(23)
    X = rng.integers(-8, 9, (B.m, k)).astype(xdt)
    Y0 = rng.integers(-8, 9, (B.n, k)).astype(xdt)
    for alpha, beta in ((1.0, 0.0), (-1.0, 2.0)):
        got = fused(M, dev(X), dev(Y0), alpha, beta, 3, 1, 1).cpu().numpy().astype(np.float64)
        assert np.array_equal(got, oracle_product(B, val, X, Y0, alpha, beta)), (alpha, beta)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["fe37", "vbr"])
def test_oracle_exact(forced, name, kind):
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_SLOT_PLANAR", "0")
    B = pattern(name)
    val = integer_values(B, vdt)
    M = with_values(B, val, narrow)
    inf = info(M, kind)
    assert_slotted(inf)
    assert inf["planar_mask"] & BIT, inf
    check_oracle(M, B, val, kind)


@functools.lru_cache(maxsize=None)
def slotted_and_merge():
    """2-wide stripes of 10 rows each (uniform: slotted under the planner's own rule) beside 1-wide stripes of 0 to
    ~120 rows (the padding of any slotted order exceeds VBC_SLOTS_PAD: merge layout)."""
    rng = np.random.default_rng(41)
    m, L2, L1 = 4000, 1500, 400
    w = np.concatenate([np.full(L2, 2), np.full(L1, 1)]).astype(np.int64)
    cnt = np.concatenate([np.full(L2, 10), (rng.pareto(1.0, L1) * 4).astype(np.int64).clip(0, 120)])
    rows = np.concatenate([np.sort(rng.choice(m, c, replace=False)) for c in cnt]) + 1
    spl = np.concatenate([[1], 1 + np.cumsum(w)])
    pos = np.concatenate([[1], 1 + np.cumsum(cnt)])
    ofs = np.concatenate([[1], 1 + np.cumsum(cnt * w)])
    val = np.zeros(int(ofs[-1]) - 1 + 64)
    return V.SparseMatrix1DVBC(8, m, int(spl[-1]) - 1, V.SplitPartition(spl), pos, rows.astype(np.int64), ofs, val)


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_oracle_exact_slotted_and_merge_buckets(monkeypatch, kind):
    for k in ("VBC_SLOTS", "VBC_MM_SLOTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VBC_SLOTS_SORT", "0")  # natural segment order only: the ragged bucket stays in the merge layout
    monkeypatch.setenv("VBC_SMALL_FUSE", "0")  # (no fused split of a small matrix: the two buckets as a large one has them)
    B = slotted_and_merge()
    val = integer_values(B, KINDS[kind][0])
    M = with_values(B, val)
    inf = info(M, kind)
    assert inf["slot_bins"] > 0 and inf["bins_t"] > 0 and inf["planar_bins"] == 0 and inf["sweep_bins"] == 0, inf
    assert inf["planar_mask"] & BIT, inf
    check_oracle(M, B, val, kind)


# ---------------------------------------------------------------------------------------------------------------
# 4. memory discipline, 5. non-finite x
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_memory_discipline(forced, kind):
    """fused() embeds X and Y in NaN: gap columns, pads and all of X unchanged (asserted there); here: no NaN of
    X's surroundings reaches Y, and beta = 0 overwrites a NaN-filled Y in its live columns."""
    vdt, xdt, narrow = KINDS[kind]
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    assert info(M, kind)["planar_mask"] & BIT
    X, Y0 = operands(M, xdt)
    for k in (3, 8, 13):
        for xo, yo in ((0, 0), (1, 1)):
            got = fused(M, X[:, :k], torch.full_like(Y0[:, :k], float("nan")), 1.0, 0.0, 5, xo, yo)
            assert torch.isfinite(got).all(), (k, xo, yo)
            got = fused(M, X[:, :k], Y0[:, :k], -0.5, 2.0, 5, xo, yo)
            assert torch.isfinite(got).all(), (k, xo, yo)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["vbr", "fe37"])
def test_nonfinite_rows_of_x(forced, name, kind):
    """Inf / NaN in single rows of X: bitwise the per-column result, and a stripe that stores none of those rows
    stays finite -- its padding rows take x as 0 by a select."""
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_SLOT_PLANAR", "0")
    B = pattern(name)
    M = with_values(B, random_values(B, vdt), narrow)
    assert info(M, kind)["planar_mask"] & BIT
    X, Y0 = operands(M, xdt, 5)
    bad = [0, B.m // 3, B.m - 1]
    X[bad[0], :] = float("inf")
    X[bad[1], 1] = float("nan")
    X[bad[2], 3] = -float("inf")
    for alpha, beta in AB:
        got = fused(M, X, Y0, alpha, beta, 2, 1, 0)
        assert same(got, per_column(M, X, Y0, alpha, beta))
    spl, pos, idx = B.Phi.spl, B.pos, B.idx
    touched = np.zeros(B.n, bool)
    for l in range(len(spl) - 1):
        if np.isin(idx[pos[l] - 1: pos[l + 1] - 1] - 1, bad).any():
            touched[spl[l] - 1: spl[l + 1] - 1] = True
    assert touched.any() and not touched.all()
    clean = torch.from_numpy(~touched).to(DEV)
    assert torch.isfinite(got[clean]).all()


# ---------------------------------------------------------------------------------------------------------------
# 6. graph and update, 7. knob off
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_graph_replays(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    assert info(M, kind)["planar_mask"] & BIT
    X, Y0 = operands(M, xdt, 5)
    Y = torch.empty_like(Y0)
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        V.mulmat_(Y, V.adjoint(M), X, 1.0, 0.0, engine="vector")  # (handles built, code loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        V.mulmat_(Y, V.adjoint(M), X, 1.0, 0.0, engine="vector")
    for r in range(3):
        X.copy_(operands(M, xdt, 5, seed=100 + r)[0])
        g.replay()
        torch.cuda.synchronize()
        assert same(Y, per_column(M, X, Y0, 1.0, 0.0)), r


@pytest.mark.parametrize("kind,updatable", [("f32", True), ("f64", True), ("narrow", "narrow")])
def test_update_then_fused(forced, kind, updatable):
    vdt, xdt, narrow = KINDS[kind]
    B = pattern("fe37")
    v1, v2 = random_values(B, vdt, 5), random_values(B, vdt, 6)
    M = with_values(B, v1, narrow, updatable)
    assert info(M, kind)["planar_mask"] & BIT
    X, Y0 = operands(M, xdt, 5)
    first = fused(M, X, Y0, -0.5, 2.0)
    M.update_values(v2)
    N = with_values(B, v2, narrow)
    got, want = fused(M, X, Y0, -0.5, 2.0), fused(N, X, Y0, -0.5, 2.0)
    assert same(got, want) and not same(got, first)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_knob_off_same_result(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_MM_SLOTS", "0")
    B = pattern("fe120")
    M = with_values(B, random_values(B, vdt), narrow)
    assert not info(M, kind)["planar_mask"] & BIT
    sweep(M, xdt, lds=(1,), offs=((1, 1),))
