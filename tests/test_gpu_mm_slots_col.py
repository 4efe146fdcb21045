"""Column-major multi-RHS B'X fused over the slotted layout (spmm_slots_col, csrc/vbc_slots_mm.h; vbc.h planar_mask
bit 23).

The operands are what a Julia Matrix is: X[i + j * ldx], Y[i + j * ldy].  A slot folds its stripe serially in stored
row order and spmm_slots_col keeps one accumulator per right-hand side and flushes with run_slots's expressions, so
every column of the fused product is, bit for bit, the single-vector product of that column on the same handle: the
comparisons with the per-column products below are np.array_equal on the raw bits, no tolerance.  The oracle
comparisons use integer inputs (every partial sum exact), again without tolerance.

Bit 23 needs what bit 22 needs of a slotted layout and, on top, no merge bucket in the B'x launch and
VBC_MM_SLOTS_COL not 0 (VBC_MM_SLOTS=0 clears both).  Every test that expects the bit also asserts the layout
(assert_slotted), so a change of the planner cannot make it vacuous.
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
BIT22, BIT = 1 << 22, 1 << 23
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
    for k in ("VBC_MM_SLOTS", "VBC_MM_SLOTS_COL", "VBC_SLOT_KEYS16", "VBC_SLOTS_SORT", "VBC_SLOT_DEDUP"):
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
    """Integers in [-8, 8], a tenth of them zero."""
    rng = np.random.default_rng(seed)
    val = np.zeros(len(B.val), vdt)
    nv = int(B.ofs[-1]) - 1
    v = rng.integers(1, 9, nv) * rng.choice([-1, 1], nv)
    v[rng.permutation(nv)[: nv // 10]] = 0
    val[:nv] = v
    return val


EMPTY_STRIPES = {"vbr": 3, "vbr12": 5, "vbr-empty": 63}


@functools.lru_cache(maxsize=None)
def pattern(name):
    if name == "fe37":
        return V.synthetic.fe_grid_2d(37, dof=2)
    if name == "fe120":  # several ranges, several chunks per range, a partial last chunk
        return V.synthetic.fe_grid_2d(120, dof=2)
    if name == "vbr":  # mixed widths 1..8, unequal stripe lengths: padding rows in every chunk; 3 empty stripes
        return V.synthetic.vbr_1dvbc(400, 300, 1400, np.arange(300) % 8 + 1, W=8, seed=7)
    if name == "vbr12":  # widths 1 and 2 only; 5 empty stripes
        return V.synthetic.vbr_1dvbc(400, 300, 1400, np.arange(300) % 2 + 1, W=8, seed=8)
    if name == "vbr-empty":  # 63 of 300 stripes store no row: the fill list
        return V.synthetic.vbr_1dvbc(400, 300, 450, np.arange(300) % 2 + 1, W=8, seed=9)
    raise KeyError(name)


def test_empty_stripe_counts():
    """The fill list the vbr patterns are here for (stripes that store no row)."""
    for name, want in EMPTY_STRIPES.items():
        B = pattern(name)
        assert int((np.diff(B.pos) == 0).sum()) == want, name


def info(M, kind):
    return M.info(trans=True, compute=L.dtype_code(np.dtype(KINDS[kind][1])))


def assert_slotted(inf):
    assert inf["slot_bins"] > 0 and inf["planar_bins"] == 0 and inf["sweep_bins"] == 0, inf


def assert_fuses(inf):
    assert_slotted(inf)
    assert inf["bins_t"] == 0, inf
    assert inf["planar_mask"] & BIT, inf


def view2d(rows, k, ld, off, dt, fill, cols=None):
    """(buffer, rows x k column-major view with column stride ld at element offset off, inside an allocation of
    `cols` >= k columns); 16 elements of `fill` on either side, in the ld - rows tail of every column and in the
    columns >= k."""
    cols = k if cols is None else cols
    buf = torch.full((16 + off + cols * ld + 16,), fill, dtype=dt, device=DEV)
    return buf, buf[16 + off: 16 + off + ld * k].view(k, ld).T[:rows]


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


def fused(M, X, Y0, alpha, beta, ld_extra=0, xoff=0, yoff=0, cols=None):
    """The engine="vector" product on column-major views; returns the window of Y, and checks that nothing else of
    the Y allocation and nothing of the X allocation changed (the NaN around and between the columns of X reach no
    output: the callers compare with finite references)."""
    n, k = Y0.shape
    m = X.shape[0]
    xbuf, Xv = view2d(m, k, m + ld_extra, xoff, X.dtype, float("nan"), cols)
    Xv.copy_(X)
    xbefore = bits(xbuf)
    ybuf, Yv = view2d(n, k, n + ld_extra, yoff, Y0.dtype, float("nan"), cols)
    if beta != 0:
        Yv.copy_(Y0)
    assert Xv.stride(0) == 1 and Yv.stride(0) == 1 and Yv.stride(1) == n + ld_extra
    canary = bits(ybuf).copy()
    V.mulmat_(Yv, V.adjoint(M), Xv, alpha, beta, engine="vector")
    got = Yv.clone()
    after = bits(ybuf).copy()
    win = torch.zeros_like(ybuf, dtype=torch.bool)
    win[16 + yoff: 16 + yoff + k * (n + ld_extra)].view(k, n + ld_extra)[:, :n] = True
    out = ~win.cpu().numpy()
    assert np.array_equal(after[out], canary[out]), "stray write outside the live rows x k window of Y"
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
def test_bit23_set_on_forced_slotted_fe_grid(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    inf = info(M, kind)
    assert_fuses(inf)
    assert inf["planar_mask"] & BIT22, inf
    assert bool(inf["planar_mask"] & (1 << 12)) == narrow, inf


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bit23_clear_with_its_knob_off(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_MM_SLOTS_COL", "0")
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    inf = info(M, kind)
    assert_slotted(inf)
    assert not inf["planar_mask"] & BIT, inf
    assert inf["planar_mask"] & BIT22, inf


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bits_22_and_23_clear_with_mm_slots_off(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_MM_SLOTS", "0")
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    inf = info(M, kind)
    assert_slotted(inf)
    assert not inf["planar_mask"] & (BIT | BIT22), inf


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
def test_bit23_clear_with_a_merge_bucket(monkeypatch, kind):
    """A slotted and a merge bucket in one launch: row-major fuses (bit 22), column-major runs per column, and the
    per-column product is still exact against the oracle."""
    for k in ("VBC_SLOTS", "VBC_MM_SLOTS", "VBC_MM_SLOTS_COL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VBC_SLOTS_SORT", "0")  # natural segment order only: the ragged bucket stays in the merge layout
    monkeypatch.setenv("VBC_SMALL_FUSE", "0")  # (no fused split of a small matrix)
    B = slotted_and_merge()
    val = integer_values(B, KINDS[kind][0])
    M = with_values(B, val)
    inf = info(M, kind)
    assert inf["slot_bins"] > 0 and inf["bins_t"] > 0 and inf["planar_bins"] == 0 and inf["sweep_bins"] == 0, inf
    assert inf["planar_mask"] & BIT22, inf
    assert not inf["planar_mask"] & BIT, inf
    check_oracle(M, B, val, kind)


def test_bit23_clear_on_runtime_width(forced):
    B = V.synthetic.vbr_1dvbc(900, 300, 1800, 16, W=16, seed=16)  # 16-wide stripes: a runtime-width bucket
    M = with_values(B, random_values(B, np.float64))
    assert not info(M, "f64")["planar_mask"] & BIT


def test_bit23_clear_on_planar_bucket(monkeypatch):
    monkeypatch.delenv("VBC_SLOTS", raising=False)
    B = V.synthetic.fe_stiffness_3d_1dvbc(3 * 4000, 3 * 4000 * 40, 3)  # the ldoor-like stand-in at small scale
    inf = B.info(trans=True)
    _LIVE.append(B)
    assert inf["planar_bins"] > 0, inf
    assert not inf["planar_mask"] & BIT, inf


def test_bit23_clear_on_int64(forced):
    B = pattern("fe37")
    M = with_values(B, integer_values(B, np.int64))
    assert not M.info(trans=True, compute=L.VBC_I64)["planar_mask"] & BIT


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
@pytest.mark.parametrize("name", ["fe120", "vbr", "vbr12", "vbr-empty"])
def test_bitwise_against_columns(forced, name, kind):
    vdt, xdt, narrow = KINDS[kind]
    B = pattern(name)
    forced.setenv("VBC_SLOT_PLANAR", "0")  # every width bucket in the plain slotted form
    M = with_values(B, random_values(B, vdt), narrow)
    assert_fuses(info(M, kind))
    ref = sweep(M, xdt)
    if narrow:  # the narrow handle against the wide one (the same float32 values, widened exactly)
        W = with_values(B, random_values(B, vdt))
        X, Y0 = operands(W, xdt)
        assert same(ref, per_column(W, X, Y0, *AB[-1]))
        assert same(fused(W, X, Y0, *AB[-1], 1, 1, 1), ref)


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
                assert_fuses(info(M, kind))
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
    assert_fuses(info(M, kind))
    check_oracle(M, B, val, kind)


# ---------------------------------------------------------------------------------------------------------------
# 4. memory discipline, 5. non-finite x
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["fe37", "vbr-empty"])
def test_memory_discipline(forced, name, kind):
    """fused() embeds X and Y in NaN -- around them, in the tail of every column and, here, in the columns >= nr of
    an allocation of 16 -- and asserts that nothing outside the live rows x k window of Y and nothing of X changed.
    Here: beta = 0 overwrites a NaN-filled Y with finite values (empty stripes included), and no NaN reaches Y."""
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_SLOT_PLANAR", "0")
    B = pattern(name)
    M = with_values(B, random_values(B, vdt), narrow)
    assert_fuses(info(M, kind))
    X, Y0 = operands(M, xdt)
    for k in (3, 8, 13):
        for xo, yo in ((0, 0), (1, 1)):
            got = fused(M, X[:, :k], torch.full_like(Y0[:, :k], float("nan")), 1.0, 0.0, 5, xo, yo, cols=16)
            assert torch.isfinite(got).all(), (k, xo, yo)
            got = fused(M, X[:, :k], Y0[:, :k], -0.5, 2.0, 5, xo, yo, cols=16)
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
    assert_fuses(info(M, kind))
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
# 6. graph and update, 7. host operands, 8. knob off, 9. CSC
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_graph_captured_on_first_use(forced, kind):
    """The fused column-major product allocates nothing and uses no side stream, so its first call on a fresh handle
    may be a captured one: no eager product of any kind precedes the capture."""
    vdt, xdt, narrow = KINDS[kind]
    B = pattern("fe37")
    M = with_values(B, random_values(B, vdt), narrow)
    assert_fuses(info(M, kind))  # (the handle is created here: a create allocates, a product does not)
    X, Y0 = operands(M, xdt, 5)
    _, Xv = view2d(M.m, 5, M.m + 1, 1, X.dtype, float("nan"))
    _, Yv = view2d(M.n, 5, M.n + 3, 0, X.dtype, float("nan"))
    Xv.copy_(X)
    stream = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        V.mulmat_(Yv, V.adjoint(M), Xv, 1.0, 0.0, engine="vector")
    for r in range(4):  # the graph's first launch, then 3 replays with new X
        if r:
            X = operands(M, xdt, 5, seed=100 + r)[0]
            Xv.copy_(X)
        g.replay()
        torch.cuda.synchronize()
        assert same(Yv, per_column(M, X, Y0, 1.0, 0.0)), r


@pytest.mark.parametrize("kind,updatable", [("f32", True), ("f64", True), ("narrow", "narrow")])
def test_update_then_fused(forced, kind, updatable):
    vdt, xdt, narrow = KINDS[kind]
    B = pattern("fe37")
    v1, v2 = random_values(B, vdt, 5), random_values(B, vdt, 6)
    M = with_values(B, v1, narrow, updatable)
    assert_fuses(info(M, kind))
    X, Y0 = operands(M, xdt, 5)
    first = fused(M, X, Y0, -0.5, 2.0)
    M.update_values(v2)
    N = with_values(B, v2, narrow)
    got, want = fused(M, X, Y0, -0.5, 2.0), fused(N, X, Y0, -0.5, 2.0)
    assert same(got, want) and not same(got, first)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_host_operands(forced, kind):
    """numpy order="F" operands: staged into packed device buffers, the fused product there, copied back."""
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_SLOT_PLANAR", "0")
    B = pattern("vbr-empty")
    M = with_values(B, random_values(B, vdt), narrow)
    assert_fuses(info(M, kind))
    rng = np.random.default_rng(31)
    for k in (3, 8):
        X = np.asfortranarray(rng.uniform(-1, 1, (M.m, k)).astype(xdt))
        Y0 = np.asfortranarray(rng.uniform(-1, 1, (M.n, k)).astype(xdt))
        for alpha, beta in AB:
            Y = Y0.copy(order="F")
            V.mulmat_(Y, V.adjoint(M), X, alpha, beta, engine="vector")
            ref = per_column(M, dev(X), dev(Y0), alpha, beta)
            assert same(torch.from_numpy(np.ascontiguousarray(Y)), ref), (k, alpha, beta)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_knob_off_same_result(forced, kind):
    vdt, xdt, narrow = KINDS[kind]
    forced.setenv("VBC_MM_SLOTS_COL", "0")
    forced.setenv("VBC_SLOT_PLANAR", "0")
    B = pattern("fe120")
    M = with_values(B, random_values(B, vdt), narrow)
    inf = info(M, kind)
    assert_slotted(inf)
    assert not inf["planar_mask"] & BIT
    sweep(M, xdt, lds=(1,), offs=((1, 1),))
    X, Y0 = operands(M, xdt)
    off = fused(M, X, Y0, *AB[-1], 1, 1, 1)
    forced.delenv("VBC_MM_SLOTS_COL")
    N = with_values(B, random_values(B, vdt), narrow)
    assert_fuses(info(N, kind))
    assert same(fused(N, X, Y0, *AB[-1], 1, 1, 1), off)


def test_csc_handle(forced):
    """A SparseMatrixCSC (TrSpMV!) handle keeps one segment per lane slot, the plain form spmm_slots_col covers: bit
    23 is set exactly when the layout is slotted without merge, planar or swept buckets, and the product equals the
    per-column one bit for bit either way."""
    rng = np.random.default_rng(3)
    A = sp.random(500, 700, density=0.02, format="csc", random_state=4, data_rvs=lambda n: rng.uniform(0.25, 1, n))
    A.sort_indices()
    M = V.SparseMatrixCSC(A)
    _LIVE.append(M)
    inf = M.info(trans=True)
    assert inf["slot_bins"] > 0, inf
    want = inf["planar_bins"] == 0 and inf["sweep_bins"] == 0 and inf["bins_t"] == 0
    assert bool(inf["planar_mask"] & BIT) == want, inf
    X, Y0 = operands(M, np.float64, 5)
    for alpha, beta in AB:
        assert same(fused(M, X, Y0, alpha, beta, 1), per_column(M, X, Y0, alpha, beta))
