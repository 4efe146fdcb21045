"""Column-major multi-RHS forward product B X fused over forward row runs and forward lane pairs
(spmm_planar_fwd_col, csrc/vbc_planar_fwd_mmc.h; spmm_pair_col with DOT, csrc/vbc_planar_mmc.h; vbc.h planar_mask
bit 25).

The operands are what a Julia Matrix is: X[i + j * ldx], Y[i + j * ldy].  A lane (or lane pair) adds the dot
products of its output rows block by block in stored order, the fused kernels keep accumulators of their own per
right-hand side and flush with the single-vector kernels' expressions, so every column of the fused product is, bit
for bit, the single-vector product mul_(y, B, x, alpha, beta) of that column on the same handle, whichever write
path (staged or direct) that product took: the comparisons with the per-column products below are np.array_equal on
the raw bits, no tolerance.  The oracle comparisons use integer inputs (every partial sum exact), again without
tolerance.

Every case sets VBC_MM_FWD_COL=1 and asserts through info(trans=False) the layout it means to test.  The inputs are
the smallest the suite has for these layouts: the 13 x 13 mesh of tests/test_gpu_narrow_planar.py (169 node
segments: three chunks of 64, the last one partial) under its FWD_FORMS, the sp_blocked construction of
tests/test_gpu_planar.py::test_forward_row_runs at 150 node rows (three chunks again, 22 segments in the last), and
the 300-node stiffness operand of tests/test_gpu_narrow_pairs.py (one node empty) under FWD_PAIR."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_mm_slots_col import bits, dev, same, view2d
from tests.test_gpu_narrow_pairs import FWD_PAIR
from tests.test_gpu_narrow_planar import FWD_FORMS, KNOBS, mesh
from tests.test_gpu_planar import _to_csc, sp_blocked

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
BIT22, BIT23, BIT24, BIT = 1 << 22, 1 << 23, 1 << 24, 1 << 25
NRHS = (2, 3, 4, 5, 8, 9)
AB = ((1.0, 0.0), (-0.5, 2.0))  # the single-vector product's FASTE / staged writes, and the path that reads y
# value dtype, vector dtype, B.narrow on a run layout, B.narrow on a lane-pair layout
KINDS = {"f32": (np.float32, np.float32, False, None), "f64": (np.float64, np.float64, False, False),
         "narrow": (np.float32, np.float64, "planar", "pairs")}
PAIR_KINDS = ("f64", "narrow")
WR = ((2, 2), (2, 3), (3, 2), (3, 3), (4, 2), (4, 3))
# forward row runs at any size: no fused small-matrix launch, no split product, no lane pairs, no lane streams
# (tests/test_gpu_narrow_planar.py's KNOBS without VBC_SLOTS: the forward run layout has its own padding rule)
RUNS = {k: v for k, v in KNOBS.items() if k != "VBC_SLOTS"}
PAIRS = dict(FWD_PAIR, VBC_SMALL_FUSE="0")
LAYOUT_KNOBS = sorted(set(KNOBS) | set(PAIRS) | {
    "VBC_SLOTS_SORT", "VBC_PLANAR_MASK", "VBC_PLANAR_MASK_PAIR", "VBC_SLOT_KEYS16", "VBC_SLOT_STAGE", "VBC_SLOT_RUNS",
    "VBC_SLOTS_PAD", "VBC_FWD_MIN_ROWS", "VBC_FWD_T", "VBC_LANES_PAIR", "VBC_MM_SLOTS", "VBC_MM_SLOTS_COL",
    "VBC_MM_PLANAR_COL", "VBC_MM_FWD_COL"})

_LIVE = []


@pytest.fixture(autouse=True)
def release_handles():
    yield
    for M in _LIVE:
        M.release()
    _LIVE.clear()


@pytest.fixture
def knobs(monkeypatch):
    """knobs(env, ...): exactly these layout knobs, and VBC_MM_FWD_COL=1 unless one of them sets it."""
    def set_(*envs):
        for k in LAYOUT_KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("VBC_MM_FWD_COL", "1")
        for env in envs:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
    return set_


@pytest.fixture
def capture_stream():
    """A non-blocking HIP stream of this test's own, destroyed afterwards, instead of torch.cuda.Stream(): that call
    hands out torch's pooled streams in turn, so taking some here would change which pooled streams every later test
    of the session gets (tests/test_gpu_mm_planar_col.py has the whole reason)."""
    hip = L.lib()  # (libvbc links the HIP runtime the process already uses: its symbols resolve through this handle)
    raw = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0  # hipStreamNonBlocking
    yield torch.cuda.ExternalStream(raw.value, device=DEV)
    torch.cuda.synchronize()
    assert hip.hipStreamDestroy(raw) == 0


def make(B, kind, pair=False, val=None, updatable=False):
    """A new matrix object (its own handles: the knobs are read when a handle is created) with B's pattern."""
    vdt, xdt, narrow, narrow_pair = KINDS[kind]
    val = B.val if val is None else val
    M = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, np.asarray(val).astype(vdt))
    if pair and narrow_pair or not pair and narrow:
        M.narrow = narrow_pair if pair else narrow
    if updatable:
        M.updatable = "narrow" if kind == "narrow" else True
    _LIVE.append(M)
    return M


def info(M, kind, trans=False):
    return M.info(trans=trans, compute=L.dtype_code(np.dtype(KINDS[kind][1])))


def assert_forward(inf, R, pair=False, kind=None, mask=None):
    """The forward layout: row runs of R (or the lane pairs), one wave per range, chunk rows, on B's own layout."""
    assert inf["fwd_run"] == R, inf
    assert inf["planar_mask"] & ((1 << 3) | (1 << 4) | (1 << 8)) == 0, inf  # split, lane streams, forward on C = Bᵀ
    assert bool(inf["planar_mask"] & (1 << 11)) == pair, inf  # forward lane pairs
    assert inf["bins_f"] == 0 and inf["sweep_bins"] == 0 and inf["slot_bins"] >= 1, inf
    if mask is not None:
        assert ((inf["planar_mask"] >> 1) & 1) == int(mask), inf
    if kind is not None:  # Float32 stored values exactly on the narrow kind (bit 15 runs, bit 17 pairs)
        assert bool(inf["planar_mask"] & (1 << (17 if pair else 15))) == (kind == "narrow"), inf
        assert not inf["planar_mask"] & (1 << (15 if pair else 17)), inf


def assert_fuses(inf, R, **kw):
    assert_forward(inf, R, **kw)
    assert inf["planar_mask"] & BIT, inf


def per_column(M, X, Y0, alpha, beta):
    """nrhs single-vector products mul_(y, M, x, alpha, beta) on contiguous vectors: the reference of every test."""
    Y = torch.empty_like(Y0)
    for j in range(X.shape[1]):
        y = Y0[:, j].contiguous()
        V.mul_(y, M, X[:, j].contiguous(), alpha, beta)
        Y[:, j] = y
    return Y


def fused(M, X, Y0, alpha, beta, ld_extra=0, xoff=0, yoff=0, cols=None):
    """The engine="vector" forward product on column-major views; returns the window of Y, and checks that nothing
    else of the Y allocation and nothing of the X allocation changed (NaN around the operands, in the ld - rows tail
    of every column and in the columns >= k of a wider allocation: the callers compare with finite references)."""
    m, k = Y0.shape
    n = X.shape[0]
    xbuf, Xv = view2d(n, k, n + ld_extra, xoff, X.dtype, float("nan"), cols)
    Xv.copy_(X)
    xbefore = bits(xbuf)
    ybuf, Yv = view2d(m, k, m + ld_extra, yoff, Y0.dtype, float("nan"), cols)
    if beta != 0:
        Yv.copy_(Y0)
    assert Xv.stride(0) == 1 and Yv.stride(0) == 1 and Yv.stride(1) == m + ld_extra
    canary = bits(ybuf).copy()
    V.mulmat_(Yv, M, Xv, alpha, beta, engine="vector")
    got = Yv.clone()
    after = bits(ybuf).copy()
    win = torch.zeros_like(ybuf, dtype=torch.bool)
    win[16 + yoff: 16 + yoff + k * (m + ld_extra)].view(k, m + ld_extra)[:, :m] = True
    out = ~win.cpu().numpy()
    assert np.array_equal(after[out], canary[out]), "stray write outside the live rows x k window of Y"
    assert np.array_equal(bits(xbuf), xbefore), "X changed"
    return got


def operands(M, xdt, k=max(NRHS), seed=11):
    rng = np.random.default_rng(seed)
    return dev(rng.uniform(-1, 1, (M.n, k)).astype(xdt)), dev(rng.uniform(-1, 1, (M.m, k)).astype(xdt))


def check(M, xdt, ks=(2, 5), views=((1, 1, 0),), ab=AB, seed=11):
    """fused == per column on the raw bits, for every k, (ld_extra, xoff, yoff) and (alpha, beta)."""
    X, Y0 = operands(M, xdt, max(ks), seed)
    for alpha, beta in ab:
        ref = per_column(M, X, Y0, alpha, beta)
        for k in ks:
            for ld, xo, yo in views:
                got = fused(M, X[:, :k], Y0[:, :k], alpha, beta, ld, xo, yo)
                assert same(got, ref[:, :k]), (k, ld, xo, yo, alpha, beta)
    return ref


NODES = 150  # node rows of the blocked matrices: three chunks of 64 segments, 22 in the last


class _Pattern:
    """What sp_blocked takes: an object whose to_csc() is the m x n pattern to expand."""
    def __init__(self, D):
        self.D = D

    def to_csc(self):
        return self.D


@functools.lru_cache(maxsize=None)
def blocked(w, R, empty=()):
    """tests/test_gpu_planar.py::test_forward_row_runs's matrix at NODES node rows and 60 w-wide stripes (about 6
    blocks per node row, none to 15 or so: ranges shorter than one pipeline stage beside longer ones): every row of
    the base pattern expanded into R rows with values of their own; the node rows in `empty` store nothing.
    float32 values."""
    rng = np.random.default_rng(100 * w + R)
    base = V.synthetic.vbr_1dvbc(NODES, 60, 900, w, W=8, dtype=np.float32, seed=w + R)
    D = sp.lil_matrix(sp.csr_matrix(_to_csc(base)))
    for i in empty:
        D[i, :] = 0.0
    D = D.tocsr()
    D.eliminate_zeros()
    return V.SparseMatrix1DVBC[8](sp_blocked(_Pattern(D), R, rng, np.float32), V.EquiChunker(w))


def assert_blocked_size(inf, R):
    assert inf["m"] == NODES * R and -(-inf["m"] // (64 * R)) == 3 and (inf["m"] // R) % 64 == 22, inf


@functools.lru_cache(maxsize=None)
def mesh_matrix(dof):
    return mesh(dof)


@functools.lru_cache(maxsize=None)
def pair_matrix():
    """tests/test_gpu_narrow_pairs.py's fwd_matrix: a 3-dof stiffness operand of 300 nodes, node 10 coupling to
    nothing (an empty stripe and three empty output rows of B)."""
    A = V.synthetic.fe_stiffness_3d(900, 40000, 3, np.float32).tolil()
    A[30:33, :] = 0.0
    A[:, 30:33] = 0.0
    A = A.tocsc()
    A.eliminate_zeros()
    return V.SparseMatrix1DVBC[8](A.T.tocsc(), V.StrictChunker(8))


def runs_env(form=0):
    return dict(RUNS, **FWD_FORMS[form][0])


def pair_env(keys="2", mask="1"):
    env = dict(PAIRS, VBC_SLOT_KEYS16=keys, VBC_PLANAR_MASK=mask)
    if mask == "0":
        env["VBC_SLOTS_PAD"] = "100"  # (admits the natural order's padding at this size)
    return env


# ---------------------------------------------------------------------------------------------------------------
# 1. bit 25
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bit25_set_on_forward_runs(knobs, kind):
    knobs(runs_env())
    assert_fuses(info(make(mesh_matrix(3), kind), kind), 3, kind=kind, mask=False)


@pytest.mark.parametrize("kind", PAIR_KINDS)
def test_bit25_set_on_forward_pairs(knobs, kind):
    knobs(pair_env())
    assert_fuses(info(make(pair_matrix(), kind, pair=True), kind), 3, pair=True, kind=kind, mask=True)


@pytest.mark.parametrize("off", ["VBC_MM_FWD_COL", "VBC_MM_SLOTS_COL", "VBC_MM_SLOTS"])
@pytest.mark.parametrize("pair", [False, True])
def test_bit25_clear_with_a_knob_off(knobs, pair, off):
    """... and the knob changes nothing else: the forward handle's other fields and bits, and the whole vbc_info of
    the B'x handle (bits 22 - 24 are its), are those of a handle created without VBC_MM_FWD_COL."""
    B = pair_matrix() if pair else mesh_matrix(2)
    env = pair_env() if pair else runs_env()
    knobs(env, {off: "0"})
    M = make(B, "f64", pair=pair)
    inf = info(M, "f64")
    assert_forward(inf, 3 if pair else 2, pair=pair)
    assert not inf["planar_mask"] & BIT, inf
    knobs(env)
    on, on_t = info(make(B, "f64", pair=pair), "f64"), info(make(B, "f64", pair=pair), "f64", trans=True)
    knobs(env, {"VBC_MM_FWD_COL": "0"})
    off_, off_t = info(make(B, "f64", pair=pair), "f64"), info(make(B, "f64", pair=pair), "f64", trans=True)
    assert on["planar_mask"] == off_["planar_mask"] | BIT and not off_["planar_mask"] & BIT
    assert {k: v for k, v in on.items() if k != "planar_mask"} == {k: v for k, v in off_.items() if k != "planar_mask"}
    assert on_t == off_t and not on_t["planar_mask"] & BIT
    assert on["planar_mask"] & (BIT22 | BIT23 | BIT24) == off_["planar_mask"] & (BIT22 | BIT23 | BIT24)


@functools.lru_cache(maxsize=None)
def mixed_widths():
    return V.synthetic.vbr_1dvbc(400, 300, 1400, np.arange(300) % 8 + 1, W=8, seed=7)


@functools.lru_cache(maxsize=None)
def two_widths():
    """blocked(.., 2)'s construction (NODES node rows in runs of 2 output rows) over 60 stripes of widths 2 and 3 in
    turn: two forward width buckets, each node-blocked."""
    rng = np.random.default_rng(77)
    w = np.arange(60) % 2 + 2
    base = V.synthetic.vbr_1dvbc(NODES, 60, 900, w, W=8, dtype=np.float32, seed=77)
    At = sp_blocked(_Pattern(sp.csr_matrix(_to_csc(base))), 2, rng, np.float32)
    return V.SparseMatrix1DVBC[8](At, V.SplitPartition(np.concatenate([[1], 1 + np.cumsum(w)]).astype(np.int64)))


# name: (matrix, knobs, what info(trans=False) must show of the layout)
REFUSED = {
    "split": (lambda: mesh_matrix(3), dict(RUNS, VBC_PLANAR_SPLIT="4"),
              lambda i: i["fwd_run"] == 3 and i["planar_mask"] & 8 and not i["planar_mask"] & (16 | 256)),
    "lanes": (lambda: mesh_matrix(3), dict(RUNS, VBC_PLANAR_LANES="1"),
              lambda i: i["fwd_run"] == 3 and i["planar_mask"] & 16 and not i["planar_mask"] & (8 | 256)),
    "forward-on-transposed": (mixed_widths, {"VBC_FWD_T": "2"}, lambda i: i["planar_mask"] & 256),
    # the closest a multi-bucket forward (f_scale) comes to a fusing layout: the planner builds row runs only for a
    # one-bucket forward, so two width buckets always bring slotted or merge buckets with them.  The node-blocked
    # matrix below fuses with one stripe width (test_runs_widths: (2, 2) and (3, 2)); with the two widths side by
    # side it has two forward buckets, no merge bucket among them, and keeps the per-column path
    "multi-bucket": (two_widths, dict(RUNS, VBC_FWD_T="0", VBC_SLOTS="1"),
                     lambda i: not i["planar_mask"] & 256 and i["bins_f"] == 0 and i["slot_bins"] >= 2),
    "multi-bucket-mixed": (mixed_widths, {"VBC_FWD_T": "0"},
                           lambda i: not i["planar_mask"] & 256 and i["bins_f"] + i["slot_bins"] >= 2),
}


def refused(knobs, name):
    matrix, env, layout = REFUSED[name]
    knobs(env)
    M = make(matrix(), "f64")
    inf = info(M, "f64")
    assert layout(inf), inf
    assert not inf["planar_mask"] & BIT, inf
    return M


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_bit25_clear_on_refused_layouts(knobs, name):
    """... and the engine="vector" product of such a handle still equals the per-column one."""
    M = refused(knobs, name)
    check(M, np.float64, ks=(3,))


def test_bit25_clear_on_int64(knobs):
    knobs(runs_env())
    B = mesh_matrix(3)
    M = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, np.rint(B.val * 8).astype(np.int64))
    _LIVE.append(M)
    inf = M.info(trans=False, compute=L.VBC_I64)
    assert inf["dtype"] == L.VBC_I64, inf
    assert not inf["planar_mask"] & (BIT | BIT22 | BIT23 | BIT24), inf


# ---------------------------------------------------------------------------------------------------------------
# 2. bitwise against column by column
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,R", WR)
def test_runs_widths(knobs, w, R):
    """Every (w, R) in the three value kinds; k = 2 is one NR = 2 launch, k = 5 an NR = 4 launch and an NR = 2 launch
    of one live column."""
    knobs(runs_env())
    B = blocked(w, R)
    for kind in sorted(KINDS):
        M = make(B, kind)
        inf = info(M, kind)
        assert_fuses(inf, R, kind=kind)
        assert_blocked_size(inf, R)
        check(M, KINDS[kind][1], seed=10 * w + R)
        M.release()


@pytest.mark.parametrize("dof", [2, 3])
@pytest.mark.parametrize("form", range(len(FWD_FORMS)))
def test_mesh_forms(knobs, dof, form):
    """The mesh under FWD_FORMS: both key forms, staged and direct single-vector writes, one range per chunk, the
    masked chunk-local order and the length-sorted order with its y-offset table."""
    knobs(runs_env(form))
    B = mesh_matrix(dof)
    for kind in sorted(KINDS):
        M = make(B, kind)
        assert_fuses(info(M, kind), dof, kind=kind, mask=FWD_FORMS[form][1])
        check(M, KINDS[kind][1], seed=dof + form)
        M.release()


VIEWS = tuple((ld, xo, yo) for ld in (0, 1, 5) for xo, yo in ((0, 0), (1, 0), (0, 1), (1, 1)))


@pytest.mark.parametrize("kind,w,R", [("f32", 3, 2), ("f64", 3, 3), ("narrow", 4, 3)])
def test_runs_nrhs_ld_offsets(knobs, kind, w, R):
    knobs(runs_env())
    M = make(blocked(w, R), kind)
    assert_fuses(info(M, kind), R, kind=kind)
    check(M, KINDS[kind][1], ks=NRHS, views=VIEWS)


@pytest.mark.parametrize("keys", ["0", "2"])
@pytest.mark.parametrize("mask", ["0", "1"])
def test_pair_forms(knobs, keys, mask):
    """The lane-pair kernel with DOT over both key forms, the natural and the masked order, in fp64 and on Float32
    stored values; node 10 of the matrix is empty (its three output rows get beta * y, or 0, in every column)."""
    knobs(pair_env(keys, mask))
    B = pair_matrix()
    for kind in PAIR_KINDS:
        M = make(B, kind, pair=True)
        assert_fuses(info(M, kind), 3, pair=True, kind=kind, mask=mask == "1")
        ref = check(M, np.float64, ks=(2, 3, 5), seed=int(keys) + int(mask))
        X, Y0 = operands(M, np.float64, 5, seed=int(keys) + int(mask))
        assert same(ref[30:33], 2.0 * Y0[30:33])
        assert not fused(M, X, Y0, 1.0, 0.0, 1, 0, 1)[30:33].any()
        M.release()


@pytest.mark.parametrize("kind", PAIR_KINDS)
def test_pair_nrhs_ld_offsets(knobs, kind):
    knobs(pair_env())
    M = make(pair_matrix(), kind, pair=True)
    assert_fuses(info(M, kind), 3, pair=True, kind=kind)
    check(M, np.float64, ks=NRHS, views=VIEWS)


# ---------------------------------------------------------------------------------------------------------------
# 3. against the oracle (integer inputs: exact)
# ---------------------------------------------------------------------------------------------------------------

def check_oracle(M, B, val, xdt, k=7):
    R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, np.asarray(val, np.float64))
    rng = np.random.default_rng(23)
    X = rng.integers(-8, 9, (B.n, k)).astype(xdt)
    Y0 = rng.integers(-8, 9, (B.m, k)).astype(xdt)
    for alpha, beta in ((1.0, 0.0), (-1.0, 2.0)):
        got = fused(M, dev(X), dev(Y0), alpha, beta, 3, 1, 1).cpu().numpy().astype(np.float64)
        want = np.stack([O.mul(R, X[:, j].astype(np.float64), Y0[:, j].astype(np.float64), alpha, beta,
                               ref_semantics=False) for j in range(k)], axis=1)
        assert np.array_equal(got, want), (alpha, beta)


def integer_values(B, seed=1):
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 9, len(B.val)) * rng.choice([-1, 1], len(B.val))
    v[rng.permutation(len(v))[: len(v) // 10]] = 0
    return v.astype(np.float32)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_oracle_exact_runs(knobs, kind):
    knobs(runs_env())
    B = blocked(3, 2, empty=(5, 70, 140))
    val = integer_values(B)
    M = make(B, kind, val=val)
    assert_fuses(info(M, kind), 2, kind=kind)
    check_oracle(M, B, val, KINDS[kind][1])


@pytest.mark.parametrize("kind", PAIR_KINDS)
def test_oracle_exact_pairs(knobs, kind):
    knobs(pair_env())
    B = pair_matrix()
    val = integer_values(B)
    M = make(B, kind, pair=True, val=val)
    assert_fuses(info(M, kind), 3, pair=True, kind=kind)
    check_oracle(M, B, val, np.float64)


# ---------------------------------------------------------------------------------------------------------------
# 4. operand safety and special values, 5. output rows with no entries
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,pair", [("f32", False), ("f64", False), ("narrow", False), ("f64", True), ("narrow", True)])
def test_wider_allocation_and_nan_canaries(knobs, kind, pair):
    """k columns inside an allocation of 8 whose other columns, column tails and surroundings hold NaN: none of it is
    read into a result or overwritten (fused() checks every element outside the window), for k below, at and above
    the chunk of 4; beta = 0 overwrites a Y of NaN."""
    knobs(pair_env() if pair else runs_env())
    M = make(pair_matrix() if pair else blocked(4, 2), kind, pair=pair)
    assert_fuses(info(M, kind), 3 if pair else 2, pair=pair, kind=kind)
    X, Y0 = operands(M, KINDS[kind][1], 6)
    for alpha, beta in AB:
        ref = per_column(M, X, Y0, alpha, beta)
        assert torch.isfinite(ref).all()
        for k in (1, 3, 4, 6):
            assert same(fused(M, X[:, :k], Y0[:, :k], alpha, beta, 3, 1, 1, cols=8), ref[:, :k]), (k, alpha, beta)
    got = fused(M, X, torch.full_like(Y0, float("nan")), 1.0, 0.0, 3, 1, 1, cols=8)
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_nonfinite_rows_of_x(knobs, pair, masked):
    """Inf / NaN in single rows of X: bitwise the per-column result (padding blocks add nothing by a select in both)."""
    knobs(pair_env(mask="1" if masked else "0") if pair else runs_env(4 if masked else 0))
    B = pair_matrix() if pair else mesh_matrix(3)
    M = make(B, "f64", pair=pair)
    assert_fuses(info(M, "f64"), 3, pair=pair, mask=masked)
    X, Y0 = operands(M, np.float64, 5)
    X[0, :] = float("inf")
    X[B.n // 3, 1] = float("nan")
    X[B.n - 1, 3] = -float("inf")
    for alpha, beta in AB:
        got = fused(M, X, Y0, alpha, beta, 2, 1, 0)
        assert same(got, per_column(M, X, Y0, alpha, beta))
        assert not torch.isfinite(got).all() and torch.isfinite(got).any()


@pytest.mark.parametrize("pair", [False, True])
def test_special_stored_values_narrow_against_wide(knobs, pair):
    """Float32 NaN, +-0.0, +-Inf, a subnormal and FLT_MAX among the stored values: the fused product on the narrow
    handle has the bits of the fused and of the per-column product on the wide handle."""
    knobs(pair_env() if pair else runs_env())
    B = pair_matrix() if pair else blocked(3, 3)
    nval = int(B.ofs[-1]) - 1
    v = B.val.copy()
    fi = np.finfo(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max,
                        -fi.max, fi.tiny], np.float32)
    v[np.random.default_rng(8).choice(nval, 4 * len(special), replace=False)] = np.tile(special, 4)
    N, W = make(B, "narrow", pair=pair, val=v), make(B, "f64", pair=pair, val=v)
    assert_fuses(info(N, "narrow"), 3, pair=pair, kind="narrow")
    assert_fuses(info(W, "f64"), 3, pair=pair, kind="f64")
    rng = np.random.default_rng(9)
    X, Y0 = dev(rng.uniform(0.5, 1.0, (B.n, 5))), dev(rng.uniform(-1, 1, (B.m, 5)))
    for alpha, beta in AB:
        got, wide = fused(N, X, Y0, alpha, beta, 1, 1, 1), per_column(W, X, Y0, alpha, beta)
        assert torch.isnan(wide).any() and torch.isinf(wide).any()
        assert same(got, wide) and same(fused(W, X, Y0, alpha, beta, 1, 1, 1), wide), (alpha, beta)


@pytest.mark.parametrize("w,R", [(2, 3), (4, 2)])
@pytest.mark.parametrize("form", [0, 4])
def test_output_rows_without_entries(knobs, w, R, form):
    """Node rows that store nothing, one of them in the partial last chunk: beta * y, or 0, in every column."""
    knobs(runs_env(form))
    empty = (5, 70, 140)
    B = blocked(w, R, empty=empty)
    rows = np.concatenate([np.arange(R * i, R * i + R) for i in empty])
    assert _to_csc(B).tocsr()[rows].nnz == 0
    for kind in sorted(KINDS):
        M = make(B, kind)
        assert_fuses(info(M, kind), R, kind=kind, mask=FWD_FORMS[form][1])
        xdt = KINDS[kind][1]
        ref = check(M, xdt, ks=(3, 8), seed=w)
        X, Y0 = operands(M, xdt, 8, seed=w)
        assert same(ref[rows], (Y0[rows] * 2.0))  # (alpha, beta) = (-0.5, 2): exactly 2 y
        zero = fused(M, X, Y0, 1.0, 0.0, 2, 1, 1)
        assert not zero[rows].any() and zero.any()
        M.release()


# ---------------------------------------------------------------------------------------------------------------
# 6. graph capture, 7. value updates, host operands, the paths the knob leaves alone
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,pair", [("f32", False), ("f64", False), ("narrow", False), ("f64", True), ("narrow", True)])
def test_graph_captured_on_first_use(knobs, capture_stream, kind, pair):
    """The fused product allocates nothing and uses no side stream, so its first call on a fresh handle may be a
    captured one: no eager product of any kind precedes the capture."""
    knobs(pair_env() if pair else runs_env())
    xdt = KINDS[kind][1]
    M = make(pair_matrix() if pair else blocked(3, 3, empty=(5, 70, 140)), kind, pair=pair)
    assert_fuses(info(M, kind), 3, pair=pair, kind=kind)  # (the handle is created here: a create allocates)
    X, Y0 = operands(M, xdt, 5)
    _, Xv = view2d(M.n, 5, M.n + 1, 1, X.dtype, float("nan"))
    _, Yv = view2d(M.m, 5, M.m + 3, 0, X.dtype, float("nan"))
    Xv.copy_(X)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=capture_stream):
        V.mulmat_(Yv, M, Xv, 1.0, 0.0, engine="vector")
    for r in range(3):  # the graph's first launch, then 2 replays with new X
        if r:
            X = operands(M, xdt, 5, seed=100 + r)[0]
            Xv.copy_(X)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(Yv, per_column(M, X, Y0, 1.0, 0.0)), r
    del g  # (before the fixture destroys the stream it was captured on)


@pytest.mark.parametrize("kind,pair", [("f32", False), ("f64", False), ("narrow", False), ("f64", True), ("narrow", True)])
def test_update_then_fused(knobs, kind, pair):
    knobs(pair_env() if pair else runs_env(4))
    B = pair_matrix() if pair else mesh_matrix(2)
    v2 = np.random.default_rng(6).uniform(-1, 1, len(B.val)).astype(np.float32)
    M = make(B, kind, pair=pair, updatable=True)
    assert_fuses(info(M, kind), 3 if pair else 2, pair=pair, kind=kind)
    X, Y0 = operands(M, KINDS[kind][1], 5)
    first = fused(M, X, Y0, -0.5, 2.0)
    M.update_values(v2.astype(KINDS[kind][0]))
    N = make(B, kind, pair=pair, val=v2)
    assert_fuses(info(N, kind), 3 if pair else 2, pair=pair, kind=kind)
    got, want = fused(M, X, Y0, -0.5, 2.0), fused(N, X, Y0, -0.5, 2.0)
    assert same(got, want) and not same(got, first)
    assert same(got, per_column(N, X, Y0, -0.5, 2.0))


@pytest.mark.parametrize("kind,pair", [("f32", False), ("f64", False), ("narrow", False), ("f64", True)])
def test_host_operands(knobs, kind, pair):
    """numpy order="F" operands: staged into packed device buffers, the fused product there, copied back."""
    knobs(pair_env() if pair else runs_env())
    xdt = KINDS[kind][1]
    M = make(pair_matrix() if pair else blocked(2, 2, empty=(5, 70, 140)), kind, pair=pair)
    assert_fuses(info(M, kind), 3 if pair else 2, pair=pair, kind=kind)
    rng = np.random.default_rng(31)
    for k in (3, 6):
        X = np.asfortranarray(rng.uniform(-1, 1, (M.n, k)).astype(xdt))
        Y0 = np.asfortranarray(rng.uniform(-1, 1, (M.m, k)).astype(xdt))
        for alpha, beta in AB:
            Y = Y0.copy(order="F")
            V.mulmat_(Y, M, X, alpha, beta, engine="vector")
            ref = per_column(M, dev(X), dev(Y0), alpha, beta)
            assert same(torch.from_numpy(np.ascontiguousarray(Y)), ref), (k, alpha, beta)


@pytest.mark.parametrize("pair", [False, True])
def test_other_paths_unchanged_against_knob_off(knobs, pair):
    """The fused forward product, row-major forward operands and every transposed product (single vector, column-
    and row-major) of a handle created under the knob have the bits of a handle created with VBC_MM_FWD_COL=0."""
    B = pair_matrix() if pair else mesh_matrix(3)
    env = pair_env() if pair else runs_env()
    out = {}
    for knob in ("1", "0"):
        knobs(env, {"VBC_MM_FWD_COL": knob})
        M = make(B, "f64", pair=pair)
        inf = info(M, "f64")
        assert_forward(inf, 3, pair=pair)
        assert bool(inf["planar_mask"] & BIT) == (knob == "1")
        X, Y0 = operands(M, np.float64, 5)  # X: n x 5, Y0: m x 5
        res = [fused(M, X, Y0, *AB[-1], 1, 1, 1)]
        for alpha, beta in AB:
            Y = Y0.clone()  # C-contiguous (m, k): row-major operands
            V.mulmat_(Y, M, X.contiguous(), alpha, beta, engine="vector")
            assert same(Y, per_column(M, X, Y0, alpha, beta))
            res.append(Y)
            Yt = X.clone()  # transposed: X' = Y0 (m x 5), Y' = X (n x 5), row-major ...
            V.mulmat_(Yt, V.adjoint(M), Y0.contiguous(), alpha, beta, engine="vector")
            res.append(Yt)
            _, Yc = view2d(M.n, 5, M.n + 1, 1, X.dtype, float("nan"))  # ... and column-major
            _, Xc = view2d(M.m, 5, M.m + 2, 0, X.dtype, float("nan"))
            Yc.copy_(X)
            Xc.copy_(Y0)
            V.mulmat_(Yc, V.adjoint(M), Xc, alpha, beta, engine="vector")
            assert same(Yc, Yt)
            res.append(Yc.clone())
            y = X[:, 0].contiguous()
            V.mul_(y, V.adjoint(M), Y0[:, 0].contiguous(), alpha, beta)
            assert same(y, Yt[:, 0])
            res.append(y)
        out[knob] = res
    assert len(out["1"]) == len(out["0"]) and all(same(a, b) for a, b in zip(out["1"], out["0"]))
