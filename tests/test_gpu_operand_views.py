"""Every kernel family on operands a caller owns: x / y (X / Y) embedded in a larger allocation, at element offsets
that are not 16-byte aligned, and -- for the multi-RHS kernels -- with a leading dimension larger than the extent
(`view(Y, :, 1:16)` of a wider Julia matrix).  The rest of the suite passes operands torch allocated itself:
256-byte aligned, contiguous, nothing beside them.

Every product checks three things:

1. value: the window of y equals the oracle (float64) exactly, np.array_equal, no tolerance.  x is surrounded by NaN
   (INT64_MIN // 3 for the Int64 kernels), so this also proves that no masked over-read reached an output;
2. stray writes: every element of the y allocation outside the window -- both pads and, for 2-D views, the gap
   columns / rows -- still holds the canary, a fixed NaN bit pattern compared through an integer view (a NaN with
   another payload counts as a change);
3. beta = 0: the window is NaN before an (alpha, 0) product and finite after it.

Exactness: matrix values, x and y0 are integers in [-8, 8] and (alpha, beta) is (1, 0) or (-1, 2), so every
partial sum is an integer.  With max_i (|A||x| + |beta||y0|)_i below 2^24 (fp32 products) or 2^53 (fp64, Int64) no
partial sum in any order rounds, and fp32 / fp64 results equal the float64 oracle bit for bit.
test_inputs_are_exact computes that bound through the oracle for every problem the GPU tests use and needs no GPU:
it is the proof that a mismatch on the GPU is the kernel's.

No operand touches an end of its allocation: PAD (1 MiB) of canary lies on either side, more than any masked
over-read the kernels document.  These tests look for contamination and stray writes, not faults.

Families are forced at small size with the layout knobs of INTEGRATION.md, as each family's own test file does, and
every case first asserts from vbc_info that it got the layout it means to test."""
import functools
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.conftest import golden_matrices, sprand_family
from tests.test_gpu_mfma import _vbc2d_mixed_heights
from tests.test_gpu_narrow_planar import BX_FORMS, FWD_FORMS, KNOBS, ORDERS, mesh, ragged
from tests.test_gpu_planar import expand_runs, sp_blocked
from tests.test_gpu_update import clone, two_value_sets

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
DEV = "cuda:0"

PAD_BYTES = 1 << 20
AB = ((1.0, 0.0), (-1.0, 2.0))
NRHS = (2, 16, 33)
Y_CANARY = {8: 0x7FF80000DEADBEEF, 4: 0x7FC0BEEF}  # quiet NaNs with a payload no arithmetic produces
X_CANARY_INT = -(2 ** 63) // 3
INT_OF = {8: np.int64, 4: np.int32}


# ---------------------------------------------------------------------------------------------------------------
# problems: a matrix with integer values, its inputs and its oracle products (host only)
# ---------------------------------------------------------------------------------------------------------------

PROBLEMS = {}


def problem(name, fp32=False, dirs=(True, False), multi=False, cols=None):
    """Register `fn() -> matrix` under `name`.  fp32: some GPU case runs the problem in Float32 (bound 2^24).
    multi: X and Y0 are matrices of `cols` columns (default max(NRHS))."""
    def deco(fn):
        assert name not in PROBLEMS and (multi or cols is None)
        PROBLEMS[name] = dict(make=fn, limit=2.0 ** 24 if fp32 else 2.0 ** 53, dirs=dirs, multi=multi,
                              cols=(cols or max(NRHS)) if multi else 1)
        return fn
    return deco


def integer_values(B, seed=1):
    """B's pattern with integer values in [-8, 8] (a tenth of them zero), the pattern of test_gpu_update.py."""
    return clone(B, two_value_sets(B, seed)[0])


def oracle_mul(B, val, x, y, alpha, beta, trans):
    """alpha op(B) x + beta y through the oracle in float64, for any of the three matrix types."""
    val = np.ascontiguousarray(val, dtype=np.float64)
    if isinstance(B, V.SparseMatrixCSC):
        assert trans
        A = sp.csc_matrix((val[:len(B.rowval)], B.rowval - 1, B.colptr - 1), shape=(B.m, B.n))
        return alpha * O.trspmv(A, x, np.zeros(B.n)) + beta * y  # integers: exact
    if isinstance(B, V.SparseMatrixVBC):
        R = O.RefVBC(B.m, B.n, B.U, B.W, B.Pi.spl, B.Phi.spl, B.pos, B.idx, B.ofs, val)
    else:
        R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, val)
    return O.mul(R, x, y.copy(), alpha, beta, trans=trans, ref_semantics=False)


class Solved:
    """One problem: the matrix, and per direction x (nx or nx x cols), y0, the oracle's products for both
    (alpha, beta) and the exactness bound max_i (|A||x| + |beta||y0|)_i."""

    def __init__(self, name):
        spec = PROBLEMS[name]
        self.name, self.limit, self.multi = name, spec["limit"], spec["multi"]
        self.B = B = spec["make"]()
        val = np.asarray(B.val, dtype=np.float64)
        assert np.array_equal(val, np.rint(val)) and np.abs(val).max() <= 8
        self.x, self.y0, self.ref, self.bound = {}, {}, {}, {}
        self.cols = cols = spec["cols"]
        for trans in spec["dirs"]:
            rng = np.random.default_rng(zlib.crc32(name.encode()) + int(trans))
            nx, ny = (B.m, B.n) if trans else (B.n, B.m)
            X = rng.integers(-8, 9, (nx, cols)).astype(np.float64)
            Y0 = rng.integers(-8, 9, (ny, cols)).astype(np.float64)
            ref = {ab: np.empty((ny, cols)) for ab in AB}
            bound = 0.0
            for j in range(cols):
                xj, yj = np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y0[:, j])
                for alpha, beta in AB:
                    ref[(alpha, beta)][:, j] = oracle_mul(B, val, xj, yj if beta else np.zeros(ny), alpha, beta, trans)
                bmax = max(abs(b) for _, b in AB)
                bound = max(bound, float(oracle_mul(B, np.abs(val), np.abs(xj), np.abs(yj), 1.0, bmax, trans).max(initial=0)))
            if not self.multi:
                X, Y0, ref = X[:, 0], Y0[:, 0], {ab: r[:, 0] for ab, r in ref.items()}
            self.x[trans], self.y0[trans], self.ref[trans], self.bound[trans] = X, Y0, ref, bound


@functools.lru_cache(maxsize=None)
def solve(name):
    return Solved(name)


# slotted (vbc_slots.h): the 2-dof mesh of test_gpu_slots.py::test_staged_writes (len(y) = 2738: 16 | 8 len, not
# 4 len), 38 nodes a side (16 | 4 len) and the 1-dof mesh (1369: 8 len not a multiple of 16)
for _N, _dof in ((37, 2), (38, 2), (37, 1)):
    problem(f"slotted-N{_N}-dof{_dof}", fp32=True)(
        lambda N=_N, dof=_dof: integer_values(V.synthetic.fe_grid_2d(N, dof=dof)))

# plain planar B'x (vbc_planar.h spmv_planar): len(y) = stripes * w, odd for odd w at 171 stripes and a multiple
# of 4 at 172, so the 16-byte store loops end with and without a tail at every alignment of y
PLANAR_STRIPES = (171, 172)
for _w in range(3, 9):
    for _R in (2, 3):
        for _s in PLANAR_STRIPES:
            problem(f"planar-w{_w}-R{_R}-s{_s}", fp32=True, dirs=(True,))(
                lambda w=_w, R=_R, s=_s: integer_values(ragged(w, R, stripes=s)))
for _dof in (2, 3):  # len(y) = 338 (16 | 8 len, not 4 len) and 507 (odd)
    problem(f"planar-fwd-mesh{_dof}", fp32=True, dirs=(False,))(lambda dof=_dof: integer_values(mesh(dof)))


def bench_matrix(*a):
    import bench
    return bench.build_matrix(*a)


# lane pairs: the ldoor stand-in at two scales, 3174 stripes (len(y) = 9522, 16 | 8 len) and 3237 (9711, odd)
PAIR_SCALES = {"pair-ldoor": 0.01, "pair-ldoor-odd": 0.0102}
for _name, _scale in PAIR_SCALES.items():
    problem(_name)(lambda scale=_scale: integer_values(bench_matrix("ldoor", np.float64, scale)))

# split planar (test_gpu_planar.py::test_split_chunks / test_forward_split, their shapes): 700 stripes (every len(y)
# a multiple of 4) and 701 (odd for the odd widths)
SPLIT_CASES = ((3, 3, 700), (5, 1, 700), (8, 2, 700), (3, 3, 701), (5, 1, 701))
for _w, _R, _L in SPLIT_CASES:
    def _split(w=_w, R=_R, L_=_L):
        base = V.synthetic.vbr_1dvbc(4000, L_, 30000, w, W=8, seed=w + 2)
        return integer_values(expand_runs(base, R, seed=w) if R > 1 else base)
    problem(f"split-w{_w}-R{_R}-L{_L}", fp32=True, dirs=(True,))(_split)
# forward: len(y) = R * rows of the base pattern -- 9000 / 6000 (multiples of 4), 9003 (odd), 6002 (16 | 8 len only)
FSPLIT_CASES = ((3, 3, 3000), (2, 2, 3000), (3, 3, 3001), (2, 2, 3001))
for _w, _R, _m in FSPLIT_CASES:
    def _fsplit(w=_w, R=_R, m=_m):
        rng = np.random.default_rng(10 * w + R)
        base = V.synthetic.vbr_1dvbc(m, 900, 20000, w, W=8, seed=w * R)
        return integer_values(V.SparseMatrix1DVBC[8](sp_blocked(base, R, rng, np.float64), V.EquiChunker(w)))
    problem(f"split-fwd-w{_w}-R{_R}-m{_m}", fp32=True, dirs=(False,))(_fsplit)

# lane streams (test_gpu_lanes.py, its smallest matrices).  A tile holds a multiple of 4 stripes, so only the
# bucket's last tile can end off a 16-byte boundary: 4000 stripes (every len(y) a multiple of 4) and 4001 (odd for
# the odd widths); the runs-of-3 matrix (lane pairs in Float64) at 3000 and 3001 stripes
LANES_CASES = ((3, 4000), (5, 4000), (8, 4000), (3, 4001), (5, 4001))
for _w, _L in LANES_CASES:
    problem(f"lanes-w{_w}-L{_L}", fp32=True, dirs=(True,))(
        lambda w=_w, L_=_L: integer_values(V.synthetic.vbr_1dvbc(9000, L_, 14000, w, W=8, seed=w)))
LANES_RUNS3 = (3000, 3001)
for _L in LANES_RUNS3:
    problem(f"lanes-runs3-L{_L}", fp32=True, dirs=(True,))(
        lambda L_=_L: integer_values(expand_runs(V.synthetic.vbr_1dvbc(6000, L_, 15000, 3, W=8, seed=3), 3, seed=4)))
# forward: len(y) = 3 * 5000 (a multiple of 4) and 3 * 5001 (odd)
FLANES_CASES = ((2, 5000), (3, 5000), (2, 5001), (3, 5001))
for _w, _m in FLANES_CASES:
    def _flanes(w=_w, m=_m):
        rng = np.random.default_rng(w)
        base = V.synthetic.vbr_1dvbc(m, 1500, 24000, w, W=8, seed=3 * w)
        return integer_values(V.SparseMatrix1DVBC[8](sp_blocked(base, 3, rng, np.float64), V.EquiChunker(w)))
    problem(f"lanes-fwd-w{_w}-m{_m}", fp32=True, dirs=(False,))(_flanes)

# the golden corpus under default knobs: the fused small-matrix split, its lane parts, the forward product on Bᵀ
GOLDEN_KEYS = sorted(golden_matrices())
GOLDEN_METHODS = {"strict4": lambda: V.StrictChunker(4),
                  "memory": lambda: V.DynamicTotalChunker(V.model_SparseMatrix1DVBC_memory(), 8)}
for _k in GOLDEN_KEYS:
    for _mn in GOLDEN_METHODS:
        problem(f"golden-{_k}-{_mn}")(
            lambda k=_k, mn=_mn: integer_values(V.SparseMatrix1DVBC[8](golden_matrices()[k]["A"], GOLDEN_METHODS[mn]())))

# row-swept: the 4-wide north-star matrix (30000 x 30000, every len(y) a multiple of 4) and stripes of widths
# 1..8 in turn (30001 x 29989: both lengths odd)
problem("sweep-ns", fp32=True)(lambda: integer_values(V.synthetic.north_star(scale=0.003)))
problem("sweep-w1to8-odd", fp32=True)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(30001, 6665, 66000, np.arange(6665) % 8 + 1, W=8, seed=7)))
# merge: 900 x 4800, and 901 x 4799 (the last stripe 15 wide: both lengths odd)
problem("merge-w16", fp32=True)(lambda: integer_values(V.synthetic.vbr_1dvbc(900, 300, 1800, 16, W=16, seed=16)))
problem("merge-w16-odd", fp32=True)(lambda: integer_values(
    V.synthetic.vbr_1dvbc(901, 300, 1800, np.where(np.arange(300) < 299, 16, 15), W=16, seed=16)))

# CSC: the ldoor stand-in at two scales, len(y) = 9522 (4 len not a multiple of 16) and 10092 (16 | 4 len)
CSC_SCALES = {"csc-ldoor": 0.01, "csc-ldoor-x4": 0.0106}
for _name, _scale in CSC_SCALES.items():
    def _csc(scale=_scale):
        A = V.synthetic.standin("GHS_psdef/ldoor", dtype=np.float64, scale=scale).tocsc()
        A.sort_indices()
        return integer_values(V.SparseMatrixCSC(A))
    problem(_name, fp32=True, dirs=(True,))(_csc)

# 2D VBC: lp_etamacro (400 x 816, multiples of 16 bytes) and GD99_c (105 x 105, odd)
VBC2D_KEYS = ("LPnetlib__lp_etamacro", "Pajek__GD99_c")
for _k in VBC2D_KEYS:
    problem(f"vbc2d-{_k}")(lambda k=_k: integer_values(V.SparseMatrixVBC[4, 4](
        golden_matrices()[k]["A"], V.AlternatingPacker(V.StrictChunker(4), V.StrictChunker(4)))))

for _kind in ("bool", "i32"):
    def _int(kind=_kind):
        A = [t for t in sprand_family(trials=1, kinds=(kind,)) if t[0].startswith(f"{kind}_17x16")][0][1]
        A = A.astype(np.bool_ if kind == "bool" else np.int32)
        B = V.SparseMatrix1DVBC[4](A, V.StrictChunker(4))
        assert B.val.dtype == A.dtype
        return integer_values(B)
    problem(f"int64-{_kind}")(_int)

# multi-RHS: MFMA panels (every width 1..16) and tiles (the structured mesh; tile heights 1..4 in one stripe)
problem("panel-c5", fp32=True, multi=True)(lambda: integer_values(V.synthetic.c5(dtype=np.float64, scale=0.0005)))
problem("panel-w1to16", fp32=True, multi=True)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(700, 48, 1500, np.arange(48) % 16 + 1, W=16, seed=5)))
problem("tiles-c5mesh", fp32=True, multi=True)(lambda: integer_values(bench_matrix("c5-mesh", np.float64, 0.002)))
problem("tiles-heights", fp32=True, multi=True)(lambda: integer_values(_vbc2d_mixed_heights(
    np.random.default_rng(61), 300, 400, 1200, (3, 1, 4, 2, 3), (1, 3, 2, 4, 3), np.float64)))
# the same two generators with odd numbers of rows of X and Y (701 x 409, 783 x 1041); the four above are even
problem("panel-w1to16-odd", fp32=True, multi=True)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(701, 49, 1500, np.arange(49) % 16 + 1, W=16, seed=5)))
problem("tiles-heights-odd", fp32=True, multi=True)(lambda: integer_values(_vbc2d_mixed_heights(
    np.random.default_rng(61), 301, 401, 1200, (3, 1, 4, 2, 3), (1, 3, 2, 4, 3), np.float64)))

# merge layout at compile-time widths (VBC_SLOTS=0, VBC_SWEEP=0; stripes at most 8 wide), 70 columns: the fused
# vector multi-RHS kernel (spmm_ranges / fixup_mm, row-major B'X) and, on column 0, spmv_ranges / fixup.
#   fixed-w1to8, -odd: one merge bin per stored width (the per-bin carry slice and the bin lookup), 700 x 216 and
#     701 x 217 (both extents odd);
#   fixed-long: three 5-wide stripes of about 2100 stored rows each.  A range is one wave's share of a bin's tiles;
#     build_bucket (csrc/vbc_plan_bins.hip) gives a bin nranges = min(round(target_ranges * its share of the entries),
#     (ntiles + 1) / 2) ranges of tiles_per_range = ceil(ntiles / nranges) tiles, and a tile holds rpi * tile_k
#     entries: rpi = 64 / 5 = 12 slots of tile_k = 4 (Float64) / 8 (Float32) entries.  The 6326 entries are 132 /
#     66 tiles; target_ranges is CUs x occupancy x 4 >= 1024 on any gfx950 part, so nranges = 66 / 33 and
#     tiles_per_range = 2: a range holds 96 / 192 entries, every stripe's segment crosses about 21 / 10 range
#     boundaries, and most ranges hold no segment head at all.  Every output of the problem therefore comes from
#     hand_mm / hand_off partials summed by fixup_mm / fixup;
#   fixed-long-w1to8: two stripes of about 660 stored rows for each width 1..8, so every one of the 8 bins has
#     two ranges or more (a range holds at most 2 tiles x 64 slots x 8 entries = 1024 entries, a bin about 1320):
#     ranges of up to 512 entries cut both 660-entry segments, ranges of 1024 the second one.  Each bin's own slice
#     of the carry buffer is written and read back;
#   fixed-empty: 60 stored rows in 48 stripes, some of them empty: the fill list (beta * y, or 0, from fixup_mm).
FIXED_COLS = 70
FIXED = ("fixed-w1to8", "fixed-w1to8-odd", "fixed-long", "fixed-long-w1to8", "fixed-empty")
problem("fixed-w1to8", fp32=True, multi=True, cols=FIXED_COLS)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(700, 48, 1500, np.arange(48) % 8 + 1, W=8, seed=5)))
problem("fixed-w1to8-odd", fp32=True, multi=True, cols=FIXED_COLS)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(701, 49, 1500, np.arange(49) % 8 + 1, W=8, seed=5)))
problem("fixed-long", fp32=True, multi=True, cols=FIXED_COLS)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(4000, 3, 9000, 5, W=8, seed=9)))
problem("fixed-long-w1to8", fp32=True, multi=True, cols=FIXED_COLS)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(3001, 16, 12000, np.arange(16) % 8 + 1, W=8, seed=11)))


@problem("fixed-empty", fp32=True, multi=True, cols=FIXED_COLS)
def _fixed_empty():
    B = V.synthetic.vbr_1dvbc(700, 48, 60, np.arange(48) % 8 + 1, W=8, seed=6)
    empty = np.diff(B.pos) == 0
    assert empty.any() and not empty.all()
    return integer_values(B)


# engine="vector" products that run one SpMV per column: matrices whose B'x layout is not merge-only (a golden
# matrix under default knobs, the slotted mesh) or has a runtime-width bin (16-wide stripes), 5 columns
PERCOL_COLS = 5
PERCOL_GOLDEN = "LPnetlib__lp_blend"
problem("percol-golden", fp32=True, multi=True, cols=PERCOL_COLS)(lambda: integer_values(
    V.SparseMatrix1DVBC[8](golden_matrices()[PERCOL_GOLDEN]["A"], GOLDEN_METHODS["strict4"]())))
problem("percol-slotted", fp32=True, multi=True, cols=PERCOL_COLS)(
    lambda: integer_values(V.synthetic.fe_grid_2d(37, dof=2)))
problem("percol-merge-w16", fp32=True, multi=True, cols=PERCOL_COLS)(
    lambda: integer_values(V.synthetic.vbr_1dvbc(900, 300, 1800, 16, W=16, seed=16)))


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_inputs_are_exact(name):
    """max_i (|A||x| + |beta||y0|)_i < 2^24 (problems some case runs in Float32) or 2^53: every partial sum of every
    product of the problem is an integer that its eltype holds exactly."""
    s = solve(name)
    assert s.bound, name
    for trans, b in s.bound.items():
        print(name, "trans", trans, "bound", b, "limit", s.limit)
        assert b < s.limit, (name, trans, b)
        for r in s.ref[trans].values():
            assert np.array_equal(r, np.rint(r)) and np.abs(r).max(initial=0) <= b


# ---------------------------------------------------------------------------------------------------------------
# the harness: operands embedded in canary
# ---------------------------------------------------------------------------------------------------------------

def _window(buf, pad, off, shape, ld, layout):
    if len(shape) == 1:
        return buf[pad + off: pad + off + shape[0]]
    rows, nrhs = shape
    if layout == "R":
        return buf[pad + off: pad + off + rows * ld].view(rows, ld)[:, :nrhs]
    return buf[pad + off: pad + off + nrhs * ld].view(nrhs, ld)[:, :rows].T


def _extent(shape, ld, layout):
    if len(shape) == 1:
        return shape[0]
    return (shape[0] if layout == "R" else shape[1]) * ld


def embed(a, off, fill, ld=None, layout="R"):
    """(buffer, view): a 1-D device buffer of PAD + off + len + PAD elements of a's eltype whose window
    [PAD + off, PAD + off + len) is `a` and whose every other element is `fill` -- a float (stored in a's eltype)
    or an int (the element's bit pattern; for integer arrays its value).  2-D `a` (rows x nrhs): len = rows * ld
    ("R", row-major, ld > nrhs) or nrhs * ld ("C", column-major, ld > rows); the gap columns / rows hold `fill`."""
    a = np.asarray(a)
    it = INT_OF[a.dtype.itemsize]
    if a.ndim == 2:
        assert ld > (a.shape[1] if layout == "R" else a.shape[0]) or (ld, layout, a.shape[1]) == (16, "R", 16)
    bits = int(np.array(fill, dtype=a.dtype).view(it)) if isinstance(fill, float) else int(fill)
    pad = PAD_BYTES // a.dtype.itemsize
    total = pad + off + _extent(a.shape, ld, layout) + pad
    buf = torch.full((total,), bits, dtype=getattr(torch, np.dtype(it).name), device=DEV)
    buf = buf.view(getattr(torch, a.dtype.name))
    view = _window(buf, pad, off, a.shape, ld, layout)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return buf, view


@functools.lru_cache(maxsize=256)
def _outside(itemsize, off, shape, ld, layout):
    """Boolean device mask of the elements of embed()'s buffer that are not the window."""
    pad = PAD_BYTES // itemsize
    m = torch.ones(pad + off + _extent(shape, ld, layout) + pad, dtype=torch.bool, device=DEV)
    _window(m, pad, off, shape, ld, layout).fill_(False)
    return m


def product_checked(op, x, xoff, y_start, yoff, ref, alpha, beta, what, xbuf=None, ld=(None, None), layout="R",
                    engine="auto", call=None):
    """One product on embedded operands and its three checks.  x, y_start, ref: host arrays in the operand eltype
    (ref in float64).  The product is V.mul_(..., engine=engine), or call(y_view, x_view, alpha, beta) when given.
    Returns the embedded x so that a caller can reuse it."""
    dt = y_start.dtype
    if xbuf is None:
        xbuf = embed(x, xoff, float("nan") if dt.kind == "f" else X_CANARY_INT, ld[0], layout)
    canary = Y_CANARY[dt.itemsize]
    if beta == 0 and dt.kind == "f":
        y_start = np.full_like(y_start, np.nan)
    ybuf, yv = embed(y_start, yoff, canary, ld[1], layout)
    if call is None:
        V.mul_(yv, op, xbuf[1], alpha, beta, engine=engine)
    else:
        call(yv, xbuf[1], alpha, beta)
    got = yv.cpu().numpy()
    if dt.kind == "f":
        assert np.isfinite(got).all(), (what, "non-finite values in the window")
    bad = np.argwhere(got.astype(np.float64) != ref)
    assert len(bad) == 0, (what, "value", len(bad), bad[:4].tolist())
    ibits = ybuf.view(getattr(torch, np.dtype(INT_OF[dt.itemsize]).name))
    stray = (ibits != canary) & _outside(dt.itemsize, yoff, y_start.shape, ld[1], layout)
    nstray = int(stray.sum())
    assert nstray == 0, (what, "stray writes", nstray, (torch.nonzero(stray)[:4, 0] - PAD_BYTES // dt.itemsize - yoff).tolist())
    return xbuf


def offsets(dt):
    return range(4) if np.dtype(dt).itemsize == 4 else range(2)


def fresh(B, dt, narrow=None):
    """A new matrix object (its own handles: the knobs are read when a handle is created) with values in `dt`."""
    vdt = np.float32 if narrow else dt
    M = clone(B, B.val.astype(vdt) if B.val.dtype.kind == "f" else B.val)
    if narrow:
        M.narrow = narrow
    _LIVE.append(M)
    return M


_LIVE = []


@pytest.fixture(autouse=True)
def release_handles():
    """Every matrix fresh() made gives its device memory back when the test ends, passed or failed."""
    yield
    for M in _LIVE:
        M.release()
    _LIVE.clear()


def sweep_vector(M, s, trans, dt, what):
    """Every x offset x y offset x (alpha, beta) of one direction of one handle."""
    dt = np.dtype(dt)
    op = V.adjoint(M) if trans else M
    x, y0 = s.x[trans].astype(dt), s.y0[trans].astype(dt)
    for xo in offsets(dt):
        xbuf = None
        for yo in offsets(dt):
            for alpha, beta in AB:
                xbuf = product_checked(op, x, xo, y0, yo, s.ref[trans][(alpha, beta)], alpha, beta,
                                       (s.name, what, "trans", trans, "x+", xo, "y+", yo, alpha, beta), xbuf)


def setenvs(mp, knobs, clear=()):
    for k in clear:
        mp.delenv(k, raising=False)
    for k, v in knobs.items():
        mp.setenv(k, v)


F32_F64 = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
KINDS = {"f32": (np.float32, None), "f64": (np.float64, None), "narrow": (np.float64, "planar")}


# ---------------------------------------------------------------------------------------------------------------
# SpMV families
# ---------------------------------------------------------------------------------------------------------------

@gpu
@F32_F64
@pytest.mark.parametrize("name", ["slotted-N37-dof2", "slotted-N38-dof2", "slotted-N37-dof1"])
def test_slotted(monkeypatch, name, dt):
    """spmv_slots, both directions: 32-bit and int16 keys, direct (VBC_SLOT_STAGE=0) and LDS-staged y writes."""
    s = solve(name)
    monkeypatch.setenv("VBC_SLOTS", "1")
    for keys in ("0", "2"):
        for stage in ("0", "8"):
            setenvs(monkeypatch, {"VBC_SLOT_KEYS16": keys, "VBC_SLOT_STAGE": stage})
            M = fresh(s.B, dt)
            for trans in (True, False):
                inf = M.info(trans=trans)
                assert inf["slot_bins"] > 0 and inf["sweep_bins"] == 0, inf
                assert inf["planar_bins"] == 0 or not trans, inf  # B'x: spmv_slots, not a planar bucket
                sweep_vector(M, s, trans, dt, ("keys16", keys, "stage", stage))
            M.release()


def check_plain_planar(inf, trans, run, masked, narrow):
    assert inf["planar_split"] == 1 and inf["planar_pair"] == 0, inf
    pm = inf["planar_mask"]
    assert pm & ((1 << 2) | (1 << 3) | (1 << 4) | (1 << 5) | (1 << 6) | (1 << 11)) == 0, pm
    if trans:
        assert inf["planar_bins"] >= 1 and inf["planar_run"] == run, inf
        assert (pm & 1) == int(masked), pm
        assert bool(pm & (1 << 14)) == bool(narrow), pm
    else:
        assert inf["slot_bins"] >= 1 and inf["fwd_run"] == run, inf
        assert ((pm >> 1) & 1) == int(masked), pm
        assert bool(pm & (1 << 15)) == bool(narrow), pm


PLANAR_CASES = [(w, run, k) for w in range(3, 9) for run in (1, 2, 3) for k in KINDS
                if not (w == 4 and k == "f32")]  # Float32 rows of width 4 are one 16-byte lane vector: not planar


@gpu
@pytest.mark.parametrize("w,run,kind", PLANAR_CASES)
def test_planar_bx(monkeypatch, w, run, kind):
    """spmv_planar<T, W, ...>: widths 3..8, row runs 1 / 2 / 3 (run 1: the run-3 matrix under VBC_SLOT_RUNS=0),
    natural / masked / sorted order, 32-bit and int16 keys, staged and direct writes; Float32, Float64 and the
    narrow-planar instantiation (Float32 values, Float64 operands), at 171 and 172 stripes."""
    dt, narrow = KINDS[kind]
    setenvs(monkeypatch, KNOBS)
    monkeypatch.setenv("VBC_SLOT_RUNS", "1" if run > 1 else "0")
    for stripes in PLANAR_STRIPES:
        s = solve(f"planar-w{w}-R{2 if run == 2 else 3}-s{stripes}")
        for order, keys, stage in BX_FORMS:
            setenvs(monkeypatch, ORDERS[order], clear=("VBC_SLOTS_SORT", "VBC_PLANAR_MASK", "VBC_SLOT_STAGE"))
            monkeypatch.setenv("VBC_SLOT_KEYS16", keys)
            if stage is not None:
                monkeypatch.setenv("VBC_SLOT_STAGE", stage)
            M = fresh(s.B, dt, narrow)
            check_plain_planar(M.info(trans=True, compute=L.dtype_code(np.dtype(dt))), True, run, order == "masked", narrow)
            sweep_vector(M, s, True, dt, (order, "keys16", keys, "stage", stage))
            M.release()


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name,dof", [("planar-fwd-mesh2", 2), ("planar-fwd-mesh3", 3)])
def test_planar_forward_runs(monkeypatch, name, dof, kind):
    """spmv_planar_fwd<T, W, R, ...> on the dof-2 and dof-3 mesh operators: every order, key form and write form
    of test_gpu_narrow_planar.py::FWD_FORMS; Float32, Float64 and narrow-planar."""
    dt, narrow = KINDS[kind]
    setenvs(monkeypatch, KNOBS)
    monkeypatch.delenv("VBC_SLOTS")  # (the forward run layout has its own padding rule)
    s = solve(name)
    for knobs, masked in FWD_FORMS:
        setenvs(monkeypatch, knobs, clear=("VBC_SLOTS_PAD", "VBC_SLOT_KEYS16", "VBC_SLOT_STAGE", "VBC_PLANAR_MASK",
                                           "VBC_FWD_MIN_ROWS"))
        M = fresh(s.B, dt, narrow)
        check_plain_planar(M.info(trans=False, compute=L.dtype_code(np.dtype(dt))), False, dof, masked, narrow)
        sweep_vector(M, s, False, dt, tuple(knobs.items()))
        M.release()


@gpu
@pytest.mark.parametrize("name", list(PAIR_SCALES))
def test_lane_pairs_both_directions(monkeypatch, name):
    """spmv_planar_pair, B'x and forward (DOT form), on the ldoor stand-in."""
    setenvs(monkeypatch, {"VBC_PLANAR_PAIR": "2", "VBC_PLANAR_SPLIT": "0"})
    s = solve(name)
    M = fresh(s.B, np.float64)
    assert M.info(trans=True)["planar_pair"] == 1, M.info(trans=True)
    assert M.info(trans=False)["planar_mask"] & 2048, M.info(trans=False)
    for trans in (True, False):
        sweep_vector(M, s, trans, np.float64, "pair")


@gpu
@F32_F64
@pytest.mark.parametrize("w,R,stripes", SPLIT_CASES)
def test_split_planar(monkeypatch, w, R, stripes, dt):
    """Split planar product (P = 2 / 4 / 8 waves per chunk, partial sums met in LDS), affine and table-mapped
    outputs."""
    s = solve(f"split-w{w}-R{R}-L{stripes}")
    monkeypatch.setenv("VBC_SLOTS", "1")
    for P in ("2", "4", "8"):
        for sort in ("0", "2"):
            setenvs(monkeypatch, {"VBC_PLANAR_SPLIT": P, "VBC_SLOTS_SORT": sort})
            M = fresh(s.B, dt)
            inf = M.info(trans=True)
            assert inf["planar_bins"] == 1 and inf["planar_split"] == int(P) and inf["planar_run"] == R, inf
            sweep_vector(M, s, True, dt, ("P", P, "sort", sort))
            M.release()


@gpu
@F32_F64
@pytest.mark.parametrize("w,R,rows", FSPLIT_CASES)
def test_split_forward(monkeypatch, w, R, rows, dt):
    """spmv_planar_fwd_split (planar_mask bit 3), P = 2 / 4 / 8."""
    s = solve(f"split-fwd-w{w}-R{R}-m{rows}")
    monkeypatch.setenv("VBC_SLOTS_PAD", "100")  # keep the natural order (the split product needs it)
    for P in ("2", "4", "8"):
        monkeypatch.setenv("VBC_PLANAR_SPLIT", P)
        M = fresh(s.B, dt)
        inf = M.info(trans=False)
        assert inf["fwd_run"] == R and inf["planar_mask"] & 8, inf
        sweep_vector(M, s, False, dt, ("P", P))
        M.release()


LANES_KNOBS = {"VBC_SLOTS": "1", "VBC_PLANAR_LANES": "1", "VBC_PLANAR_SPLIT": "0"}


@gpu
@F32_F64
@pytest.mark.parametrize("name,run", [(f"lanes-w{w}-L{n}", 1) for w, n in LANES_CASES] +
                         [(f"lanes-runs3-L{n}", 3) for n in LANES_RUNS3])
def test_lane_streams_bx(monkeypatch, name, run, dt):
    """spmv_planar_lanes (planar_mask bit 2), one lane or a lane pair per stream (VBC_LANES_PAIR)."""
    s = solve(name)
    setenvs(monkeypatch, LANES_KNOBS)
    for pair in ("0", "1"):
        monkeypatch.setenv("VBC_LANES_PAIR", pair)
        M = fresh(s.B, dt)
        inf = M.info(trans=True)
        assert inf["planar_mask"] & 4 and inf["planar_run"] == run, inf
        # lane pairs: Float64 3-wide runs of 3 only
        assert inf["planar_pair"] == int(pair == "1" and run == 3 and dt == np.float64), inf
        sweep_vector(M, s, True, dt, ("lanes_pair", pair))
        M.release()


@gpu
@F32_F64
@pytest.mark.parametrize("w,rows", FLANES_CASES)
def test_lane_streams_forward(monkeypatch, w, rows, dt):
    """Forward lane streams (planar_mask bit 4): node blocks of 3 output rows transposed into the lane-stream
    layout, 3 outputs in runs of w.  VBC_LANES_PAIR=1 gives the Float64 w = 3 case a lane pair per stream
    (spmv_pair_lanes); vbc_info reports planar_pair for B'x buckets only, so the pair form is not asserted here."""
    s = solve(f"lanes-fwd-w{w}-m{rows}")
    setenvs(monkeypatch, LANES_KNOBS)
    for pair in ("0", "1"):
        monkeypatch.setenv("VBC_LANES_PAIR", pair)
        M = fresh(s.B, dt)
        inf = M.info(trans=False)
        assert inf["planar_mask"] & 16 and inf["fwd_run"] == 3, inf
        sweep_vector(M, s, False, dt, ("fwd lanes_pair", pair))
        M.release()


@gpu
def test_golden_fused_split_lane_parts_forward_on_transpose():
    """The reference's corpus under default knobs: the fused small-matrix split (planar_mask bit 5), its lane parts
    (bit 6) and the forward product on C = Bᵀ (bit 8), each hit at least once over the set."""
    hit = {5: 0, 6: 0, 8: 0}
    for k in GOLDEN_KEYS:
        for mn in GOLDEN_METHODS:
            s = solve(f"golden-{k}-{mn}")
            M = fresh(s.B, np.float64)
            for trans in (True, False):
                pm = M.info(trans=trans)["planar_mask"]
                for b in (5, 6) if trans else (8,):
                    hit[b] += bool(pm & (1 << b))
                sweep_vector(M, s, trans, np.float64, "default knobs")
            M.release()
    assert all(hit.values()), hit


@gpu
@F32_F64
@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("name", ["sweep-ns", "sweep-w1to8-odd"])
def test_row_swept(monkeypatch, name, pack, dt):
    """The row-swept layout, both directions, packed and unpacked keys."""
    setenvs(monkeypatch, {"VBC_SWEEP": "1", "VBC_SWEEP_PACK": pack})
    s = solve(name)
    M = fresh(s.B, dt)
    for trans in (True, False):
        assert M.info(trans=trans)["sweep_bins"] > 0, M.info(trans=trans)
        sweep_vector(M, s, trans, dt, ("pack", pack))


@gpu
@F32_F64
@pytest.mark.parametrize("name", ["merge-w16", "merge-w16-odd"])
def test_merge_runtime_width(monkeypatch, name, dt):
    """The merge layout (VBC_SLOTS=0) on 16-wide stripes: the runtime-width kernels."""
    monkeypatch.setenv("VBC_SLOTS", "0")
    s = solve(name)
    M = fresh(s.B, dt)
    assert M.info(trans=True)["bins_t"] > 0 and M.info(trans=False)["bins_f"] > 0
    for trans in (True, False):
        sweep_vector(M, s, trans, dt, "merge")


class Column:
    """Column j of a multi-RHS problem as a single-vector problem (what sweep_vector takes)."""

    def __init__(self, s, j=0):
        self.name = s.name
        self.x = {t: np.ascontiguousarray(X[:, j]) for t, X in s.x.items()}
        self.y0 = {t: np.ascontiguousarray(Y[:, j]) for t, Y in s.y0.items()}
        self.ref = {t: {ab: np.ascontiguousarray(r[:, j]) for ab, r in refs.items()} for t, refs in s.ref.items()}


MERGE_FIXED_KNOBS = {"VBC_SLOTS": "0", "VBC_SWEEP": "0", "VBC_FWD_T": "0"}


def check_merge_fixed(M, trans):
    """The handle's layout is merge-only and every stripe at most 8 wide: every bin has a compile-time width."""
    assert np.diff(M.Phi.spl).max() <= 8
    inf = M.info(trans=trans)
    assert inf["bins_t" if trans else "bins_f"] > 0, inf
    assert inf["slot_bins"] == 0 and inf["sweep_bins"] == 0 and inf["planar_bins"] == 0, inf


@gpu
@F32_F64
@pytest.mark.parametrize("name", ["fixed-w1to8", "fixed-w1to8-odd", "fixed-long", "fixed-long-w1to8"])
def test_merge_fixed_width(monkeypatch, name, dt):
    """spmv_ranges<T, 0 | 1, K, P> at compile-time widths, both directions (the forward product as merge bins of
    B, VBC_FWD_T=0): the load-free writer at beta = 0, the reading one at beta = 2, and fixup on segments that
    span ranges (fixed-long: every B'x output).  Stored widths are the padded ones -- Float64 1, 2, 4, 4, 5, 6, 8,
    8 and Float32 1, 2, 4, 4, 5, 8, 8, 8 for stripes 1..8 wide -- so wkey 3 and 7 (and Float32 6) have no bin."""
    setenvs(monkeypatch, MERGE_FIXED_KNOBS)
    s = Column(solve(name))
    M = fresh(solve(name).B, dt)
    for trans in (True, False):
        check_merge_fixed(M, trans)
        sweep_vector(M, s, trans, dt, "merge, fixed widths")


@gpu
@pytest.mark.parametrize("name", list(CSC_SCALES))
def test_csc_trspmv_blocked_columns_fp32(name):
    """TrSpMV! on the CSC handle of the ldoor stand-in, Float32: columns blocked into stripes (L < n)."""
    s = solve(name)
    M = fresh(s.B, np.float32)
    inf = M.info(trans=True)
    assert inf["L"] < M.n, inf
    sweep_vector(M, s, True, np.float32, "csc")


@gpu
@pytest.mark.parametrize("key", VBC2D_KEYS)
def test_vbc2d(key):
    """2D VBC (4 x 4 blocks), both directions."""
    s = solve(f"vbc2d-{key}")
    M = fresh(s.B, np.float64)
    assert M.info(trans=True)["K"] > 0
    for trans in (True, False):
        sweep_vector(M, s, trans, np.float64, "2d")


@gpu
@pytest.mark.parametrize("kind", ["bool", "i32"])
def test_int64(kind):
    """The exact Int64 kernels on Bool and Int32 values; x is surrounded by INT64_MIN // 3."""
    s = solve(f"int64-{kind}")
    M = fresh(s.B, np.int64)
    for trans in (True, False):
        assert M.info(trans=trans, compute=L.VBC_I64)["dtype"] == L.VBC_I64
        sweep_vector(M, s, trans, np.int64, kind)


# ---------------------------------------------------------------------------------------------------------------
# multi-RHS families
# ---------------------------------------------------------------------------------------------------------------

def sweep_multi(M, s, trans, dt, what):
    """nrhs 2 / 16 / 33, row- and column-major, every base offset pair, leading dimensions extent + 1 and
    extent + 5 (row-major Float32 also 70 elements: a row stride above 255 bytes, the tile kernel's non-buffer
    path), both (alpha, beta); then 16 row-major right-hand sides at ld = 16 (the contiguous case) at base
    offsets 0 and 1, which select the tile kernel's store forms fast_dw = 1 / 2 and 0."""
    dt = np.dtype(dt)
    op = V.adjoint(M) if trans else M
    X, Y0 = s.x[trans].astype(dt), s.y0[trans].astype(dt)
    nx, ny = X.shape[0], Y0.shape[0]
    for nrhs in NRHS:
        Xn, Yn = np.ascontiguousarray(X[:, :nrhs]), np.ascontiguousarray(Y0[:, :nrhs])
        refs = {ab: np.ascontiguousarray(r[:, :nrhs]) for ab, r in s.ref[trans].items()}
        for layout in ("R", "C"):
            extra = (1, 5) + ((70 - nrhs,) if layout == "R" and dt.itemsize == 4 else ())
            for e in extra:
                ld = (nrhs + e, nrhs + e) if layout == "R" else (nx + e, ny + e)
                for xo in offsets(dt):
                    xbuf = None
                    for yo in offsets(dt):
                        for alpha, beta in AB:
                            xbuf = product_checked(op, Xn, xo, Yn, yo, refs[(alpha, beta)], alpha, beta,
                                                   (s.name, what, "trans", trans, "nrhs", nrhs, layout, "ld", ld,
                                                    "X+", xo, "Y+", yo, alpha, beta), xbuf, ld, layout)
    X16, Y16 = np.ascontiguousarray(X[:, :16]), np.ascontiguousarray(Y0[:, :16])
    for off in (0, 1):
        for alpha, beta in AB:
            product_checked(op, X16, off, Y16, off, np.ascontiguousarray(s.ref[trans][(alpha, beta)][:, :16]), alpha,
                            beta, (s.name, what, "trans", trans, "16 contiguous", "+", off, alpha, beta), None,
                            (16, 16), "R")


MULTI = pytest.mark.parametrize("nobuf", ["0", "1"], ids=["buf", "nobuf"])
TRANS = pytest.mark.parametrize("trans", [True, False], ids=["BtX", "BX"])


@gpu
@MULTI
@TRANS
@F32_F64
@pytest.mark.parametrize("name", ["panel-c5", "panel-w1to16", "panel-w1to16-odd"])
def test_multi_rhs_panels(monkeypatch, name, dt, trans, nobuf):
    """spmm_panel (MFMA): buffer and 64-bit addressing (VBC_PANEL_NOBUF=1), B'X and B X."""
    setenvs(monkeypatch, {"VBC_PANEL_TILES": "0", "VBC_PANEL_NOBUF": nobuf})
    s = solve(name)
    M = fresh(s.B, dt)
    inf = M.info(trans=trans, multi=True)
    assert inf["bins_m"] > 0 and not inf["planar_mask"] & 512, inf
    sweep_multi(M, s, trans, dt, ("panels", "nobuf", nobuf))


@gpu
@MULTI
@TRANS
@F32_F64
@pytest.mark.parametrize("name", ["tiles-c5mesh", "tiles-heights", "tiles-heights-odd"])
def test_multi_rhs_tiles(monkeypatch, name, dt, trans, nobuf):
    """spmm_tiles (planar_mask bit 9): the structured 3 x 3 node-tile mesh, and tile heights 1..4 in one stripe
    (slot rows past a tile's height are loaded and masked)."""
    setenvs(monkeypatch, {"VBC_PANEL_TILES": "1", "VBC_PANEL_NOBUF": nobuf})
    s = solve(name)
    M = fresh(s.B, dt)
    inf = M.info(trans=trans, multi=True)
    assert inf["bins_m"] > 0 and inf["planar_mask"] & 512, inf
    sweep_multi(M, s, trans, dt, ("tiles", "nobuf", nobuf))


# ---------------------------------------------------------------------------------------------------------------
# engine="vector": the fused vector kernel, the per-column branches, vbc_mul_mat_ex on an Int64 handle
# ---------------------------------------------------------------------------------------------------------------

FUSED_NRHS = (2, 16, 17, 64, 65, 70)  # NR = 16 (2, 16), NR = 64 (17, 64), a second chunk of 1 and of 6 columns


def sweep_fused(M, s, dt, what):
    """Row-major B'X, engine="vector": every nrhs of FUSED_NRHS at ld = nrhs + 1 and nrhs + 5, X and Y at base
    offsets 0 and 1, both (alpha, beta); then 16 contiguous right-hand sides (ld = 16) at both offsets."""
    dt = np.dtype(dt)
    op = V.adjoint(M)
    X, Y0 = s.x[True].astype(dt), s.y0[True].astype(dt)
    cases = [(nrhs, nrhs + e) for nrhs in FUSED_NRHS for e in (1, 5)] + [(16, 16)]
    for nrhs, ld in cases:
        Xn, Yn = np.ascontiguousarray(X[:, :nrhs]), np.ascontiguousarray(Y0[:, :nrhs])
        refs = {ab: np.ascontiguousarray(r[:, :nrhs]) for ab, r in s.ref[True].items()}
        for xo in (0, 1):
            xbuf = None
            for yo in (0, 1):
                for alpha, beta in AB:
                    xbuf = product_checked(op, Xn, xo, Yn, yo, refs[(alpha, beta)], alpha, beta,
                                           (s.name, what, "nrhs", nrhs, "ld", ld, "X+", xo, "Y+", yo, alpha, beta),
                                           xbuf, (ld, ld), "R", engine="vector")


@gpu
@F32_F64
@pytest.mark.parametrize("name", FIXED)
def test_fused_vector_multi_rhs(monkeypatch, name, dt):
    """spmm_ranges<T, 16 | 64, K> and fixup_mm<T, 16 | 64>: row-major B'X with engine="vector" on a merge-only
    layout of compile-time widths (mul_mat_device's `fused` branch).  One bin per stored width (each bin its own
    slice of the carry buffer, a quarter as long at NR = 16), segments that span ranges (fixed-long: hand_mm and
    fixup_mm produce every output), empty stripes (fixed-empty: fixup_mm's fill list), a second 64-column chunk."""
    setenvs(monkeypatch, MERGE_FIXED_KNOBS)
    s = solve(name)
    assert s.cols == FIXED_COLS >= max(FUSED_NRHS)
    M = fresh(s.B, dt)
    check_merge_fixed(M, True)
    sweep_fused(M, s, dt, "fused vector")


PERCOL_NRHS = (2, 5)


def sweep_per_column(M, s, trans, dt, what, layouts=("R", "C")):
    """engine="vector", nrhs 2 and 5, row- and column-major, ld = extent + 1 and extent + 5, X and Y at base offsets
    0 and 1, both (alpha, beta).  Row-major: the columns go through the handle's contiguous temporaries by strided
    copies (beta = 2 reads Y through them), so the gap columns of Y must keep the canary."""
    dt = np.dtype(dt)
    op = V.adjoint(M) if trans else M
    X, Y0 = s.x[trans].astype(dt), s.y0[trans].astype(dt)
    nx, ny = X.shape[0], Y0.shape[0]
    for nrhs in PERCOL_NRHS:
        Xn, Yn = np.ascontiguousarray(X[:, :nrhs]), np.ascontiguousarray(Y0[:, :nrhs])
        refs = {ab: np.ascontiguousarray(r[:, :nrhs]) for ab, r in s.ref[trans].items()}
        for layout in layouts:
            for e in (1, 5):
                ld = (nrhs + e, nrhs + e) if layout == "R" else (nx + e, ny + e)
                for xo in (0, 1):
                    xbuf = None
                    for yo in (0, 1):
                        for alpha, beta in AB:
                            xbuf = product_checked(op, Xn, xo, Yn, yo, refs[(alpha, beta)], alpha, beta,
                                                   (s.name, what, "trans", trans, "nrhs", nrhs, layout, "ld", ld,
                                                    "X+", xo, "Y+", yo, alpha, beta), xbuf, ld, layout,
                                                   engine="vector")


# problem -> (knobs, what vbc_info must say about the B'x handle)
PERCOL_CASES = {
    "percol-golden": ({}, lambda inf: inf["slot_bins"] > 0),                     # default knobs: not merge-only
    "percol-slotted": ({"VBC_SLOTS": "1"}, lambda inf: inf["slot_bins"] > 0),
    # merge-only, but the 16-wide stripes' bin has a runtime width (wkey = 0): no fused kernel
    "percol-merge-w16": ({"VBC_SLOTS": "0"}, lambda inf: inf["bins_t"] > 0 and inf["slot_bins"] == 0 and
                         inf["sweep_bins"] == 0 and inf["planar_bins"] == 0),
}


@gpu
@TRANS
@F32_F64
@pytest.mark.parametrize("name", list(PERCOL_CASES))
def test_vector_engine_per_column(monkeypatch, name, dt, trans):
    """vbc_mul_mat without panels and without the fused kernel: one SpMV per column.  Row-major operands go through
    staging buffers 2 / 3 (copy2d), column-major ones are passed column by column; B'X on layouts the fused kernel
    does not read, and B X (always per column)."""
    knobs, layout_ok = PERCOL_CASES[name]
    setenvs(monkeypatch, knobs)
    s = solve(name)
    M = fresh(s.B, dt)
    inf = M.info(trans=True)
    assert layout_ok(inf), inf
    if name == "percol-merge-w16":
        assert np.diff(M.Phi.spl).max() == 16
    assert M.info(trans=trans)["bins_m"] == 0  # (the vector handle: no panel layout)
    sweep_per_column(M, s, trans, dt, "per column")


@gpu
@F32_F64
def test_vector_engine_column_major_on_fixed_merge(monkeypatch, dt):
    """Column-major operands never take the fused kernel, even on the layout it reads: the per-column loop on
    fixed-w1to8-odd, both directions."""
    setenvs(monkeypatch, MERGE_FIXED_KNOBS)
    s = solve("fixed-w1to8-odd")
    M = fresh(s.B, dt)
    for trans in (True, False):
        check_merge_fixed(M, trans)
        sweep_per_column(M, s, trans, dt, "column-major on the fused layout", layouts=("C",))


def dense_int(B):
    """B as a dense Int64 array, column by column through the oracle (small integer values: exact)."""
    val = np.asarray(B.val, dtype=np.float64)
    D = np.empty((B.m, B.n), np.int64)
    for j in range(B.n):
        e = np.zeros(B.n)
        e[j] = 1.0
        D[:, j] = oracle_mul(B, val, e, np.zeros(B.m), 1.0, 0.0, False).astype(np.int64)
    return D


def int64_operands(B, trans, nrhs=3):
    rng = np.random.default_rng(64 + int(trans))
    nx, ny = (B.m, B.n) if trans else (B.n, B.m)
    return rng.integers(-8, 9, (nx, nrhs)).astype(np.int64), rng.integers(-8, 9, (ny, nrhs)).astype(np.int64)


@gpu
@pytest.mark.parametrize("layout", ["R", "C"])
@pytest.mark.parametrize("kind", ["bool", "i32"])
def test_mul_mat_ex_int64(kind, layout):
    """vbc_mul_mat_ex on an Int64 handle, called directly (the Python mirror loops over the columns itself): 3
    right-hand sides, (alpha, beta) = (3, -2), against numpy's Int64 product (test_gpu_eltypes.py::expected)."""
    B = solve(f"int64-{kind}").B
    M = fresh(B, np.int64)
    D = dense_int(B)
    alpha, beta = 3, -2
    for trans in (True, False):
        h = M.handle(0, trans, compute=L.VBC_I64)
        assert M.info(trans=trans, compute=L.VBC_I64)["dtype"] == L.VBC_I64
        X, Y0 = int64_operands(B, trans)
        ref = alpha * ((D.T if trans else D) @ X) + beta * Y0  # Int64, wrapping
        nx, ny, nrhs = X.shape[0], Y0.shape[0], X.shape[1]
        for e in (1, 5):
            ld = (nrhs + e, nrhs + e) if layout == "R" else (nx + e, ny + e)

            def call(yv, xv, a, b, ld=ld):
                stream = torch.cuda.current_stream(yv.device).cuda_stream
                L.check(L.lib().vbc_mul_mat_ex(h, int(trans), nrhs, xv.data_ptr(), L.VBC_I64, ld[0], nx, yv.data_ptr(),
                                               L.VBC_I64, ld[1], ny, float(a), float(b), L.VBC_MEM_DEVICE, stream,
                                               L.VBC_MAT_ROWMAJOR if layout == "R" else 0), "vbc_mul_mat_ex")

            for xo in (0, 1):
                for yo in (0, 1):
                    product_checked(None, X, xo, Y0, yo, ref, alpha, beta,
                                    (kind, "mul_mat_ex", "trans", trans, layout, "ld", ld, "X+", xo, "Y+", yo),
                                    None, ld, layout, call=call)


@gpu
@pytest.mark.parametrize("layout", ["R", "C"])
def test_mul_mat_ex_int64_refuses_int32_y(layout):
    """Y_dtype = VBC_I32 on an Int64 handle: VBC_UNSUPPORTED_DTYPE, and no element of Y's allocation changes."""
    B = solve("int64-i32").B
    M = fresh(B, np.int64)
    for trans in (True, False):
        h = M.handle(0, trans, compute=L.VBC_I64)
        X, Y0 = int64_operands(B, trans)
        nx, ny, nrhs = X.shape[0], Y0.shape[0], X.shape[1]
        ld = (nrhs + 1, nrhs + 1) if layout == "R" else (nx + 1, ny + 1)
        _, xv = embed(X, 1, X_CANARY_INT, ld[0], layout)
        ybuf, yv = embed(Y0.astype(np.int32), 1, Y_CANARY[4], ld[1], layout)
        before = ybuf.clone()
        stream = torch.cuda.current_stream(yv.device).cuda_stream
        st = L.lib().vbc_mul_mat_ex(h, int(trans), nrhs, xv.data_ptr(), L.VBC_I64, ld[0], nx, yv.data_ptr(), L.VBC_I32,
                                    ld[1], ny, 3.0, -2.0, L.VBC_MEM_DEVICE, stream,
                                    L.VBC_MAT_ROWMAJOR if layout == "R" else 0)
        assert st == L.VBC_UNSUPPORTED_DTYPE, (st, L.last_error())
        torch.cuda.synchronize()
        assert torch.equal(ybuf, before), (layout, trans)
        assert np.array_equal(yv.cpu().numpy(), Y0.astype(np.int32))
