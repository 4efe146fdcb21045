"""Column-major multi-RHS B'X fused over the planar and the lane-pair layout (spmm_planar_col / spmm_pair_col,
csrc/vbc_planar_mmc.h; vbc.h planar_mask bit 24).

The operands are what a Julia Matrix is: X[i + j * ldx], Y[i + j * ldy].  A lane (or lane pair) folds its stripe
serially in stored row order, the fused kernels keep accumulators of their own per right-hand side and flush with
the single-vector kernels' expressions, so every column of the fused product is, bit for bit, the single-vector
product of that column on the same handle, whichever write path (staged or direct) that product took: the
comparisons with the per-column products below are np.array_equal on the raw bits, no tolerance.  The oracle
comparisons use integer inputs (every partial sum exact), again without tolerance.

Every case sets VBC_MM_PLANAR_COL=1 and asserts through info() the layout it means to test.  The forced layouts are
those of tests/test_gpu_narrow_planar.py (plain planar: 170 ragged stripes over m = 300, three chunks of 64, the
last one partial) and tests/test_gpu_narrow_pairs.py (lane pairs: 85 stripes, three chunks of 32); the operand views
are those of tests/test_gpu_mm_slots_col.py (NaN around the operands, in every column's ld - rows tail and in the
columns >= nr of a wider allocation)."""
import ctypes
import functools

import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_mm_slots_col import bits, dev, fused, per_column, same, view2d
from tests.test_gpu_narrow_pairs import BX_FORMS as PAIR_FORMS
from tests.test_gpu_narrow_pairs import PAIR
from tests.test_gpu_narrow_planar import BX_FORMS, KNOBS, ORDERS, ragged

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
BIT22, BIT23, BIT = 1 << 22, 1 << 23, 1 << 24
NRHS = (2, 3, 4, 5, 8, 9)
AB = ((1.0, 0.0), (-0.5, 2.0))  # the single-vector product's FASTE / staged writes, and the path that reads y
# value dtype, vector dtype, B.narrow on a plain planar layout, B.narrow on a lane-pair layout
KINDS = {"f32": (np.float32, np.float32, False, None), "f64": (np.float64, np.float64, False, False),
         "narrow": (np.float32, np.float64, "planar", "pairs")}
PAIR_KINDS = ("f64", "narrow")
LAYOUT_KNOBS = sorted(set(KNOBS) | set(PAIR) | {
    "VBC_SLOTS_SORT", "VBC_PLANAR_MASK", "VBC_PLANAR_MASK_PAIR", "VBC_SLOT_KEYS16", "VBC_SLOT_STAGE", "VBC_SLOT_RUNS",
    "VBC_SLOTS_PAD", "VBC_LANES_PAIR", "VBC_MM_SLOTS", "VBC_MM_SLOTS_COL", "VBC_MM_PLANAR_COL", "VBC_KSPLIT"})

_LIVE = []


@pytest.fixture(autouse=True)
def release_handles():
    yield
    for M in _LIVE:
        M.release()
    _LIVE.clear()


@pytest.fixture
def knobs(monkeypatch):
    """knobs(env, ...): exactly these layout knobs, and VBC_MM_PLANAR_COL=1 unless one of them sets it."""
    def set_(*envs):
        for k in LAYOUT_KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("VBC_MM_PLANAR_COL", "1")
        for env in envs:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
    return set_


@pytest.fixture
def capture_stream():
    """A non-blocking HIP stream of this test's own, destroyed afterwards, instead of torch.cuda.Stream(): that call
    hands out torch's 32 pooled streams in turn, each bound to one of the process's few hardware queues at its first
    use, so taking some here would change which pair of pooled streams every later test of the session gets --
    tests/test_gpu_stream_order.py needs its two consecutive streams on different hardware queues."""
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


def info(M, kind):
    return M.info(trans=True, compute=L.dtype_code(np.dtype(KINDS[kind][1])))


def assert_planar(inf, pair=False, kind=None, run=None, mask=None, slotted=False):
    """The B'x layout: planar buckets of the forms the fused kernels cover (one wave per range, chunk rows), no swept
    and no merge bucket; slotted buckets beside them only where the case means to have them."""
    assert inf["planar_bins"] >= 1 and inf["bins_t"] == 0 and inf["sweep_bins"] == 0, inf
    assert inf["planar_split"] == 1 and inf["planar_pair"] == int(pair), inf
    assert inf["planar_mask"] & ((1 << 2) | (1 << 5) | (1 << 6)) == 0, inf  # lane streams, fused split, cut stripes
    if run is not None:
        assert inf["planar_run"] == run, inf
    if mask is not None:
        assert (inf["planar_mask"] & 1) == int(mask), inf
    if kind is not None:  # Float32 stored values exactly on the narrow kind (bit 14 plain, bit 16 pairs)
        assert bool(inf["planar_mask"] & (1 << (16 if pair else 14))) == (kind == "narrow"), inf
    assert inf["slot_bins"] > inf["planar_bins"] if slotted else True, inf


def assert_fuses(inf, **kw):
    assert_planar(inf, **kw)
    assert inf["planar_mask"] & BIT, inf
    assert not inf["planar_mask"] & (BIT22 | BIT23), inf


def assert_fuses_w(inf, kind, w, run, **kw):
    """assert_fuses, but for fp32 w = 4: a row is exactly one 16-B lane vector, which the planner keeps in the plain
    slotted form whatever VBC_SLOT_PLANAR says (slot_planar(), csrc/vbc_plan_bins.hip).  There the product is
    spmm_slots_col's (bit 23), and the case still compares a fused product with the per-column one."""
    if kind == "f32" and w == 4:
        assert inf["planar_bins"] == 0 and inf["slot_bins"] >= 1 and inf["bins_t"] == 0 and inf["sweep_bins"] == 0, inf
        assert inf["planar_mask"] & BIT23 and not inf["planar_mask"] & BIT, inf
    else:
        assert_fuses(inf, kind=kind, run=run, **kw)


def operands(M, xdt, k=max(NRHS), seed=11):
    rng = np.random.default_rng(seed)
    return dev(rng.uniform(-1, 1, (M.m, k)).astype(xdt)), dev(rng.uniform(-1, 1, (M.n, k)).astype(xdt))


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


@functools.lru_cache(maxsize=None)
def plain_matrix(w, R, empty=()):
    return ragged(w, R, empty=empty)


@functools.lru_cache(maxsize=None)
def pair_matrix(empty=(), seed=1):
    return ragged(3, 3, stripes=85, empty=empty, seed=seed)


def plain_env(order="natural", keys="2", stage=None, run=3):
    env = dict(KNOBS, **ORDERS[order])
    env.update({"VBC_SLOT_KEYS16": keys, "VBC_SLOT_RUNS": "1" if run > 1 else "0"})
    if stage is not None:
        env["VBC_SLOT_STAGE"] = stage
    return env


def pair_env(order=None, keys="2", stage=None):
    env = dict(PAIR, **(order or {}))
    env["VBC_SLOT_KEYS16"] = keys
    if stage is not None:
        env["VBC_SLOT_STAGE"] = stage
    return env


# ---------------------------------------------------------------------------------------------------------------
# 1. bit 24
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bit24_set_on_plain_planar(knobs, kind):
    knobs(plain_env())
    assert_fuses(info(make(plain_matrix(5, 3), kind), kind), kind=kind, run=3)


@pytest.mark.parametrize("kind", PAIR_KINDS)
def test_bit24_set_on_lane_pairs(knobs, kind):
    knobs(pair_env())
    assert_fuses(info(make(pair_matrix(), kind, pair=True), kind), pair=True, kind=kind, run=3)


@pytest.mark.parametrize("off", ["VBC_MM_PLANAR_COL", "VBC_MM_SLOTS_COL", "VBC_MM_SLOTS"])
@pytest.mark.parametrize("pair", [False, True])
def test_bit24_clear_with_a_knob_off(knobs, pair, off):
    knobs(pair_env() if pair else plain_env(), {off: "0"})
    M = make(pair_matrix() if pair else plain_matrix(5, 3), "f64", pair=pair)
    inf = info(M, "f64")
    assert_planar(inf, pair=pair)
    assert not inf["planar_mask"] & (BIT | BIT22 | BIT23), inf


def mesh(dof=3, N=14):
    return V.synthetic.fe_grid_2d(N, dof=dof, W=8, dtype=np.float64, seed=7)


@functools.lru_cache(maxsize=None)
def planar_and_merge():
    """3-wide stripes of 10 rows each (uniform: planar under VBC_SLOT_PLANAR=1) beside 1-wide stripes of 0 to ~120
    rows (the padding of the natural order exceeds VBC_SLOTS_PAD and no other order is allowed: merge layout)."""
    rng = np.random.default_rng(41)
    m, L3, L1 = 4000, 1500, 400
    w = np.concatenate([np.full(L3, 3), np.full(L1, 1)]).astype(np.int64)
    cnt = np.concatenate([np.full(L3, 10), (rng.pareto(1.0, L1) * 4).astype(np.int64).clip(0, 120)])
    rows = np.concatenate([np.sort(rng.choice(m, c, replace=False)) for c in cnt]) + 1
    spl = np.concatenate([[1], 1 + np.cumsum(w)])
    pos = np.concatenate([[1], 1 + np.cumsum(cnt)])
    ofs = np.concatenate([[1], 1 + np.cumsum(cnt * w)])
    val = np.random.default_rng(42).uniform(0.25, 1, int(ofs[-1]) - 1 + 64)
    return V.SparseMatrix1DVBC(8, m, int(spl[-1]) - 1, V.SplitPartition(spl), pos, rows.astype(np.int64), ofs, val)


# name: (matrix, knobs, what info() must show of the layout)
REFUSED = {
    "lanes": (mesh, {"VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_LANES": "1"},
              lambda i: i["planar_bins"] >= 1 and i["planar_mask"] & 4),
    "split": (lambda: plain_matrix(3, 3), dict(KNOBS, VBC_PLANAR_SPLIT="4"),
              lambda i: i["planar_bins"] >= 1 and i["bins_t"] == 0 and i["planar_split"] == 4),
    "fused-split": (lambda: mesh(3, 9), {"VBC_SMALL_FUSE": "2"}, lambda i: i["planar_bins"] >= 1 and i["planar_mask"] & 32),
    "merge": (planar_and_merge, {"VBC_SLOT_PLANAR": "1", "VBC_SLOTS_SORT": "0", "VBC_SMALL_FUSE": "0",
                                 "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_PAIR": "0", "VBC_PLANAR_LANES": "0"},
              lambda i: i["planar_bins"] >= 1 and i["bins_t"] >= 1 and i["planar_split"] == 1 and not i["planar_mask"] & 4),
}


def refused(knobs, name):
    matrix, env, layout = REFUSED[name]
    knobs(env)
    M = make(matrix(), "f64")
    inf = info(M, "f64")
    print(sorted(inf.items()))
    assert layout(inf)
    assert not inf["planar_mask"] & (BIT | BIT22 | BIT23), inf
    return M


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_bit24_clear_on_refused_layouts(knobs, name):
    refused(knobs, name)


def test_bit24_clear_on_int64(knobs):
    knobs(plain_env())
    B = plain_matrix(5, 3)
    M = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, np.rint(B.val * 8).astype(np.int64))
    _LIVE.append(M)
    inf = M.info(trans=True, compute=L.VBC_I64)
    assert inf["dtype"] == L.VBC_I64, inf
    assert not inf["planar_mask"] & (BIT | BIT22 | BIT23), inf


# ---------------------------------------------------------------------------------------------------------------
# 2. bitwise against column by column
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("run", [1, 2, 3])
def test_plain_widths_runs(knobs, w, run):
    """Every width and row run (run 1: the run-3 matrix under VBC_SLOT_RUNS=0) in the three value kinds; k = 2 is one
    NR = 2 launch, k = 5 an NR = 4 launch and an NR = 2 launch of one live column."""
    knobs(plain_env(run=run))
    B = plain_matrix(w, 2 if run == 2 else 3)
    for kind in sorted(KINDS):
        M = make(B, kind)
        assert_fuses_w(info(M, kind), kind, w, run)
        check(M, KINDS[kind][1], seed=10 * w + run)
        M.release()


@pytest.mark.parametrize("w", [3, 5, 8])
@pytest.mark.parametrize("form", range(len(BX_FORMS)))
def test_plain_orders_keys_stage(knobs, w, form):
    """Natural, masked and sorted order; 32-bit and int16 keys; staged and direct single-vector writes."""
    order, keys, stage = BX_FORMS[form]
    knobs(plain_env(order, keys, stage))
    B = plain_matrix(w, 3)
    for kind in sorted(KINDS):
        M = make(B, kind)
        assert_fuses(info(M, kind), kind=kind, run=3, mask=order == "masked")
        check(M, KINDS[kind][1], seed=w + form)
        M.release()


VIEWS = tuple((ld, xo, yo) for ld in (0, 1, 5) for xo, yo in ((0, 0), (1, 0), (0, 1), (1, 1)))


@pytest.mark.parametrize("kind,w,run", [("f32", 7, 2), ("f64", 3, 3), ("narrow", 6, 3)])
def test_plain_nrhs_ld_offsets(knobs, kind, w, run):
    knobs(plain_env(run=run))
    M = make(plain_matrix(w, run), kind)
    assert_fuses(info(M, kind), kind=kind, run=run)
    check(M, KINDS[kind][1], ks=NRHS, views=VIEWS)


@pytest.mark.parametrize("w,run", [(3, 3), (5, 2), (8, 1)])
@pytest.mark.parametrize("order", ["natural", "masked"])
def test_plain_empty_stripes(knobs, w, run, order):
    """Empty stripes inside chunks of run-structured stripes (a lane that folds nothing and writes beta * y, or 0,
    in every column), one of them in the partial last chunk."""
    knobs(plain_env(order, run=run))
    B = plain_matrix(w, 2 if run == 2 else 3, empty=(5, 70, 150))
    for kind in sorted(KINDS):
        M = make(B, kind)
        assert_fuses_w(info(M, kind), kind, w, run, mask=order == "masked")
        check(M, KINDS[kind][1], ks=(3, 8), seed=w)
        M.release()


@pytest.mark.parametrize("form", range(len(PAIR_FORMS)))
@pytest.mark.parametrize("empty", [(), (5, 40, 80)])
def test_pair_orders_keys_stage(knobs, form, empty):
    """The lane-pair kernel over its eight forms (natural order staged and direct, masked, sorted; both key forms),
    with and without empty stripes, in fp64 and on Float32 stored values."""
    order, masked, keys, stage = PAIR_FORMS[form]
    knobs(pair_env(order, keys, stage))
    B = pair_matrix(empty)
    for kind in PAIR_KINDS:
        M = make(B, kind, pair=True)
        assert_fuses(info(M, kind), pair=True, kind=kind, run=3, mask=masked)
        check(M, np.float64, ks=(2, 3, 5), seed=form)
        M.release()


@pytest.mark.parametrize("kind", PAIR_KINDS)
def test_pair_nrhs_ld_offsets(knobs, kind):
    knobs(pair_env())
    M = make(pair_matrix(), kind, pair=True)
    assert_fuses(info(M, kind), pair=True, kind=kind, run=3)
    check(M, np.float64, ks=NRHS, views=VIEWS)


# ---------------------------------------------------------------------------------------------------------------
# 3. slotted and planar buckets in one handle
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_mixed_slotted_and_planar_buckets(knobs, kind):
    """Widths 1..8 under the planar knobs: slotted buckets for widths 1 and 2, planar ones for 3..8, 3 empty stripes:
    one product runs spmm_slots_col, spmm_planar_col per planar bucket and the fill list."""
    knobs(plain_env(run=1))
    B = V.synthetic.vbr_1dvbc(400, 300, 1400, np.arange(300) % 8 + 1, W=8, seed=7)
    assert int((np.diff(B.pos) == 0).sum()) == 3
    M = make(B, kind)
    inf = info(M, kind)
    assert_fuses(inf, slotted=True)
    # widths 3..8 planar and 1, 2 slotted; fp32 keeps w = 4 (one 16-B lane vector per row) slotted too
    assert inf["slot_bins"] == 8 and inf["planar_bins"] == (5 if kind == "f32" else 6), inf
    check(M, KINDS[kind][1], ks=(2, 3, 9), views=((0, 0, 0), (5, 1, 1)))
    X, Y0 = operands(M, KINDS[kind][1], 5)
    got = fused(M, X, torch.full_like(Y0, float("nan")), 1.0, 0.0, 3, 1, 1, cols=8)
    assert torch.isfinite(got).all()  # beta = 0 overwrites NaN everywhere, the empty stripes included


# ---------------------------------------------------------------------------------------------------------------
# 4. against the oracle (integer inputs: exact)
# ---------------------------------------------------------------------------------------------------------------

def check_oracle(M, B, val, xdt, k=7):
    R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, np.asarray(val, np.float64))
    rng = np.random.default_rng(23)
    X = rng.integers(-8, 9, (B.m, k)).astype(xdt)
    Y0 = rng.integers(-8, 9, (B.n, k)).astype(xdt)
    for alpha, beta in ((1.0, 0.0), (-1.0, 2.0)):
        got = fused(M, dev(X), dev(Y0), alpha, beta, 3, 1, 1).cpu().numpy().astype(np.float64)
        want = O.mulmat_t(R, X.astype(np.float64), np.asfortranarray(Y0.astype(np.float64)), alpha, beta)
        assert np.array_equal(got, want), (alpha, beta)


def integer_values(B, seed=1):
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 9, len(B.val)) * rng.choice([-1, 1], len(B.val))
    v[rng.permutation(len(v))[: len(v) // 10]] = 0
    return v.astype(np.float32)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_oracle_exact_plain(knobs, kind):
    knobs(plain_env("masked", run=2))
    B = plain_matrix(5, 2, empty=(5, 70, 150))
    val = integer_values(B)
    M = make(B, kind, val=val)
    assert_fuses(info(M, kind), kind=kind, run=2, mask=True)
    check_oracle(M, B, val, KINDS[kind][1])


@pytest.mark.parametrize("kind", PAIR_KINDS)
def test_oracle_exact_pair(knobs, kind):
    knobs(pair_env())
    B = pair_matrix((5, 40, 80))
    val = integer_values(B)
    M = make(B, kind, pair=True, val=val)
    assert_fuses(info(M, kind), pair=True, kind=kind)
    check_oracle(M, B, val, np.float64)


# ---------------------------------------------------------------------------------------------------------------
# 5. special values
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_nonfinite_rows_of_x(knobs, pair, masked):
    """Inf / NaN in single rows of X: bitwise the per-column result (padding rows take x as 0 by a select in both)."""
    if pair:
        knobs(pair_env({"VBC_SLOTS_SORT": "2"} if masked else None))
    else:
        knobs(plain_env("masked" if masked else "natural"))
    B = pair_matrix() if pair else plain_matrix(4, 3)
    M = make(B, "f64", pair=pair)
    assert_fuses(info(M, "f64"), pair=pair, mask=masked)
    X, Y0 = operands(M, np.float64, 5)
    X[0, :] = float("inf")
    X[B.m // 3, 1] = float("nan")
    X[B.m - 1, 3] = -float("inf")
    for alpha, beta in AB:
        got = fused(M, X, Y0, alpha, beta, 2, 1, 0)
        assert same(got, per_column(M, X, Y0, alpha, beta))
        assert not torch.isfinite(got).all() and torch.isfinite(got).any()


@pytest.mark.parametrize("pair", [False, True])
def test_special_stored_values_narrow_against_wide(knobs, pair):
    """Float32 NaN, +-0.0, +-Inf, a subnormal and FLT_MAX among the stored values: the fused product on the narrow
    handle has the bits of the fused and of the per-column product on the wide handle."""
    knobs(pair_env() if pair else plain_env(run=2))
    B = pair_matrix(seed=3) if pair else plain_matrix(5, 2)
    nval = int(B.ofs[-1]) - 1
    v = B.val.copy()
    fi = np.finfo(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max,
                        -fi.max, fi.tiny], np.float32)
    v[np.random.default_rng(8).choice(nval, 4 * len(special), replace=False)] = np.tile(special, 4)
    N, W = make(B, "narrow", pair=pair, val=v), make(B, "f64", pair=pair, val=v)
    assert_fuses(info(N, "narrow"), pair=pair, kind="narrow")
    assert_fuses(info(W, "f64"), pair=pair, kind="f64")
    rng = np.random.default_rng(9)
    X, Y0 = dev(rng.uniform(0.5, 1.0, (B.m, 5))), dev(rng.uniform(-1, 1, (B.n, 5)))
    for alpha, beta in AB:
        got, wide = fused(N, X, Y0, alpha, beta, 1, 1, 1), per_column(W, X, Y0, alpha, beta)
        assert torch.isnan(wide).any() and torch.isinf(wide).any()
        assert same(got, wide) and same(fused(W, X, Y0, alpha, beta, 1, 1, 1), wide), (alpha, beta)


# ---------------------------------------------------------------------------------------------------------------
# 6. graph capture, 7. value updates, 8. host operands, 9. refused forms
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,pair", [("f32", False), ("f64", False), ("narrow", False), ("f64", True), ("narrow", True)])
def test_graph_captured_on_first_use(knobs, capture_stream, kind, pair):
    """The fused product allocates nothing and uses no side stream, so its first call on a fresh handle may be a
    captured one: no eager product of any kind precedes the capture."""
    knobs(pair_env() if pair else plain_env())
    xdt = KINDS[kind][1]
    M = make(pair_matrix((5,)) if pair else plain_matrix(3, 3, empty=(5, 70, 150)), kind, pair=pair)
    assert_fuses(info(M, kind), pair=pair, kind=kind)  # (the handle is created here: a create allocates)
    X, Y0 = operands(M, xdt, 5)
    _, Xv = view2d(M.m, 5, M.m + 1, 1, X.dtype, float("nan"))
    _, Yv = view2d(M.n, 5, M.n + 3, 0, X.dtype, float("nan"))
    Xv.copy_(X)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=capture_stream):
        V.mulmat_(Yv, V.adjoint(M), Xv, 1.0, 0.0, engine="vector")
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
    knobs(pair_env() if pair else plain_env("masked"))
    B = pair_matrix() if pair else plain_matrix(6, 3)
    v2 = np.random.default_rng(6).uniform(-1, 1, len(B.val)).astype(np.float32)
    M = make(B, kind, pair=pair, updatable=True)
    assert_fuses(info(M, kind), pair=pair, kind=kind)
    X, Y0 = operands(M, KINDS[kind][1], 5)
    first = fused(M, X, Y0, -0.5, 2.0)
    M.update_values(v2.astype(KINDS[kind][0]))
    N = make(B, kind, pair=pair, val=v2)
    assert_fuses(info(N, kind), pair=pair, kind=kind)
    got, want = fused(M, X, Y0, -0.5, 2.0), fused(N, X, Y0, -0.5, 2.0)
    assert same(got, want) and not same(got, first)
    assert same(got, per_column(N, X, Y0, -0.5, 2.0))


@pytest.mark.parametrize("kind,pair", [("f32", False), ("f64", False), ("narrow", False), ("f64", True)])
def test_host_operands(knobs, kind, pair):
    """numpy order="F" operands: staged into packed device buffers, the fused product there, copied back."""
    knobs(pair_env() if pair else plain_env(run=2))
    xdt = KINDS[kind][1]
    M = make(pair_matrix((5, 40, 80)) if pair else plain_matrix(7, 2, empty=(5, 70, 150)), kind, pair=pair)
    assert_fuses(info(M, kind), pair=pair, kind=kind)
    rng = np.random.default_rng(31)
    for k in (3, 6):
        X = np.asfortranarray(rng.uniform(-1, 1, (M.m, k)).astype(xdt))
        Y0 = np.asfortranarray(rng.uniform(-1, 1, (M.n, k)).astype(xdt))
        for alpha, beta in AB:
            Y = Y0.copy(order="F")
            V.mulmat_(Y, V.adjoint(M), X, alpha, beta, engine="vector")
            ref = per_column(M, dev(X), dev(Y0), alpha, beta)
            assert same(torch.from_numpy(np.ascontiguousarray(Y)), ref), (k, alpha, beta)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_layouts_run_per_column(knobs, name):
    M = refused(knobs, name)
    check(M, np.float64, ks=(3, 5))


@pytest.mark.parametrize("pair", [False, True])
def test_knob_off_same_result(knobs, pair):
    """A handle created under VBC_MM_PLANAR_COL=0 runs one SpMV per column and gives the fused handle's bits."""
    B = pair_matrix() if pair else plain_matrix(5, 3)
    knobs(pair_env() if pair else plain_env(), {"VBC_MM_PLANAR_COL": "0"})
    M = make(B, "f64", pair=pair)
    inf = info(M, "f64")
    assert_planar(inf, pair=pair)
    assert not inf["planar_mask"] & BIT
    check(M, np.float64, ks=(5,))
    X, Y0 = operands(M, np.float64)
    off = fused(M, X, Y0, *AB[-1], 1, 1, 1)
    knobs(pair_env() if pair else plain_env())
    N = make(B, "f64", pair=pair)
    assert_fuses(info(N, "f64"), pair=pair)
    assert same(fused(N, X, Y0, *AB[-1], 1, 1, 1), off)


def test_rowmajor_and_forward_keep_their_paths(knobs):
    """Row-major operands on a planar layout and the forward product are out of scope: the engine="vector" product
    still equals the per-column one."""
    knobs(plain_env())
    M = make(plain_matrix(4, 3), "f64")
    assert_fuses(info(M, "f64"))
    X, Y0 = operands(M, np.float64, 5)
    for alpha, beta in AB:
        Y = Y0.clone()  # C-contiguous (n, k): row-major operands
        V.mulmat_(Y, V.adjoint(M), X.contiguous(), alpha, beta, engine="vector")
        assert same(Y, per_column(M, X, Y0, alpha, beta))
    Xf, Yf0 = Y0, X
    _, Yv = view2d(M.m, 5, M.m + 1, 0, Yf0.dtype, float("nan"))
    _, Xv = view2d(M.n, 5, M.n + 1, 0, Xf.dtype, float("nan"))
    Xv.copy_(Xf)
    V.mulmat_(Yv, M, Xv, 1.0, 0.0, engine="vector")
    for j in range(5):
        y = torch.empty(M.m, dtype=torch.float64, device=DEV)
        V.mul_(y, M, Xf[:, j].contiguous())
        assert same(Yv[:, j], y), j
