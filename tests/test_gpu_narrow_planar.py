"""Narrow value storage of the planar layout (vbc.h VBC_CREATE_NARROW_PLANAR, `B.narrow = "planar"`): on a Float64
handle of a float32 matrix the chunk-planar B'x buckets (spmv_planar) and the forward run buckets (spmv_planar_fwd)
keep Float32 values, stored in the Float32 column-group arrangement and widened in registers.  No layout decision
changes, so every vbc_info field but the byte counts and planar_mask bits 14 / 15 is that of the handle created with
VBC_CREATE_NARROW_VALUES alone (`B.narrow = True`), and every product is bit-identical to that handle's and to the
wide handle's (no flag); the oracle gets val.astype(float64).  Tolerances as in test_gpu_parity.py.

The kernel families are forced at small size with the layout knobs of INTEGRATION.md, and every case first checks
through vbc_info that it got the layout it means to test.  Shapes: about 170 stripes (three chunks of 64, the last
one partial), ragged stripe lengths of up to about 40 rows, m = 300."""
import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_parity import TOL64, dev, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"

# The plain chunk-planar kernels at any size: planar rows from width 3, no fused small-matrix launch, no split
# product, no lane pairs, no lane streams; VBC_SLOTS=1 keeps a small ragged bucket out of the merge layout.
KNOBS = {"VBC_SLOT_PLANAR": "1", "VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_PAIR": "0",
         "VBC_PLANAR_LANES": "0", "VBC_SLOTS": "1"}
# segment orders of a B'x bucket (VBC_SLOTS=1: the natural order whenever it is allowed)
ORDERS = {"natural": {}, "masked": {"VBC_SLOTS_SORT": "2", "VBC_PLANAR_MASK": "1"},
          "sorted": {"VBC_SLOTS_SORT": "2", "VBC_PLANAR_MASK": "0"}}
BYTE_FIELDS = ("device_bytes", "bytes_t", "bytes_f", "planar_mask", "narrow_planar_t", "narrow_planar_f")
PLANAR_BITS = (1 << 14) | (1 << 15)
AB = ((1.0, 0.0), (-0.5, 2.0))  # FASTE / staged writes, and the path that reads y


@pytest.fixture
def forced(monkeypatch):
    for k, v in KNOBS.items():
        monkeypatch.setenv(k, v)
    yield monkeypatch
    for k in list(KNOBS) + ["VBC_SLOTS_SORT", "VBC_PLANAR_MASK", "VBC_SLOT_KEYS16", "VBC_SLOT_STAGE", "VBC_SLOT_RUNS",
                            "VBC_SLOTS_PAD", "VBC_FWD_MIN_ROWS"]:
        monkeypatch.delenv(k, raising=False)


def ragged(w, R, stripes=170, nodes_max=None, seed=1, empty=()):
    """`stripes` w-wide stripes over m = 300 rows whose rows come in aligned runs of R (a node's dof rows): the first
    128 stripes hold 1 .. 40 / R nodes each, the rest (the partial last chunk of the natural order) 1 or 2, so some
    ranges are shorter than one pipeline step; the stripes listed in `empty` hold nothing.  float32 values."""
    rng = np.random.default_rng(seed + 10 * w + R)
    m = 300
    nodes = m // R
    nmax = nodes_max or max(1, 40 // R)
    cnt = np.where(np.arange(stripes) < 128, rng.integers(1, nmax + 1, stripes), rng.integers(1, 3, stripes))
    cnt[list(empty)] = 0
    idx = np.concatenate([np.sort(rng.choice(nodes, c, replace=False)) for c in cnt] + [np.zeros(0, np.int64)])
    idx = (idx[:, None] * R + np.arange(R)[None, :]).reshape(-1)
    rows = cnt.astype(np.int64) * R
    spl = 1 + np.arange(stripes + 1, dtype=np.int64) * w
    pos = np.concatenate([[1], 1 + np.cumsum(rows)]).astype(np.int64)
    ofs = np.concatenate([[1], 1 + np.cumsum(rows * w)]).astype(np.int64)
    val = rng.uniform(-1, 1, int(ofs[-1]) - 1).astype(np.float32)
    return V.SparseMatrix1DVBC(8, m, stripes * w, V.SplitPartition(spl), pos, idx.astype(np.int64) + 1, ofs, val)


def clone(B, narrow, val=None):
    """A fresh matrix object (its own handle cache: the knobs are read when a handle is created)."""
    C_ = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, B.val if val is None else val)
    if narrow:
        C_.narrow = narrow
    return C_


def trio(B, val=None):
    """(0x180, 0x80, wide) handles' matrices of one float32 matrix."""
    assert B.val.dtype == np.float32
    return clone(B, "planar", val), clone(B, True, val), clone(B, False, val)


def ref1d(B):
    return O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, B.val.astype(np.float64))


def info64(B, trans):
    return B.info(trans=trans, compute=L.VBC_F64)


def bitwise(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def product(B, trans, x, y0, alpha, beta):
    y = dev(y0.copy())
    V.mul_(y, V.adjoint(B) if trans else B, dev(x), alpha, beta)
    return y.cpu().numpy()


def check_layout(Bp, Bn, Bw, trans, nval_planar, run=None, mask=None):
    """The handle is the one the case means to test, and differs from the 0x80 handle in bytes and bits 14 / 15 only."""
    a, b, c = info64(Bp, trans), info64(Bn, trans), info64(Bw, trans)
    assert a["planar_split"] == 1 and a["planar_pair"] == 0, a
    assert a["planar_mask"] & ((1 << 2) | (1 << 5) | (1 << 6)) == 0, a["planar_mask"]  # lanes, fused split, cut stripes
    assert not a["planar_mask"] & 8 and not a["planar_mask"] & 16 and not a["planar_mask"] & 2048  # forward split / lanes / pairs
    if trans:
        assert a["planar_bins"] >= 1
        assert a["planar_mask"] & (1 << 14), a["planar_mask"]
        assert a["narrow_planar_t"]
        if run is not None:
            assert a["planar_run"] == run, a["planar_run"]
        if mask is not None:
            assert (a["planar_mask"] & 1) == int(mask)
    else:
        assert a["slot_bins"] >= 1  # (planar_bins counts the B'x bins; the forward planar bin shows in fwd_run)
        assert a["planar_mask"] & (1 << 15), a["planar_mask"]
        assert a["narrow_planar_f"]
        if run is not None:
            assert a["fwd_run"] == run, a["fwd_run"]
        if mask is not None:
            assert ((a["planar_mask"] >> 1) & 1) == int(mask)
    for k in a:
        if k not in BYTE_FIELDS:
            assert a[k] == b[k], (k, a[k], b[k])
    assert (a["planar_mask"] & ~PLANAR_BITS) == b["planar_mask"]
    assert not b["planar_mask"] & PLANAR_BITS and not c["planar_mask"] & PLANAR_BITS  # 0x80 alone: planar buckets stay wide
    bk = "bytes_t" if trans else "bytes_f"
    print("trans", trans, bk, a[bk], b[bk], "device_bytes", a["device_bytes"], b["device_bytes"], "4 * values", 4 * nval_planar)
    assert b[bk] - a[bk] >= 4 * nval_planar
    assert b["device_bytes"] - a["device_bytes"] >= 4 * nval_planar
    return a


def check_products(Bp, Bn, Bw, trans, R, seed):
    rng = np.random.default_rng(seed)
    nx, ny = (Bw.m, Bw.n) if trans else (Bw.n, Bw.m)
    x, y0 = rng.uniform(-1, 1, nx), rng.uniform(-1, 1, ny)
    for alpha, beta in AB:
        got = product(Bp, trans, x, y0, alpha, beta)
        assert bitwise(got, product(Bn, trans, x, y0, alpha, beta)), (trans, alpha, beta)
        assert bitwise(got, product(Bw, trans, x, y0, alpha, beta)), (trans, alpha, beta)
        err = rel(got, O.mul(R, x, y0.copy(), alpha, beta, trans=trans, ref_semantics=False))
        print("trans", trans, "alpha", alpha, "beta", beta, "rel err", err)
        assert err <= TOL64, (trans, alpha, beta)


# (order, VBC_SLOT_KEYS16, VBC_SLOT_STAGE): 32-bit and int16 keys in every order; direct y writes in the natural one
BX_FORMS = [("natural", "0", None), ("natural", "2", None), ("natural", "2", "0"), ("masked", "0", None),
            ("masked", "2", None), ("sorted", "0", None), ("sorted", "2", None)]


def run_bx(forced, B, run, seed):
    nval = int(B.ofs[-1]) - 1
    R = ref1d(B)
    forced.setenv("VBC_SLOT_RUNS", "1" if run > 1 else "0")
    for order, keys, stage in BX_FORMS:
        for k in ("VBC_SLOTS_SORT", "VBC_PLANAR_MASK", "VBC_SLOT_STAGE"):
            forced.delenv(k, raising=False)
        for k, v in ORDERS[order].items():
            forced.setenv(k, v)
        forced.setenv("VBC_SLOT_KEYS16", keys)
        if stage is not None:
            forced.setenv("VBC_SLOT_STAGE", stage)
        Bp, Bn, Bw = trio(B)
        check_layout(Bp, Bn, Bw, True, nval, run=run, mask=order == "masked")
        check_products(Bp, Bn, Bw, True, R, seed)
        for M in (Bp, Bn, Bw):
            M.release()


@pytest.mark.parametrize("w", [3, 4, 5, 6, 7, 8])  # Float32 tail groups of 12, 16, 16 + 4, 16 + 8, 16 + 12, 16 + 16 B
@pytest.mark.parametrize("run", [1, 2, 3])
def test_bx_widths_runs_orders_keys(forced, w, run):
    """spmv_planar<double, ..., float>: every width, row run, segment order and key form, both (alpha, beta).  Run 1
    is the run-3 matrix under VBC_SLOT_RUNS=0."""
    run_bx(forced, ragged(w, 2 if run == 2 else 3), run, seed=100 * w + run)


@pytest.mark.parametrize("w,run", [(3, 3), (5, 2), (8, 1)])
def test_bx_empty_stripes(forced, w, run):
    """Empty stripes inside a chunk of run-structured stripes (a lane that folds nothing and writes beta * y), one of
    them in the partial last chunk."""
    run_bx(forced, ragged(w, 2 if run == 2 else 3, empty=(5, 70, 150)), run, seed=7 * w + run)


def test_bx_special_values(forced):
    """Float32 NaN, +-0.0, +-Inf, a subnormal and FLT_MAX among the stored values: narrowing on the host and widening
    in the kernel give the wide handle's bits (compared with the wide handle only: the oracle's NaN bits are the
    CPU's)."""
    B = ragged(5, 2, seed=3)
    nval = int(B.ofs[-1]) - 1
    v = B.val.copy()
    fi = np.finfo(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max,
                        -fi.max, fi.tiny], np.float32)
    at = np.random.default_rng(8).choice(nval, 4 * len(special), replace=False)
    v[at] = np.tile(special, 4)
    rng = np.random.default_rng(9)
    x, y0 = rng.uniform(0.5, 1.0, B.m), rng.uniform(-1, 1, B.n)
    for order in ("natural", "masked"):
        for k, val_ in ORDERS[order].items():
            forced.setenv(k, val_)
        Bp, Bn, Bw = trio(B, v)
        check_layout(Bp, Bn, Bw, True, nval, run=2, mask=order == "masked")
        for alpha, beta in AB:
            got, wide = product(Bp, True, x, y0, alpha, beta), product(Bw, True, x, y0, alpha, beta)
            assert np.isnan(wide).any() and np.isinf(wide).any()
            assert bitwise(got, wide), (order, alpha, beta)


def mesh(dof):
    """The 5-point mesh operator with dof unknowns per node on 13 x 13 nodes (169 node segments: three chunks)."""
    return V.synthetic.fe_grid_2d(13, dof=dof, dtype=np.float32, seed=11 + dof)


# (knobs, masked): the natural order (staged and direct writes, both key forms), the masked chunk-local order the
# mesh takes by itself (a partial last chunk pads beyond VBC_SLOTS_PAD), and the length-sorted order
FWD_FORMS = [({"VBC_SLOTS_PAD": "100"}, False), ({"VBC_SLOTS_PAD": "100", "VBC_SLOT_KEYS16": "0"}, False),
             ({"VBC_SLOTS_PAD": "100", "VBC_SLOT_STAGE": "0"}, False),
             ({"VBC_SLOTS_PAD": "100", "VBC_FWD_MIN_ROWS": "4"}, False),  # one range per chunk instead of one for all
             ({}, True), ({"VBC_SLOT_KEYS16": "0"}, True),
             ({"VBC_PLANAR_MASK": "0", "VBC_SLOTS_PAD": "1.2"}, False)]


@pytest.mark.parametrize("dof", [2, 3])
def test_forward_mesh(forced, dof):
    """spmv_planar_fwd<double, ..., float> on the dof-2 and dof-3 mesh operators (dof x dof blocks, output rows in
    runs of dof), not split."""
    forced.delenv("VBC_SLOTS")  # (the forward run layout has its own padding rule)
    B = mesh(dof)
    nval = int(B.ofs[-1]) - 1
    R = ref1d(B)
    for knobs, masked in FWD_FORMS:
        for k in ("VBC_SLOTS_PAD", "VBC_SLOT_KEYS16", "VBC_SLOT_STAGE", "VBC_PLANAR_MASK", "VBC_FWD_MIN_ROWS"):
            forced.delenv(k, raising=False)
        for k, v in knobs.items():
            forced.setenv(k, v)
        Bp, Bn, Bw = trio(B)
        check_layout(Bp, Bn, Bw, False, nval, run=dof, mask=masked)
        check_products(Bp, Bn, Bw, False, R, seed=40 + dof)
        for M in (Bp, Bn, Bw):
            M.release()


def test_mixed_slotted_and_planar_buckets_both_narrow():
    """tests/test_gpu_narrow.py's mixed matrix (widths 2 and 3 alternating, default knobs): under 0x80 | 0x100 the
    slotted 2-wide bucket and the planar 3-wide bucket both store Float32."""
    from tests.test_gpu_narrow import mixed_matrix
    B = mixed_matrix()
    Bp, Bw = clone(B, "planar"), clone(B, False)
    nval = int(B.ofs[-1]) - 1
    a, c = info64(Bp, True), info64(Bw, True)
    assert a["planar_mask"] & (1 << 12) and a["planar_mask"] & (1 << 14), a["planar_mask"]
    assert a["narrow_t"] and a["narrow_planar_t"]
    for k in a:
        if k not in BYTE_FIELDS + ("narrow_t", "narrow_f"):
            assert a[k] == c[k], (k, a[k], c[k])
    print("bytes_t", a["bytes_t"], c["bytes_t"], "device_bytes", a["device_bytes"], c["device_bytes"], "4 * nval", 4 * nval)
    assert c["bytes_t"] - a["bytes_t"] >= 4 * nval
    assert c["device_bytes"] - a["device_bytes"] >= 4 * nval
    rng = np.random.default_rng(9)
    x, y0 = rng.uniform(-1, 1, B.m), rng.uniform(-1, 1, B.n)
    for alpha, beta in AB:
        assert bitwise(product(Bp, True, x, y0, alpha, beta), product(Bw, True, x, y0, alpha, beta)), (alpha, beta)


def test_csc_node_blocked_operand(forced):
    """vbc_csc_create_ex groups a node's dof columns into one stripe: a 3-dof stiffness operand gives a 3-wide planar
    bucket with row runs of 3, and TrSpMV! on the narrow-planar handle equals the wide handle's bit for bit."""
    A = V.synthetic.fe_stiffness_3d(900, 20000, 3, np.float32).tocsc()
    A.sort_indices()
    m, n = A.shape
    outs = {}
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, m)
    for narrow in ("planar", False):
        Cm = V.SparseMatrixCSC(A)
        if narrow:
            Cm.narrow = narrow
        inf = Cm.info(trans=True, compute=L.VBC_F64)
        assert inf["L"] == n // 3 and inf["planar_bins"] == 1 and inf["planar_split"] == 1 and inf["planar_pair"] == 0
        assert inf["planar_run"] == 3 and inf["slot_bins"] == 1  # every column in a 3-wide stripe of the one planar bucket
        assert inf["planar_mask"] & ((1 << 2) | (1 << 5) | (1 << 6)) == 0
        assert bool(inf["planar_mask"] & (1 << 14)) == bool(narrow)
        y = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
        V.TrSpMV_(y, Cm, dev(x))
        outs[narrow] = (y.cpu().numpy(), inf)
        Cm.release()
    assert bitwise(outs["planar"][0], outs[False][0])
    assert outs[False][1]["device_bytes"] - outs["planar"][1]["device_bytes"] >= 4 * A.nnz
    exact = O.trspmv(A.astype(np.float64), x, np.zeros(n))
    assert rel(outs["planar"][0], exact) <= TOL64


def test_graph_replay(forced):
    """A narrow-planar B'x product and a forward one captured into a HIP graph replay to the eager bits."""
    Bt = clone(ragged(6, 3), "planar")
    Bf = clone(mesh(2), "planar")
    assert info64(Bt, True)["narrow_planar_t"] and info64(Bf, False)["narrow_planar_f"]
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand(Bt.m, dtype=torch.float64, device=DEV, generator=gen)
    xf = torch.rand(Bf.n, dtype=torch.float64, device=DEV, generator=gen)

    def outputs():
        return [torch.full((Bt.n,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2)] + \
               [torch.full((Bf.m,), float("nan"), dtype=torch.float64, device=DEV)]

    def products(ys):
        V.mul_(ys[0], Bt.T, x)
        V.mul_(ys[1], Bt.T, x, 0.5, 0.0)
        V.mul_(ys[2], Bf, xf)

    s = torch.cuda.Stream()
    y_e, y_g = outputs(), outputs()
    torch.cuda.synchronize()  # the NaN fills ran on the default stream, which `s` does not wait for
    with torch.cuda.stream(s):
        products(y_e)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        products(y_g)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(y_g, y_e):
        assert torch.equal(a, b) and not torch.isnan(a).any()
