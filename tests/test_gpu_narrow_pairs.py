"""Narrow value storage of the lane-pair kernels (vbc.h VBC_CREATE_NARROW_PAIRS, `B.narrow = "pairs"`): on a Float64
handle of a float32 matrix the buckets of spmv_planar_pair (B'x and the forward DOT form) and of spmv_pair_lanes keep
Float32 values -- the wide run-row's 288 values as 288 floats -- widened in registers.  No layout
decision changes, so every vbc_info field but the byte counts and planar_mask bits 16 / 17 is that of the handle
created with 0x180 (`B.narrow = "planar"`), and every product is bit-identical to that handle's and to the wide
handle's; the oracle gets val.astype(float64).  Tolerances as in test_gpu_parity.py.

The kernel families are forced at small size with the layout knobs of INTEGRATION.md, and every case first checks
through vbc_info that it got the layout it means to test."""
import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_narrow_planar import AB, bitwise, check_products, clone, info64, product, ragged, ref1d
from tests.test_gpu_parity import TOL64, dev, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"

PAIR = {"VBC_PLANAR_PAIR": "2", "VBC_SLOTS": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0", "VBC_PLANAR_LANES": "0"}
PAIR_LANES = {"VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0"}
FWD_PAIR = {"VBC_PLANAR_PAIR": "2", "VBC_PLANAR_SPLIT": "0"}
ALL_KNOBS = sorted(set(PAIR) | set(PAIR_LANES) | {"VBC_SLOTS_SORT", "VBC_PLANAR_MASK", "VBC_PLANAR_MASK_PAIR", "VBC_SLOT_KEYS16",
                                                  "VBC_SLOT_STAGE", "VBC_SLOTS_PAD", "VBC_TARGET_RANGES_L"})
BYTE_FIELDS = ("device_bytes", "bytes_t", "bytes_f", "planar_mask", "narrow_pair_t", "narrow_pair_f")
PAIR_BITS = (1 << 16) | (1 << 17)


@pytest.fixture
def knobs(monkeypatch):
    def set_(*envs):
        for k in ALL_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for env in envs:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
    yield set_
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)


def trio(B, val=None):
    """(0x580, 0x180, wide) handles' matrices of one float32 matrix."""
    assert B.val.dtype == np.float32
    return clone(B, "pairs", val), clone(B, "planar", val), clone(B, False, val)


def check_layout(Bq, Bp, Bw, trans, nval, lanes=False, mask=None, dot=False):
    """The handle is the one the case means to test, and differs from the 0x180 handle in bytes and bits 16 / 17
    only; the byte fields fall by at least 4 bytes per stored pair value (every value of these matrices)."""
    a, b, c = info64(Bq, trans), info64(Bp, trans), info64(Bw, trans)
    bit, key = (16, "narrow_pair_t") if trans else (17, "narrow_pair_f")
    assert a["planar_mask"] & (1 << bit) and a[key], a["planar_mask"]
    assert not a["planar_mask"] & (PAIR_BITS & ~(1 << bit))
    if trans:
        assert a["planar_pair"] == 1 and a["planar_bins"] == 1 and a["planar_split"] == 1 and a["planar_run"] == 3, a
        assert bool(a["planar_mask"] & 4) == lanes, a["planar_mask"]  # bit 2: lane streams
        if mask is not None:
            assert (a["planar_mask"] & 1) == int(mask), a["planar_mask"]
    else:
        assert dot and a["planar_mask"] & 2048 and a["fwd_run"] == 3, a  # bit 11: forward lane pairs
        assert not a["planar_mask"] & 8 and not a["planar_mask"] & 16  # not split, not lane streams
        if mask is not None:
            assert ((a["planar_mask"] >> 1) & 1) == int(mask), a["planar_mask"]
    for k in a:
        if k not in BYTE_FIELDS:
            assert a[k] == b[k] == c[k], (k, a[k], b[k], c[k])
    assert (a["planar_mask"] & ~PAIR_BITS) == b["planar_mask"] == c["planar_mask"]
    # 0x180 alone: the pair buckets stay wide, byte for byte the wide handle's counts
    assert not b["planar_mask"] & PAIR_BITS and not b["narrow_pair_t"] and not b["narrow_pair_f"]
    bk, other = ("bytes_t", "bytes_f") if trans else ("bytes_f", "bytes_t")
    assert b[bk] == c[bk] and b["device_bytes"] == c["device_bytes"]
    print("trans", trans, bk, a[bk], b[bk], "device_bytes", a["device_bytes"], b["device_bytes"], "4 * values", 4 * nval)
    assert b[bk] - a[bk] >= 4 * nval
    assert b["device_bytes"] - a["device_bytes"] >= 4 * nval
    assert a[other] == b[other]
    return a


# (order knobs, masked, VBC_SLOT_KEYS16, VBC_SLOT_STAGE): natural order staged and direct, both key forms; the masked
# chunk-local order; the length-sorted order a pair bucket takes when it may not be masked.  Only the natural order is
# crossed with VBC_SLOT_STAGE: the masked and sorted orders take the table-mapped (non-FASTE) kernels, where the knob
# has no effect.  vbc_info does not say which launch variant ran (FASTE staged or direct): those cases rest on the knob.
MASKED = {"VBC_SLOTS_SORT": "2"}
SORTED = {"VBC_SLOTS_SORT": "2", "VBC_PLANAR_MASK_PAIR": "0"}
BX_FORMS = [({}, False, "0", None), ({}, False, "2", None), ({}, False, "0", "0"), ({}, False, "2", "0"),
            (MASKED, True, "0", None), (MASKED, True, "2", None), (SORTED, False, "0", None), (SORTED, False, "2", None)]


def run_bx(knobs, B, seed):
    nval = int(B.ofs[-1]) - 1
    R = ref1d(B)
    for order, masked, keys, stage in BX_FORMS:
        knobs(PAIR, order, {"VBC_SLOT_KEYS16": keys}, {} if stage is None else {"VBC_SLOT_STAGE": stage})
        Bq, Bp, Bw = trio(B)
        check_layout(Bq, Bp, Bw, True, nval, mask=masked)
        check_products(Bq, Bp, Bw, True, R, seed)
        for M in (Bq, Bp, Bw):
            M.release()


def test_pair_bx_orders_keys_stage(knobs):
    """spmv_planar_pair<..., float>, B'x: 85 stripes (three chunks of 32, the last one partial) of 1 .. 13 node runs,
    so ranges are shorter than one 4-run-row pipeline stage and lengths are no multiples of 8; m = 300.  Natural,
    masked and length-sorted order, 32-bit and int16 keys, staged and direct y writes, both (alpha, beta)."""
    run_bx(knobs, ragged(3, 3, stripes=85), seed=31)


def test_pair_bx_empty_stripes(knobs):
    """The same with empty stripes inside full chunks and in the partial last one."""
    run_bx(knobs, ragged(3, 3, stripes=85, empty=(5, 40, 80)), seed=32)


def test_pair_bx_special_values(knobs):
    """Float32 NaN, +-0.0, +-Inf, a subnormal and FLT_MAX among the stored values: narrowing on the host and widening
    in the kernel give the wide handle's bits (compared with the wide handle only: the oracle's NaN bits are the
    CPU's)."""
    B = ragged(3, 3, stripes=85, seed=3)
    nval = int(B.ofs[-1]) - 1
    v = B.val.copy()
    fi = np.finfo(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max,
                        -fi.max, fi.tiny], np.float32)
    at = np.random.default_rng(8).choice(nval, 4 * len(special), replace=False)
    v[at] = np.tile(special, 4)
    rng = np.random.default_rng(9)
    x, y0 = rng.uniform(0.5, 1.0, B.m), rng.uniform(-1, 1, B.n)
    for order, masked in (({}, False), (MASKED, True)):
        knobs(PAIR, order)
        Bq, Bp, Bw = trio(B, v)
        check_layout(Bq, Bp, Bw, True, nval, mask=masked)
        for alpha, beta in AB:
            got, wide = product(Bq, True, x, y0, alpha, beta), product(Bw, True, x, y0, alpha, beta)
            assert np.isnan(wide).any() and np.isinf(wide).any()
            assert bitwise(got, wide), (masked, alpha, beta)
            assert bitwise(got, product(Bp, True, x, y0, alpha, beta)), (masked, alpha, beta)


@pytest.fixture(scope="module")
def fwd_matrix():
    """A 3-dof stiffness operand of 300 nodes (about 15 blocks per node), one node's rows and columns zeroed (a node
    that couples to nothing: an empty stripe and empty output rows of B), as SparseMatrix1DVBC{8}(permutedims(A),
    StrictChunker(8)); and its oracle."""
    A = V.synthetic.fe_stiffness_3d(900, 40000, 3, np.float32).tolil()
    A[30:33, :] = 0.0
    A[:, 30:33] = 0.0
    A = A.tocsc()
    A.eliminate_zeros()
    B = V.SparseMatrix1DVBC[8](A.T.tocsc(), V.StrictChunker(8))
    return B, ref1d(B)


# natural order (it pads; VBC_SLOTS_PAD lets it) and the masked chunk-local order the planner takes by itself
@pytest.mark.parametrize("mask", ["0", "1"])
@pytest.mark.parametrize("keys16", ["0", "2"])
def test_forward_dot_pairs(knobs, fwd_matrix, keys16, mask):
    """spmv_planar_pair<..., DOT, float>: the forward product of 3 x 3 node blocks, both key forms, natural
    (VBC_PLANAR_MASK=0; VBC_SLOTS_PAD=100 admits the natural order's padding at this size) and masked order:
    bits 11 and 17, bitwise equal to the wide handle's product, and equal to the oracle (the reference's forward
    association)."""
    B, R = fwd_matrix
    knobs(FWD_PAIR, {"VBC_SLOT_KEYS16": keys16, "VBC_PLANAR_MASK": mask}, {"VBC_SLOTS_PAD": "100"} if mask == "0" else {})
    nval = int(B.ofs[-1]) - 1
    Bq, Bp, Bw = trio(B)
    check_layout(Bq, Bp, Bw, False, nval, mask=mask == "1", dot=True)
    check_products(Bq, Bp, Bw, False, R, seed=41)
    x = np.random.default_rng(42).uniform(-1, 1, B.n)
    got = product(Bq, False, x, np.zeros(B.m), 1.0, 0.0)
    assert np.array_equal(got, O.mul(R, x, np.zeros(B.m)))
    assert not got[30:33].any()
    for M in (Bq, Bp, Bw):
        M.release()


@pytest.fixture(scope="module")
def lanes_matrix():
    B = V.synthetic.fe_stiffness_3d_1dvbc(3000, 30000, dtype=np.float32)
    return B, ref1d(B)


@pytest.mark.parametrize("target", ["8", "256"])  # tiles of many streams' worth of stripes, and of few
def test_pair_lanes(knobs, lanes_matrix, target):
    """spmv_pair_lanes<RD, float> (both RD: beta = 0 and beta != 0): FE-3D's 1000 node stripes as lane-pair streams,
    bits 2 and 16."""
    B, R = lanes_matrix
    knobs(PAIR_LANES, {"VBC_TARGET_RANGES_L": target})
    nval = int(B.ofs[-1]) - 1
    Bq, Bp, Bw = trio(B)
    check_layout(Bq, Bp, Bw, True, nval, lanes=True)
    check_products(Bq, Bp, Bw, True, R, seed=51)
    for M in (Bq, Bp, Bw):
        M.release()


def test_csc_operand(knobs):
    """TrSpMV! on a 3-dof stiffness operand (vbc_csc_create_ex groups a node's columns into a 3-wide stripe) under
    VBC_PLANAR_PAIR=2: bitwise the wide handle's result."""
    knobs(PAIR)
    A = V.synthetic.fe_stiffness_3d(900, 40000, 3, np.float32).tocsc()
    A.sort_indices()
    m, n = A.shape
    x = np.random.default_rng(12).uniform(-1, 1, m)
    outs = {}
    for narrow in ("pairs", "planar", False):
        Cm = V.SparseMatrixCSC(A)
        if narrow:
            Cm.narrow = narrow
        inf = Cm.info(trans=True, compute=L.VBC_F64)
        assert inf["planar_pair"] == 1 and inf["planar_bins"] == 1 and inf["planar_split"] == 1 and inf["planar_run"] == 3, inf
        assert bool(inf["planar_mask"] & (1 << 16)) == (narrow == "pairs") and not inf["planar_mask"] & (1 << 17)
        y = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
        V.TrSpMV_(y, Cm, dev(x))
        outs[narrow] = (y.cpu().numpy(), inf)
        Cm.release()
    assert bitwise(outs["pairs"][0], outs[False][0]) and bitwise(outs["pairs"][0], outs["planar"][0])
    for k in outs[False][1]:
        if k not in BYTE_FIELDS:
            assert outs["pairs"][1][k] == outs[False][1][k], k
    assert outs[False][1]["device_bytes"] - outs["pairs"][1]["device_bytes"] >= 4 * A.nnz
    assert outs[False][1]["bytes_t"] - outs["pairs"][1]["bytes_t"] >= 4 * A.nnz
    assert rel(outs["pairs"][0], O.trspmv(A.astype(np.float64), x, np.zeros(n))) <= TOL64


@pytest.mark.parametrize("name", ["pair", "pair_masked", "pair_lanes"])
def test_update(knobs, lanes_matrix, name):
    """0x400 | 0x200: after update_values(val2) the product is bitwise that of a fresh 0x580 handle of val2; a float64
    val raises UnsupportedDtype and leaves the products unchanged."""
    if name == "pair_lanes":
        B = lanes_matrix[0]
        knobs(PAIR_LANES)
    else:
        B = ragged(3, 3, stripes=85, empty=(7,))
        knobs(PAIR, MASKED if name == "pair_masked" else {})
    rng = np.random.default_rng(61)
    val2 = rng.uniform(-2, 2, len(B.val)).astype(np.float32)
    val2[::11] = -0.0
    x, y0 = rng.uniform(-1, 1, B.m), rng.uniform(-1, 1, B.n)
    Bu = clone(B, "pairs")
    Bu.updatable = "narrow"
    inf = info64(Bu, True)
    assert inf["narrow_pair_t"] and inf["planar_pair"] == 1 and bool(inf["planar_mask"] & 4) == (name == "pair_lanes")
    fresh1, fresh2 = clone(B, "pairs"), clone(B, "pairs", val2)
    f1 = info64(fresh1, True)
    for k in inf:
        if k != "device_bytes":
            assert inf[k] == f1[k], k
    assert inf["device_bytes"] > f1["device_bytes"]  # the map
    before = [product(Bu, True, x, y0, a, b) for a, b in AB]
    for got, (a, b) in zip(before, AB):
        assert bitwise(got, product(fresh1, True, x, y0, a, b))
    with pytest.raises(L.UnsupportedDtype):
        Bu.update_values(val2.astype(np.float64))
    for got, (a, b) in zip(before, AB):
        assert bitwise(got, product(Bu, True, x, y0, a, b))  # unchanged
    Bu.update_values(dev(val2))
    for a, b in AB:
        got = product(Bu, True, x, y0, a, b)
        assert bitwise(got, product(fresh2, True, x, y0, a, b)), (a, b)
        assert not bitwise(got, before[AB.index((a, b))])
    Bu.update_values(B.val)  # and back, from the host
    for got, (a, b) in zip(before, AB):
        assert bitwise(got, product(Bu, True, x, y0, a, b))
    for M in (Bu, fresh1, fresh2):
        M.release()


def test_graph_replay(knobs, fwd_matrix):
    """A narrow pair B'x product and a forward pair product captured into a HIP graph replay to the eager bits."""
    knobs(PAIR)
    Bt = clone(ragged(3, 3, stripes=85), "pairs")
    assert info64(Bt, True)["narrow_pair_t"]
    knobs(FWD_PAIR)
    Bf = clone(fwd_matrix[0], "pairs")
    assert info64(Bf, False)["narrow_pair_f"]
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


def test_0x180_alone_leaves_pair_buckets_wide(knobs, fwd_matrix, lanes_matrix):
    """The documented behaviour of VBC_CREATE_NARROW_PLANAR stays: bits 16 / 17 clear, the byte counts the wide
    handle's, in the B'x pair, forward pair and pair-lanes layouts."""
    for env, B, trans in ((PAIR, ragged(3, 3, stripes=85), True), (FWD_PAIR, fwd_matrix[0], False),
                          (PAIR_LANES, lanes_matrix[0], True)):
        knobs(env)
        Bp, Bw = clone(B, "planar"), clone(B, False)
        a, c = info64(Bp, trans), info64(Bw, trans)
        assert a["planar_pair"] == 1 if trans else a["planar_mask"] & 2048
        assert not a["planar_mask"] & PAIR_BITS and not a["narrow_pair_t"] and not a["narrow_pair_f"]
        for k in a:
            assert a[k] == c[k], (k, a[k], c[k])
        Bp.release()
        Bw.release()
