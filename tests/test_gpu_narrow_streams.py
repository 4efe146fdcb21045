"""Narrow value storage of the lane-stream kernel (vbc.h VBC_CREATE_NARROW_STREAMS, `B.narrow = "streams"`): on a
Float64 handle of a float32 matrix the buckets of spmv_planar_lanes -- the per-lane compacted streams of B'x and the
forward lane streams -- keep Float32 values, rows of 64 * w floats in the Float32 column-group arrangement, widened in
registers.  No layout decision changes, so every vbc_info field but the byte counts and planar_mask bits 18 / 19 is
that of the handle created with 0x580 (`B.narrow = "pairs"`) and of the wide handle, and every product is
bit-identical to theirs; the oracle gets val.astype(float64).  Tolerances as in test_gpu_parity.py.

The layout is forced at small size with the layout knobs of INTEGRATION.md, and every case first checks through
vbc_info that it got the layout it means to test.  Shapes: m = 300 rows, so a lane's stream is shorter than one
pipeline step and the clamped loads past a range's end run; VBC_TARGET_RANGES_L = 1 / 8 / 256 gives one or two tiles
of all stripes (lanes walk several stripes), tiles of a few dozen stripes, and tiles of 4 stripes (most lanes dead)."""
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

# plain lane streams of spmv_planar_lanes at any size (no lane pairs, no split product, no fused small-matrix launch)
LANES = {"VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "0", "VBC_SLOTS": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0"}
FWD_LANES = {"VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "0", "VBC_PLANAR_PAIR": "0", "VBC_PLANAR_SPLIT": "0"}
ALL_KNOBS = sorted(set(LANES) | set(FWD_LANES) | {"VBC_TARGET_RANGES_L"})
NARROW_KEYS = ("narrow_t", "narrow_f", "narrow_planar_t", "narrow_planar_f", "narrow_pair_t", "narrow_pair_f",
               "narrow_streams_t", "narrow_streams_f")
BYTE_FIELDS = ("device_bytes", "bytes_t", "bytes_f", "planar_mask") + NARROW_KEYS
STREAM_BITS = (1 << 18) | (1 << 19)
OTHER_NARROW_BITS = (1 << 14) | (1 << 15) | (1 << 16) | (1 << 17)


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
    """(0xD80, 0x580, wide) handles' matrices of one float32 matrix."""
    assert B.val.dtype == np.float32
    return clone(B, "streams", val), clone(B, "pairs", val), clone(B, False, val)


def release(*Ms):
    for M in Ms:
        M.release()


def check_layout(Bs, Bp, Bw, trans, nval, run):
    """The handle is a plain lane-stream one, and differs from the 0x580 and the wide handle in bytes and in bit 18
    (B'x) or 19 (forward) only; the byte fields fall by at least 4 bytes per stored value (`nval`: the values of the
    lane bucket)."""
    a, b, c = info64(Bs, trans), info64(Bp, trans), info64(Bw, trans)
    bit, key = (18, "narrow_streams_t") if trans else (19, "narrow_streams_f")
    assert a["planar_mask"] & (4 if trans else 16), a["planar_mask"]  # bit 2: B'x lane streams, bit 4: forward ones
    assert a["planar_pair"] == 0 and not a["planar_mask"] & 2048, a
    assert a["planar_run" if trans else "fwd_run"] == run, a
    assert a["planar_mask"] & (1 << bit) and a[key], a["planar_mask"]
    assert not a["planar_mask"] & (STREAM_BITS & ~(1 << bit))
    assert not a["planar_mask"] & OTHER_NARROW_BITS, a["planar_mask"]  # bits 14 - 17 keep their meaning
    for other in (b, c):
        assert not other["planar_mask"] & (STREAM_BITS | OTHER_NARROW_BITS), other["planar_mask"]
        assert not other["narrow_streams_t"] and not other["narrow_streams_f"]
    for k in a:
        if k not in BYTE_FIELDS:
            assert a[k] == b[k] == c[k], (k, a[k], b[k], c[k])
    drop = ~(STREAM_BITS | (1 << 12) | (1 << 13))  # (bits 12 / 13: a slotted bucket beside the lanes, narrow since 0x80)
    assert (a["planar_mask"] & drop) == (b["planar_mask"] & drop) == (c["planar_mask"] & drop)
    bk, other = ("bytes_t", "bytes_f") if trans else ("bytes_f", "bytes_t")
    print("trans", trans, bk, a[bk], b[bk], c[bk], "device_bytes", a["device_bytes"], b["device_bytes"], c["device_bytes"],
          "4 * values", 4 * nval)
    return a, b, c, bk, other


def check_bytes(a, b, c, bk, other, nval):
    # 0x580 alone: the lane streams stay wide, byte for byte the wide handle's counts
    assert b[bk] == c[bk] and b["device_bytes"] == c["device_bytes"] and b[other] == c[other]
    assert b[bk] - a[bk] >= 4 * nval
    assert b["device_bytes"] - a["device_bytes"] >= 4 * nval
    assert a[other] == b[other]


def run_case(knobs, env, B, trans, run, seed, R=None, targets=("1", "8", "256"), extra=()):
    nval = int(B.ofs[-1]) - 1
    R = ref1d(B) if R is None else R
    for target in targets:
        knobs(env, {"VBC_TARGET_RANGES_L": target}, *extra)
        Bs, Bp, Bw = trio(B)
        check_bytes(*check_layout(Bs, Bp, Bw, trans, nval, run), nval)
        check_products(Bs, Bp, Bw, trans, R, seed)
        release(Bs, Bp, Bw)


# every width 3 .. 8 and every run length 1 .. 3: the load shapes 12 B, 16 B, 16 + 4, 16 + 8, 16 + 12 and 16 + 16
@pytest.mark.parametrize("w,run", [(3, 3), (3, 1), (4, 2), (5, 1), (6, 3), (7, 1), (8, 2)])
def test_bx_widths_runs_tiles(knobs, w, run):
    """spmv_planar_lanes<double, w, run, false, RD, 0, float>, both RD (the two (alpha, beta) of AB): 170 ragged
    stripes over m = 300 as one or two tiles, tiles of a few dozen stripes and tiles of 4.  (The DEEP form is instantiated as
    launch_stream (vbc_planar_launch.inc) has it, but VBC_LANES_DEEP is a tuning knob the product library does not read: no product test
    can launch it, for the wide kernel as for this one.)"""
    run_case(knobs, LANES, ragged(w, run, stripes=170), True, run, seed=70 + w)


@pytest.mark.parametrize("w,run,stripes,empty", [(3, 3, 85, (5, 40, 80)), (5, 1, 170, (0, 169))])
def test_bx_empty_stripes(knobs, w, run, stripes, empty):
    """Empty stripes are one zero run with PAD | LAST: inside a tile, and as a tile's first and last stripe."""
    B = ragged(w, run, stripes=stripes, empty=empty)
    run_case(knobs, LANES, B, True, run, seed=90 + w, targets=("1", "256"))
    knobs(LANES, {"VBC_TARGET_RANGES_L": "256"})
    Bs = clone(B, "streams")
    rng = np.random.default_rng(5)
    y = product(Bs, True, rng.uniform(-1, 1, B.m), rng.uniform(-1, 1, B.n), 1.0, 0.0)
    for s in empty:
        assert not y[s * w: (s + 1) * w].any()
    release(Bs)


def test_bx_special_values(knobs):
    """Float32 NaN, +-0.0, +-Inf, subnormals, FLT_MAX and tiny among the stored values: narrowing on the host and
    widening in the kernel give the wide handle's bits (no oracle: its NaN bits are the CPU's)."""
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
    for target in ("1", "256"):
        knobs(LANES, {"VBC_TARGET_RANGES_L": target})
        Bs, Bp, Bw = trio(B, v)
        check_bytes(*check_layout(Bs, Bp, Bw, True, nval, 3), nval)
        for alpha, beta in AB:
            got, wide = product(Bs, True, x, y0, alpha, beta), product(Bw, True, x, y0, alpha, beta)
            assert np.isnan(wide).any() and np.isinf(wide).any()
            assert bitwise(got, wide), (target, alpha, beta)
            assert bitwise(got, product(Bp, True, x, y0, alpha, beta)), (target, alpha, beta)
        release(Bs, Bp, Bw)


@pytest.fixture(scope="module")
def fwd_matrix():
    """tests/test_gpu_narrow_pairs.py's forward operand: a 3-dof stiffness matrix of 300 nodes, one node's rows and
    columns zeroed (empty segments and empty output rows of B); and its oracle."""
    A = V.synthetic.fe_stiffness_3d(900, 40000, 3, np.float32).tolil()
    A[30:33, :] = 0.0
    A[:, 30:33] = 0.0
    A = A.tocsc()
    A.eliminate_zeros()
    B = V.SparseMatrix1DVBC[8](A.T.tocsc(), V.StrictChunker(8))
    return B, ref1d(B)


@pytest.fixture(scope="module")
def fwd_matrix_w2():
    """Rows in runs of 3 on 2-wide stripes (tests/test_gpu_lanes.py test_forward_lanes' operand at 1500 rows), two
    node rows without blocks: the forward lane kernel with W = 3 outputs and runs of 2."""
    from tests.test_gpu_planar import sp_blocked
    rng = np.random.default_rng(23)
    base = V.synthetic.vbr_1dvbc(500, 450, 2400, 2, W=8, dtype=np.float32, seed=6)
    A = sp_blocked(base, 3, rng, np.float32).tolil()
    A[30:36, :] = 0
    A = A.tocsc()
    A.eliminate_zeros()
    B = V.SparseMatrix1DVBC[8](A, V.EquiChunker(2))
    return B, ref1d(B)


@pytest.mark.parametrize("which", ["w3", "w2"])
def test_forward_lane_streams(knobs, fwd_matrix, fwd_matrix_w2, which):
    """Forward lane streams (planar_mask bits 4 and 19): node blocks transposed into the lane-stream kernel; rows
    without blocks stay exactly zero."""
    B, R = fwd_matrix if which == "w3" else fwd_matrix_w2
    zero = slice(30, 33) if which == "w3" else slice(30, 36)
    run_case(knobs, FWD_LANES, B, False, 3, seed=41, R=R, targets=("8", "256"))
    knobs(FWD_LANES, {"VBC_TARGET_RANGES_L": "256"})
    Bs = clone(B, "streams")
    x = np.random.default_rng(42).uniform(-1, 1, B.n)
    got = product(Bs, False, x, np.zeros(B.m), 1.0, 0.0)
    assert not got[zero].any() and got.any()
    release(Bs)


@pytest.fixture(scope="module")
def fe3d():
    B = V.synthetic.fe_stiffness_3d_1dvbc(3000, 30000, dtype=np.float32)
    return B, ref1d(B)


# every lane knob but VBC_PLANAR_LANES at its default (the layout FE-3D takes by itself at full size); at 1000 stripes
# the split product and the fused small-matrix launch would come first
FE3D = {"VBC_PLANAR_LANES": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0"}


@pytest.mark.parametrize("target", ["8", "256"])
def test_fe3d_shape(knobs, fe3d, target):
    """FE-3D's 1000 node stripes (1 .. 19 node runs each) as plain lane streams: vbc_mul, and vbc_mul_ex's strided /
    converted path (a reversed y view of host memory), bitwise against the wide handle."""
    B, R = fe3d
    nval = int(B.ofs[-1]) - 1
    knobs(FE3D, {"VBC_TARGET_RANGES_L": target})
    Bs, Bp, Bw = trio(B)
    check_bytes(*check_layout(Bs, Bp, Bw, True, nval, 3), nval)
    check_products(Bs, Bp, Bw, True, R, seed=51)
    rng = np.random.default_rng(52)
    x, y0 = rng.uniform(-1, 1, B.m), rng.uniform(-1, 1, B.n)
    outs = []
    for M in (Bs, Bw):
        y = y0.copy()
        V.mul_(y[::-1], V.adjoint(M), x, -0.5, 2.0)
        outs.append(y)
    assert bitwise(outs[0], outs[1])
    assert bitwise(outs[0][::-1].copy(), product(Bs, True, x, y0[::-1].copy(), -0.5, 2.0))
    release(Bs, Bp, Bw)


def test_mul_mat_rowmajor(knobs, fe3d):
    """vbc_mul_mat, row-major, 4 right-hand sides, trans = 1 on the 0xD80 handle: the fused vector multi-RHS kernel reads
    the merge layout only (it is taken when the handle has no slotted, swept or planar bucket), so a handle with a
    lane bucket runs one SpMV per column through staging buffers -- the per-column path is what is tested here."""
    B, _ = fe3d
    knobs(FE3D, {"VBC_TARGET_RANGES_L": "8"})
    Bs, Bw = clone(B, "streams"), clone(B, False)
    assert info64(Bs, True)["narrow_streams_t"] and info64(Bs, True)["planar_mask"] & 4
    rng = np.random.default_rng(53)
    X, Y0 = rng.uniform(-1, 1, (B.m, 4)), rng.uniform(-1, 1, (B.n, 4))
    outs = []
    for M in (Bs, Bw):
        Y = dev(Y0.copy())
        V.mulmat_(Y, V.adjoint(M), dev(X), -0.5, 2.0, engine="vector")
        outs.append(Y.cpu().numpy())
    for c in range(4):
        assert bitwise(np.ascontiguousarray(outs[0][:, c]), np.ascontiguousarray(outs[1][:, c])), c
        assert bitwise(np.ascontiguousarray(outs[0][:, c]), product(Bw, True, X[:, c].copy(), Y0[:, c].copy(), -0.5, 2.0)), c
    release(Bs, Bw)


@pytest.mark.parametrize("name", ["bx", "forward"])
def test_update(knobs, fwd_matrix, name):
    """0xF80 (`B.narrow = "streams"`, `B.updatable = "narrow"`): after update_values(val2) the products are bitwise
    those of a fresh 0xD80 handle of val2; a float64 val raises UnsupportedDtype and leaves the products unchanged;
    the value map costs at least 4 bytes per stored slot."""
    trans = name == "bx"
    B = ragged(3, 3, stripes=170) if trans else fwd_matrix[0]
    knobs(LANES if trans else FWD_LANES, {"VBC_TARGET_RANGES_L": "8"})
    nval = int(B.ofs[-1]) - 1
    rng = np.random.default_rng(61)
    val2 = rng.uniform(-2, 2, len(B.val)).astype(np.float32)
    val2[::11] = -0.0
    nx, ny = (B.m, B.n) if trans else (B.n, B.m)
    x, y0 = rng.uniform(-1, 1, nx), rng.uniform(-1, 1, ny)
    Bu = clone(B, "streams")
    Bu.updatable = "narrow"
    inf = info64(Bu, trans)
    assert inf["narrow_streams_t" if trans else "narrow_streams_f"] and inf["planar_pair"] == 0
    assert inf["planar_mask"] & (4 if trans else 16)
    fresh1, fresh2 = clone(B, "streams"), clone(B, "streams", val2)
    f1 = info64(fresh1, trans)
    for k in inf:
        if k != "device_bytes":
            assert inf[k] == f1[k], k
    print("device_bytes", inf["device_bytes"], f1["device_bytes"], "4 * slots", 4 * nval)
    assert inf["device_bytes"] - f1["device_bytes"] >= 4 * nval  # the map: one 4-byte entry per stored slot at least
    before = [product(Bu, trans, x, y0, a, b) for a, b in AB]
    for got, (a, b) in zip(before, AB):
        assert bitwise(got, product(fresh1, trans, x, y0, a, b))
    with pytest.raises(L.UnsupportedDtype):
        Bu.update_values(val2.astype(np.float64))
    for got, (a, b) in zip(before, AB):
        assert bitwise(got, product(Bu, trans, x, y0, a, b))  # unchanged
    Bu.update_values(dev(val2))
    for a, b in AB:
        got = product(Bu, trans, x, y0, a, b)
        assert bitwise(got, product(fresh2, trans, x, y0, a, b)), (a, b)
        assert not bitwise(got, before[AB.index((a, b))])
    Bu.update_values(B.val)  # and back, from the host
    for got, (a, b) in zip(before, AB):
        assert bitwise(got, product(Bu, trans, x, y0, a, b))
    release(Bu, fresh1, fresh2)


def mixed_matrix():
    """85 stripes 3 wide with rows in runs of 3 (tests/test_gpu_narrow_planar.py's ragged shape: the lane bucket, its
    outputs contiguous) followed by 90 stripes 1 wide of 1 .. 12 rows (the slotted bucket), m = 300."""
    B3 = ragged(3, 3, stripes=85)
    rng = np.random.default_rng(77)
    cnt = rng.integers(1, 13, 90)
    idx1 = np.concatenate([np.sort(rng.choice(B3.m, c, replace=False)) for c in cnt]).astype(np.int64) + 1
    n3 = int(B3.pos[-1]) - 1  # stored rows of the 3-wide part
    v3 = int(B3.ofs[-1]) - 1
    spl = np.concatenate([B3.Phi.spl, B3.Phi.spl[-1] + 1 + np.arange(90)]).astype(np.int64)
    pos = np.concatenate([B3.pos, B3.pos[-1] + np.cumsum(cnt)]).astype(np.int64)
    ofs = np.concatenate([B3.ofs, B3.ofs[-1] + np.cumsum(cnt)]).astype(np.int64)
    idx = np.concatenate([B3.idx[:n3], idx1])
    val = np.concatenate([B3.val[:v3], rng.uniform(-1, 1, int(cnt.sum())).astype(np.float32)])
    return V.SparseMatrix1DVBC(8, B3.m, 85 * 3 + 90, V.SplitPartition(spl), pos, idx, ofs, val), v3


def test_mixed_slotted_and_lane_buckets_both_narrow(knobs):
    """A handle with a slotted (1-wide) and a lane-stream (3-wide, runs of 3) bucket: under 0xD80 both report narrow
    (bits 12 and 18), under 0x580 only the slotted one (bit 12); products bitwise equal across the trio."""
    B, v3 = mixed_matrix()
    nval = int(B.ofs[-1]) - 1
    knobs(LANES, {"VBC_TARGET_RANGES_L": "8"})
    Bs, Bp, Bw = trio(B)
    a, b, c, bk, other = check_layout(Bs, Bp, Bw, True, nval, 3)
    assert a["slot_bins"] - a["planar_bins"] >= 1, a  # (planar bins count as slotted ones in slot_bins)
    assert a["planar_mask"] & (1 << 12) and b["planar_mask"] & (1 << 12) and not c["planar_mask"] & (1 << 12)
    assert a["narrow_t"] and b["narrow_t"] and not c["narrow_t"]
    assert b[bk] - a[bk] >= 4 * v3 and b["device_bytes"] - a["device_bytes"] >= 4 * v3  # the lane bucket's values
    assert c[bk] - a[bk] >= 4 * nval and c["device_bytes"] - a["device_bytes"] >= 4 * nval  # and the slotted ones
    check_products(Bs, Bp, Bw, True, ref1d(B), seed=71)
    release(Bs, Bp, Bw)


def test_csc_operand(knobs):
    """TrSpMV! on a 3-dof stiffness operand (vbc_csc_create_ex groups a node's columns into a 3-wide stripe) under the
    lane knobs: bit 18 on the 0xD80 handle only, bitwise the wide handle's result."""
    knobs(LANES, {"VBC_TARGET_RANGES_L": "8"})
    A = V.synthetic.fe_stiffness_3d(900, 40000, 3, np.float32).tocsc()
    A.sort_indices()
    m, n = A.shape
    x = np.random.default_rng(12).uniform(-1, 1, m)
    outs = {}
    for narrow in ("streams", "pairs", False):
        Cm = V.SparseMatrixCSC(A)
        if narrow:
            Cm.narrow = narrow
        inf = Cm.info(trans=True, compute=L.VBC_F64)
        assert inf["planar_mask"] & 4 and inf["planar_pair"] == 0 and inf["planar_bins"] == 1 and inf["planar_run"] == 3, inf
        assert bool(inf["planar_mask"] & (1 << 18)) == (narrow == "streams") and not inf["planar_mask"] & (1 << 19)
        assert not inf["planar_mask"] & OTHER_NARROW_BITS
        y = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
        V.TrSpMV_(y, Cm, dev(x))
        outs[narrow] = (y.cpu().numpy(), inf)
        Cm.release()
    assert bitwise(outs["streams"][0], outs[False][0]) and bitwise(outs["streams"][0], outs["pairs"][0])
    for k in outs[False][1]:
        if k not in BYTE_FIELDS:
            assert outs["streams"][1][k] == outs[False][1][k] == outs["pairs"][1][k], k
    for k in ("device_bytes", "bytes_t"):
        assert outs["pairs"][1][k] == outs[False][1][k], k
        assert outs[False][1][k] - outs["streams"][1][k] >= 4 * A.nnz, k
    assert rel(outs["streams"][0], O.trspmv(A.astype(np.float64), x, np.zeros(n))) <= TOL64
