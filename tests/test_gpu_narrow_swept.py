"""Narrow value storage of the row-swept kernel (vbc.h VBC_CREATE_NARROW_SWEPT, 0x1000, `B.narrow = "swept"`): on a
Float64 handle of a float32 matrix every bucket create lays out swept (spmv_sweep, B'x and forward) keeps Float32
values, lane l of step s at float offset (s * 64 + l) * w, widened in registers.  No layout decision changes, so every
vbc_info field but the byte counts and planar_mask bits 20 / 21 is that of the handle created with 0x80 and of the
wide handle, and every product is bit-identical to theirs; the oracle gets val.astype(float64).  Tolerance TOL64 of
test_gpu_parity.py.

The layout is forced with VBC_SWEEP=1, as tests/test_gpu_sweep.py does, and every case first checks through vbc_info
that `sweep_bins` is what it means to test and that bit 20 / 21 is set.  The 0x1080 handles pass exactly
VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_SWEPT (the Python ladder's "swept" passes 0x1D80: the update and the
auto-layout cases use it).  Shapes: m = 300 rows; 8 KB tiles hold 1024 / w stripes of a B'x bucket, so 260 stripes
are one tile (w <= 3), two with a last tile of 4 stripes (w = 4: its steps hold 4 entries and 60 padding lanes) or
three (w >= 7); 16 KB tiles halve that; 60 stripes of 2 rows make a tile of 2 steps, shorter than the 8 steps of
one pipeline stage (w = 1, 2), so the clamped loads past the tile's last step run."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_narrow_planar import bitwise, info64, product, ref1d
from tests.test_gpu_parity import TOL64, dev, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"

SWEPT = 0x1000
AB = ((1.0, 0.0), (0.5, -1.5))
KNOBS = ("VBC_SWEEP", "VBC_SWEEP_TILE", "VBC_SWEEP_PACK")
NARROW_KEYS = ("narrow_t", "narrow_f", "narrow_planar_t", "narrow_planar_f", "narrow_pair_t", "narrow_pair_f",
               "narrow_streams_t", "narrow_streams_f", "narrow_swept_t", "narrow_swept_f")
BYTE_FIELDS = ("device_bytes", "bytes_t", "bytes_f", "planar_mask") + NARROW_KEYS
SWEPT_BITS = (1 << 20) | (1 << 21)
OLDER_NARROW_BITS = 0xFF << 12  # bits 12 - 19


@pytest.fixture
def knobs(monkeypatch):
    def set_(tile="8", pack="1", sweep="1"):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if sweep is not None:
            monkeypatch.setenv("VBC_SWEEP", sweep)
        monkeypatch.setenv("VBC_SWEEP_TILE", tile)
        monkeypatch.setenv("VBC_SWEEP_PACK", pack)
    yield set_
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def swept_only(M):
    """M with `narrow = True` whose creates also pass VBC_CREATE_NARROW_SWEPT: exactly 0x1080."""
    M.narrow = True
    create = M._create

    def with_swept(out, device, flags, compute):
        return create(out, device, flags | (SWEPT if flags & L.VBC_CREATE_NARROW_VALUES else 0), compute)
    M._create = with_swept
    return M


def clone(B, narrow, val=None):
    """A fresh matrix object (its own handle cache: the knobs are read when a handle is created).  narrow: "1080",
    True (0x80), "swept" (0x1D80) or False."""
    M = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, B.val if val is None else val)
    if narrow == "1080":
        return swept_only(M)
    if narrow:
        M.narrow = narrow
    return M


def trio(B, val=None):
    """(0x1080, 0x80, wide) handles' matrices of one float32 matrix."""
    assert B.val.dtype == np.float32
    return clone(B, "1080", val), clone(B, True, val), clone(B, False, val)


def release(*Ms):
    for M in Ms:
        M.release()


def swept_values(B, max_w=8):
    """Stored values of the stripes of width <= max_w: those of the swept buckets under VBC_SWEEP=1."""
    w = np.diff(B.Phi.spl)
    return int(((np.diff(B.pos)) * w)[w <= max_w].sum())


def check_layout(Bs, Bn, Bw, trans, nbins, nval):
    """The 0x1080 handle has the swept buckets the case means to test, all narrow (bit 20 for B'x, 21 for forward), and
    differs from the 0x80 and the wide handle in bytes and in that bit only; bytes fall by at least 4 per stored value
    of the swept buckets (`nval`); the 0x80 handle's swept bytes are the wide handle's."""
    a, b, c = info64(Bs, trans), info64(Bn, trans), info64(Bw, trans)
    bit, key = (20, "narrow_swept_t") if trans else (21, "narrow_swept_f")
    assert a["sweep_bins"] == nbins and b["sweep_bins"] == nbins and c["sweep_bins"] == nbins, (a["sweep_bins"], nbins)
    assert a["planar_mask"] & (1 << bit) and a[key], hex(a["planar_mask"])
    assert not a["planar_mask"] & (SWEPT_BITS & ~(1 << bit)), hex(a["planar_mask"])
    for other in (b, c):
        assert not other["planar_mask"] & SWEPT_BITS, hex(other["planar_mask"])
        assert not other["narrow_swept_t"] and not other["narrow_swept_f"]
    assert not c["planar_mask"] & OLDER_NARROW_BITS
    assert a["planar_mask"] & OLDER_NARROW_BITS == b["planar_mask"] & OLDER_NARROW_BITS  # bits 12 - 19 keep their meaning
    for k in a:
        if k not in BYTE_FIELDS:
            assert a[k] == b[k] == c[k], (k, a[k], b[k], c[k])
    drop = ~(SWEPT_BITS | OLDER_NARROW_BITS)
    assert (a["planar_mask"] & drop) == (b["planar_mask"] & drop) == (c["planar_mask"] & drop)
    bk, other = ("bytes_t", "bytes_f") if trans else ("bytes_f", "bytes_t")
    print("trans", trans, bk, a[bk], b[bk], c[bk], "device_bytes", a["device_bytes"], b["device_bytes"], c["device_bytes"],
          "4 * swept values", 4 * nval)
    assert b[bk] - a[bk] >= 4 * nval
    assert b["device_bytes"] - a["device_bytes"] >= 4 * nval
    assert a[other] == b[other]
    return a, b, c, bk


def check_products(Bs, Bn, Bw, trans, R, seed):
    rng = np.random.default_rng(seed)
    nx, ny = (Bw.m, Bw.n) if trans else (Bw.n, Bw.m)
    x, y0 = rng.uniform(-1, 1, nx), rng.uniform(-1, 1, ny)
    for alpha, beta in AB:
        got = product(Bs, trans, x, y0, alpha, beta)
        assert bitwise(got, product(Bn, trans, x, y0, alpha, beta)), (trans, alpha, beta)
        assert bitwise(got, product(Bw, trans, x, y0, alpha, beta)), (trans, alpha, beta)
        err = rel(got, O.mul(R, x, y0.copy(), alpha, beta, trans=trans, ref_semantics=False))
        print("trans", trans, "alpha", alpha, "beta", beta, "rel err", err)
        assert err <= TOL64, (trans, alpha, beta)


def run_case(B, nbins, seed, all_swept=True, R=None):
    """Both directions of one matrix under the knobs already set."""
    R = ref1d(B) if R is None else R
    nval = swept_values(B)
    for trans in (True, False):
        Bs, Bn, Bw = trio(B)
        a, b, c, bk = check_layout(Bs, Bn, Bw, trans, nbins, nval)
        if all_swept:  # no slotted bucket: 0x80 alone stores what the wide handle stores
            assert b[bk] == c[bk] and b["device_bytes"] == c["device_bytes"]
        check_products(Bs, Bn, Bw, trans, R, seed)
        release(Bs, Bn, Bw)


def vbr(L_, q, widths, seed, W=8):
    return V.synthetic.vbr_1dvbc(300, L_, q, widths, W=W, dtype=np.float32, seed=seed)


# every width: the float load shapes 4 / 8 / 12 / 16 / 20 / 24 / 28 / 32 B; 60 + 25 w stripes (85 .. 260), 700 .. 3000 rows
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6, 7, 8])
def test_widths(knobs, w):
    knobs("8", "1")
    run_case(vbr(60 + 25 * w, 370 + 330 * w, w, seed=100 + w), 1, seed=10 + w)


@pytest.mark.parametrize("tile,pack", [("8", "1"), ("8", "0"), ("16", "1"), ("16", "0")])
def test_tiles_and_key_forms(knobs, tile, pack):
    """260 stripes 4 wide and 260 stripes 8 wide: 2 / 3 tiles of 8 KB, 1 / 2 of 16 KB, each with a partial last tile
    (4 stripes: steps of 4 entries, 60 padding lanes); packed and unpacked keys."""
    knobs(tile, pack)
    for w in (4, 8):
        B = vbr(260, 3000, w, seed=200 + w)
        run_case(B, 1, seed=20 + w)
    Bp = clone(B, "1080")
    a = info64(Bp, True)  # the handle (and its layout) is made now, under this setting
    knobs(tile, "1" if pack == "0" else "0")
    Bo = clone(B, "1080")
    o = info64(Bo, True)
    assert (a["bytes_t"] < o["bytes_t"]) == (pack == "1") and a["bytes_t"] != o["bytes_t"]  # the case got its key form
    release(Bp, Bo)


@pytest.mark.parametrize("w", [1, 2, 4])
def test_tile_shorter_than_a_stage(knobs, w):
    """60 stripes of ~2 rows: one tile of 2 - 3 steps, fewer than the U = 8 (w = 1, 2) or 4 (w = 4) steps of one pipeline
    stage, the last step partly padding: every load past S1 - 1 is clamped and never folded."""
    knobs("8", "1")
    B = vbr(60, 120, w, seed=300 + w)
    assert int(B.pos[-1]) - 1 <= 128
    run_case(B, 1, seed=30 + w)


def with_empty(B, empty):
    """B with the stripes in `empty` holding no rows."""
    keep = np.ones(len(B.idx), bool)
    cnt = np.diff(B.pos).copy()
    w = np.diff(B.Phi.spl)
    vkeep = np.ones(int(B.ofs[-1]) - 1, bool)
    for s in empty:
        keep[B.pos[s] - 1: B.pos[s + 1] - 1] = False
        vkeep[B.ofs[s] - 1: B.ofs[s + 1] - 1] = False
        cnt[s] = 0
    pos = np.concatenate([[1], 1 + np.cumsum(cnt)]).astype(np.int64)
    ofs = np.concatenate([[1], 1 + np.cumsum(cnt * w)]).astype(np.int64)
    val = np.concatenate([B.val[: vkeep.size][vkeep], np.zeros(8, np.float32)])
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, pos, B.idx[keep], ofs, val)


def test_empty_stripes(knobs):
    """Empty stripes inside a tile, and a tile made of empty stripes only (S0 == S1: 128 stripes 8 wide per 8 KB tile,
    stripes 128 .. 255 empty): their outputs are exactly 0 (beta = 0) or beta * y."""
    knobs("8", "1")
    B = with_empty(vbr(300, 3000, 8, seed=41), [3, 50, 127] + list(range(128, 256)))
    run_case(B, 1, seed=42)
    Bs = clone(B, "1080")
    rng = np.random.default_rng(43)
    y0 = rng.uniform(-1, 1, B.n)
    y = product(Bs, True, rng.uniform(-1, 1, B.m), y0, 1.0, 0.0)
    y2 = product(Bs, True, rng.uniform(-1, 1, B.m), y0, 0.5, -1.5)
    for s in (3, 50, 127, 128, 200, 255):
        assert not y[8 * s: 8 * s + 8].any()
        assert np.array_equal(y2[8 * s: 8 * s + 8], -1.5 * y0[8 * s: 8 * s + 8])
    assert y[8 * 256:].any()
    release(Bs)


def test_mixed_buckets(knobs):
    """Widths [3, 17, 64]: the 3-wide bucket is swept and narrow, the w > 8 buckets keep their own storage and bits."""
    knobs("8", "1")
    w = np.array([[3, 17, 64][i % 3] for i in range(90)])
    B = vbr(90, 900, w, seed=51, W=64)
    run_case(B, 1, seed=52, all_swept=False)


def test_special_values(knobs):
    """Float32 NaN, +-0.0, +-Inf, subnormals, FLT_MAX and tiny among the stored values: narrowing on the host and
    widening in the kernel give the wide handle's bits (no oracle: its NaN bits are the CPU's)."""
    knobs("8", "1")
    B = vbr(160, 1500, 5, seed=61)
    nval = int(B.ofs[-1]) - 1
    v = B.val.copy()
    fi = np.finfo(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max,
                        -fi.max, fi.tiny], np.float32)
    at = np.random.default_rng(8).choice(nval, 4 * len(special), replace=False)
    v[at] = np.tile(special, 4)
    rng = np.random.default_rng(9)
    for trans in (True, False):
        nx, ny = (B.m, B.n) if trans else (B.n, B.m)
        x, y0 = rng.uniform(0.5, 1.0, nx), rng.uniform(-1, 1, ny)
        Bs, Bn, Bw = trio(B, v)
        check_layout(Bs, Bn, Bw, trans, 1, nval)
        for alpha, beta in AB:
            got, wide = product(Bs, trans, x, y0, alpha, beta), product(Bw, trans, x, y0, alpha, beta)
            assert np.isnan(wide).any() and np.isinf(wide).any()
            assert bitwise(got, wide), (trans, alpha, beta)
            assert bitwise(got, product(Bn, trans, x, y0, alpha, beta)), (trans, alpha, beta)
        release(Bs, Bn, Bw)


def test_nonfinite_x_stays_in_place(knobs):
    """Padding lanes are skipped: an Inf / NaN of x reaches exactly the stripes (rows) that store its row (column)."""
    knobs("8", "1")
    B = vbr(60, 700, np.arange(60) % 4 + 1, seed=77)
    R = ref1d(B)
    rng = np.random.default_rng(8)
    Bs, Bw = clone(B, "1080"), clone(B, False)
    assert info64(Bs, True)["sweep_bins"] == 4 and info64(Bs, True)["narrow_swept_t"]
    assert info64(Bs, False)["sweep_bins"] == 4 and info64(Bs, False)["narrow_swept_f"]
    for trans, bad in ((True, (0, 17, 101)), (False, (0, 5, 33))):
        nx, ny = (B.m, B.n) if trans else (B.n, B.m)
        x = rng.uniform(-1, 1, nx)
        x[bad[0]], x[bad[1]], x[bad[2]] = np.nan, np.inf, -np.inf
        got = product(Bs, trans, x, np.zeros(ny), 1.0, 0.0)
        ref = O.mul(R, x, np.zeros(ny), trans=trans)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
        assert np.isfinite(ref).any() and not np.isfinite(ref).all()
        fin = np.isfinite(ref)
        assert rel(got[fin], ref[fin]) <= TOL64
        assert bitwise(got, product(Bw, trans, x, np.zeros(ny), 1.0, 0.0))
    release(Bs, Bw)


def test_2d_handle(knobs):
    """A 2D (SparseMatrixVBC) handle under VBC_SWEEP=1: bits 20 / 21, bitwise the 0x80 and the wide handle."""
    knobs("8", "1")
    A = sp.random(300, 240, density=0.04, random_state=5, format="csc", dtype=np.float64).astype(np.float32)
    x, xf = np.random.default_rng(6).uniform(-1, 1, 300), np.random.default_rng(7).uniform(-1, 1, 240)
    outs = {}
    for narrow in ("1080", True, False):
        M = V.SparseMatrixVBC[4, 4](A, V.AlternatingPacker(V.StrictChunker(4), V.StrictChunker(4)))
        if narrow == "1080":
            swept_only(M)
        elif narrow:
            M.narrow = True
        it, if_ = M.info(trans=True, compute=L.VBC_F64), M.info(trans=False, compute=L.VBC_F64)
        assert it["sweep_bins"] >= 1 and if_["sweep_bins"] >= 1
        assert it["narrow_swept_t"] == (narrow == "1080") and if_["narrow_swept_f"] == (narrow == "1080")
        assert not it["narrow_swept_f"] and not if_["narrow_swept_t"]
        outs[narrow] = (product(M, True, x, np.zeros(240), 0.5, -1.5), product(M, False, xf, np.zeros(300), 1.0, 0.0), it, if_)
        M.release()
    for k in (True, False):
        assert bitwise(outs["1080"][0], outs[k][0]) and bitwise(outs["1080"][1], outs[k][1])
    assert outs[False][2]["bytes_t"] > outs["1080"][2]["bytes_t"] and outs[False][3]["bytes_f"] > outs["1080"][3]["bytes_f"]
    D = A.astype(np.float64)
    assert rel(outs["1080"][0], 0.5 * (D.T @ x)) <= TOL64 and rel(outs["1080"][1], D @ xf) <= TOL64


def test_csc_operand(knobs):
    """TrSpMV! on a CSC operand (1-wide stripes) under VBC_SWEEP=1: bit 20 on the 0x1080 handle only."""
    knobs("8", "1")
    A = sp.random(300, 200, density=0.05, random_state=11, format="csc", dtype=np.float64).astype(np.float32)
    A.sort_indices()
    x = np.random.default_rng(12).uniform(-1, 1, 300)
    outs = {}
    for narrow in ("1080", True, False):
        Cm = V.SparseMatrixCSC(A)
        if narrow == "1080":
            swept_only(Cm)
        elif narrow:
            Cm.narrow = True
        inf = Cm.info(trans=True, compute=L.VBC_F64)
        assert inf["sweep_bins"] >= 1, inf
        assert bool(inf["planar_mask"] & (1 << 20)) == (narrow == "1080") and not inf["planar_mask"] & (1 << 21)
        y = torch.full((200,), float("nan"), dtype=torch.float64, device=DEV)
        V.TrSpMV_(y, Cm, dev(x))
        outs[narrow] = (y.cpu().numpy(), inf)
        Cm.release()
    assert bitwise(outs["1080"][0], outs[False][0]) and bitwise(outs["1080"][0], outs[True][0])
    for k in outs[False][1]:
        if k not in BYTE_FIELDS:
            assert outs["1080"][1][k] == outs[False][1][k] == outs[True][1][k], k
    for k in ("device_bytes", "bytes_t"):
        assert outs[False][1][k] - outs["1080"][1][k] >= 4 * A.nnz, k
    assert rel(outs["1080"][0], O.trspmv(A.astype(np.float64), x, np.zeros(200))) <= TOL64


@pytest.mark.parametrize("trans", [True, False])
def test_update(knobs, trans):
    """`B.narrow = "swept"` with `B.updatable = "narrow"` (0x1F80): after update_values(val2) the products are bitwise
    those of a fresh narrow handle of val2; a float64 val raises UnsupportedDtype and leaves the handle as it was."""
    knobs("8", "1")
    B = vbr(160, 1500, 4, seed=81)
    rng = np.random.default_rng(82)
    val2 = rng.uniform(-2, 2, len(B.val)).astype(np.float32)
    val2[::11] = -0.0
    nx, ny = (B.m, B.n) if trans else (B.n, B.m)
    x, y0 = rng.uniform(-1, 1, nx), rng.uniform(-1, 1, ny)
    Bu = clone(B, "swept")
    Bu.updatable = "narrow"
    inf = info64(Bu, trans)
    assert inf["sweep_bins"] == 1 and inf["narrow_swept_t" if trans else "narrow_swept_f"]
    fresh1, fresh2 = clone(B, "swept"), clone(B, "swept", val2)
    f1 = info64(fresh1, trans)
    for k in inf:
        if k != "device_bytes":
            assert inf[k] == f1[k], k
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
    release(Bu, fresh1, fresh2)


def test_no_swept_bucket_keeps_the_narrow_handle(knobs, monkeypatch):
    """Without VBC_SWEEP a banded matrix takes no swept bucket: the 0x1080 handle has the 0x80 handle's bytes, bits and
    products."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    B = V.synthetic.vbr_1dvbc_banded(3000, 700, 9000, 4, 64, W=8, dtype=np.float32, seed=91)
    R = ref1d(B)
    for trans in (True, False):
        Bs, Bn, Bw = trio(B)
        a, b = info64(Bs, trans), info64(Bn, trans)
        assert a["sweep_bins"] == 0 and not a["planar_mask"] & SWEPT_BITS
        assert a == b, {k: (a[k], b[k]) for k in a if a[k] != b[k]}
        check_products(Bs, Bn, Bw, trans, R, seed=92)
        release(Bs, Bn, Bw)
