"""Narrow value storage of the slotted layout (vbc.h VBC_CREATE_NARROW_VALUES, `B.narrow = True`): a float32
matrix applied to Float64 vectors keeps its values as Float32 in device memory and the slotted kernel widens them
in registers.  Widening is exact and the flag changes no layout decision, so every product is bit-identical to
that of the same float32 matrix without the flag (the "wide" handle); the oracle gets val.astype(float64).
Tolerances as in test_gpu_parity.py: one-hot probes bit-exact, random x <= 1e-12 against the oracle."""
import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.conftest import sprand_family
from tests.test_gpu_parity import METHODS_1D, METHODS_2D, TOL64, dev, one_hot_probes, rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"

# vbc_info fields that may differ between the narrow and the wide handle of one matrix
BYTE_FIELDS = ("device_bytes", "bytes_t", "bytes_f", "planar_mask", "narrow_t", "narrow_f")
NARROW_BITS = (1 << 12) | (1 << 13)


def as_f32(B):
    """B (1DVBC) with float32 values."""
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, B.val.astype(np.float32))


def pair_of(make):
    """(narrow, wide): the same float32 matrix twice, one with B.narrow set."""
    Bn, Bw = make(), make()
    assert Bn.val.dtype == np.float32 and np.array_equal(Bn.val, Bw.val)
    Bn.narrow = True
    return Bn, Bw


def info64(B, trans):
    return B.info(trans=trans, compute=L.VBC_F64)


def same_layout(Bn, Bw, trans):
    """Every vbc_info field except the byte counts and bits 12 / 13 is the wide handle's."""
    a, b = info64(Bn, trans), info64(Bw, trans)
    for k in a:
        if k not in BYTE_FIELDS:
            assert a[k] == b[k], (k, a[k], b[k])
    assert (a["planar_mask"] & ~NARROW_BITS) == b["planar_mask"]
    assert not b["narrow_t"] and not b["narrow_f"]
    return a, b


def product(B, trans, x, y0=None, alpha=1.0, beta=0.0):
    ny = B.n if trans else B.m
    y = torch.full((ny,), float("nan"), dtype=torch.float64, device=DEV) if y0 is None else dev(y0)
    V.mul_(y, V.adjoint(B) if trans else B, dev(x), alpha, beta)
    return y.cpu().numpy()


def bitwise(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ref1d(B):
    return O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, B.val.astype(np.float64))


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("VBC_SLOTS", "1")
    yield monkeypatch
    monkeypatch.delenv("VBC_SLOTS", raising=False)


@pytest.fixture(scope="module")
def fe200():
    """The FE operator in its production layout: narrow and wide handle, the oracle's matrix."""
    Bn, Bw = pair_of(lambda: V.synthetic.fe_grid_2d(200, dof=2, dtype=np.float32))
    return Bn, Bw, ref1d(Bw)


def test_fe_layout_and_bytes(fe200):
    Bn, Bw, _ = fe200
    nval = int(Bw.ofs[-1]) - 1
    a, b = same_layout(Bn, Bw, True)
    print("bytes_t narrow", a["bytes_t"], "wide", b["bytes_t"], "device_bytes", a["device_bytes"], b["device_bytes"],
          "4*nval", 4 * nval)
    assert a["narrow_t"] and a["slot_bins"] == b["slot_bins"] == 1
    assert 4 * nval <= b["bytes_t"] - a["bytes_t"] <= 1.10 * 4 * nval
    assert b["device_bytes"] - a["device_bytes"] >= 4 * nval
    af, bf = same_layout(Bn, Bw, False)
    if af["narrow_f"]:
        assert 4 * nval <= bf["bytes_f"] - af["bytes_f"] <= 1.10 * 4 * nval
        assert bf["device_bytes"] - af["device_bytes"] >= 4 * nval
    else:  # the forward bucket is not slotted: nothing changes
        assert af["bytes_f"] == bf["bytes_f"] and af["device_bytes"] == bf["device_bytes"]


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-0.5, 2.0)])  # the second pair: the non-FASTE path
def test_fe_products(fe200, alpha, beta):
    Bn, Bw, R = fe200
    rng = np.random.default_rng(31)
    assert info64(Bn, True)["narrow_t"]
    for trans, nx, ny in ((True, Bw.m, Bw.n), (False, Bw.n, Bw.m)):
        x, y0 = rng.uniform(-1, 1, nx), rng.uniform(-1, 1, ny)
        got = product(Bn, trans, x, y0, alpha, beta)
        wide = product(Bw, trans, x, y0, alpha, beta)
        assert bitwise(got, wide), trans
        ref = O.mul(R, x, y0.copy(), alpha, beta, trans=trans, ref_semantics=False)
        err = rel(got, ref)
        print("trans", trans, "alpha", alpha, "beta", beta, "rel err", err)
        assert err <= TOL64, trans


def golden_f32(golden, key):
    A = golden[key]["A"].astype(np.float32)
    A.sort_indices()
    return A


@pytest.mark.parametrize("meth", range(len(METHODS_1D)))
def test_forced_golden_one_hot_1d(golden, forced, meth):
    for key in golden:
        A = golden_f32(golden, key)
        B = V.SparseMatrix1DVBC[4](A, METHODS_1D[meth]())
        B.narrow = True
        assert info64(B, True)["narrow_t"] and info64(B, False)["narrow_f"], key
        one_hot_probes(B, A)


def test_forced_golden_one_hot_2d(golden, forced):
    for key in golden:
        A = golden_f32(golden, key)
        B = V.SparseMatrixVBC[4, 4](A, METHODS_2D[1]())
        B.narrow = True
        assert info64(B, True)["narrow_t"] and info64(B, False)["narrow_f"], key
        one_hot_probes(B, A)


@pytest.mark.parametrize("knob,value", [("VBC_SLOT_KEYS16", "0"), ("VBC_SLOT_STAGE", "0"), ("VBC_SLOT_STAGE", "4")])
def test_forced_golden_one_hot_key_and_stage_forms(golden, forced, knob, value):
    forced.setenv(knob, value)
    A = golden_f32(golden, "HB__west0132")
    B = V.SparseMatrix1DVBC[4](A, METHODS_1D[1]())
    B.narrow = True
    assert info64(B, True)["narrow_t"] and info64(B, False)["narrow_f"]
    one_hot_probes(B, A)


def wide_cases():
    """Stripes wider than 8 (the runtime-width kernel): the widest sprand_family shapes as one stripe of up to
    17 columns, and the wide buckets of test_gpu_slots.py's test_forced_widths."""
    cases = []
    for name, A in sprand_family(trials=1, kinds=("f64",)):
        if A.shape[1] == 17 and A.shape[0] in (16, 17):
            A32 = A.astype(np.float32)
            cases.append((name, lambda A32=A32: V.SparseMatrix1DVBC[17](A32, V.EquiChunker(17))))
    for widths in ([9, 12, 16], [17, 31, 33, 64]):
        w = np.array([widths[i % len(widths)] for i in range(70)])
        cases.append((str(widths), lambda w=w: as_f32(V.synthetic.vbr_1dvbc(400, 70, 1400, w, W=64, seed=int(w.sum()) + 1))))
    return cases


@pytest.mark.parametrize("name,make", wide_cases(), ids=[c[0] for c in wide_cases()])
def test_forced_runtime_width(forced, name, make):
    Bn, Bw = pair_of(make)
    assert int(np.diff(Bw.Phi.spl).max()) > 8
    rng = np.random.default_rng(41)
    for trans, nx, ny in ((True, Bw.m, Bw.n), (False, Bw.n, Bw.m)):
        a, _ = same_layout(Bn, Bw, trans)
        assert a["narrow_t" if trans else "narrow_f"], trans
        x, y0 = rng.uniform(-1, 1, nx), rng.uniform(-1, 1, ny)
        for alpha, beta in ((1.0, 0.0), (0.5, -1.5)):
            assert bitwise(product(Bn, trans, x, y0, alpha, beta), product(Bw, trans, x, y0, alpha, beta)), (trans, alpha)
        assert rel(product(Bn, trans, x), O.mul(ref1d(Bw), x, np.zeros(ny), trans=trans)) <= TOL64


def test_fe_nonfinite_and_unaligned_x():
    """The construction of test_gpu_slots.py's test_fe_nonfinite_and_unaligned_x on the float32 FE matrix, and
    +-Inf among the stored values."""
    Bn, Bw = pair_of(lambda: V.synthetic.fe_grid_2d(120, dof=2, dtype=np.float32))
    assert info64(Bn, True)["narrow_t"]
    rng = np.random.default_rng(23)
    x = rng.uniform(-1, 1, Bw.m)
    x[[0, 7, 501, Bw.m - 1]] = [np.nan, np.inf, -np.inf, np.nan]
    ref = O.mul(ref1d(Bw), x, np.zeros(Bw.n), trans=True)
    for off in (0, 1):
        buf = torch.zeros(Bw.m + 1, dtype=torch.float64, device=DEV)
        buf[off:off + Bw.m] = dev(x)
        got = []
        for B in (Bn, Bw):
            y = torch.zeros(B.n, dtype=torch.float64, device=DEV)
            V.mul_(y, B.T, buf[off:off + B.m])
            got.append(y.cpu().numpy())
        n, w = got
        assert np.array_equal(np.isnan(n), np.isnan(w)) and np.array_equal(np.isinf(n), np.isinf(w)), off
        assert np.array_equal(np.isnan(n), np.isnan(ref)) and np.array_equal(np.isinf(n), np.isinf(ref)), off
        fin = np.isfinite(w)
        assert bitwise(n[fin], w[fin]), off
        assert np.array_equal(n[np.isfinite(ref)], ref[np.isfinite(ref)]), off

    def with_inf():
        B = V.synthetic.fe_grid_2d(120, dof=2, dtype=np.float32)
        v = B.val.copy()
        v[3], v[int(B.ofs[-1]) - 5] = np.inf, -np.inf
        return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, v)
    Cn, Cw = pair_of(with_inf)
    xs = rng.uniform(0.5, 1, Cw.m)  # positive: an infinite value gives that sign's infinity, no NaN from inf - inf
    n, w = product(Cn, True, xs), product(Cw, True, xs)
    assert np.isposinf(n).sum() == 1 and np.isneginf(n).sum() == 1 and not np.isnan(n).any()
    assert bitwise(n, w)


def test_no_slotted_bucket_is_a_no_op():
    """The 3D stiffness stand-in at the planar tests' size runs the lane-stream layouts: nothing is stored narrow."""
    Bn, Bw = pair_of(lambda: V.synthetic.fe_stiffness_3d_1dvbc(300000, 3_000_000, dtype=np.float32))
    rng = np.random.default_rng(7)
    for trans, nx in ((True, Bw.m), (False, Bw.n)):
        a, b = same_layout(Bn, Bw, trans)
        assert not a["narrow_t"] and not a["narrow_f"]
        assert a["bytes_t"] == b["bytes_t"] and a["bytes_f"] == b["bytes_f"] and a["device_bytes"] == b["device_bytes"]
        x = rng.uniform(-1, 1, nx)
        assert bitwise(product(Bn, trans, x), product(Bw, trans, x)), trans


def mixed_matrix():
    """Banded stripes of about 10 rows, widths 2 and 3 alternating: by default the 2-wide bucket of B'x is slotted and
    the 3-wide one planar (an fp64 row of 24 B takes one stripe per lane).  300,000 stripes: with fewer chunks
    than half the chip's wave slots every bucket would join the fused small-matrix split, which is planar."""
    L_ = 300000
    w = np.where(np.arange(L_) % 2 == 0, 2, 3)
    return as_f32(V.synthetic.vbr_1dvbc_banded(600000, L_, 10 * L_, w, band=400, W=8, seed=19))


def test_mixed_narrow_and_wide_buckets():
    Bn, Bw = pair_of(mixed_matrix)
    a, b = same_layout(Bn, Bw, True)
    slotted = a["slot_bins"] - a["planar_bins"]  # planar bins count as slotted ones in slot_bins
    print("slot_bins", a["slot_bins"], "planar_bins", a["planar_bins"], "bins_t", a["bins_t"], "sweep", a["sweep_bins"])
    assert slotted >= 1 and a["planar_bins"] + a["bins_t"] + a["sweep_bins"] >= 1
    assert a["narrow_t"]
    widths = np.diff(Bw.Phi.spl)
    rows = np.diff(Bw.pos)
    vals2 = int((rows[widths == 2] * 2).sum())  # the values of the slotted (2-wide) bucket
    assert b["bytes_t"] - a["bytes_t"] >= 4 * vals2
    assert b["device_bytes"] - a["device_bytes"] >= 4 * vals2
    assert b["bytes_t"] - a["bytes_t"] < 4 * (int(Bw.ofs[-1]) - 1)  # the 3-wide bucket stays wide
    rng = np.random.default_rng(9)
    x, y0 = rng.uniform(-1, 1, Bw.m), rng.uniform(-1, 1, Bw.n)
    for alpha, beta in ((1.0, 0.0), (-0.5, 2.0)):
        got = product(Bn, True, x, y0, alpha, beta)
        assert bitwise(got, product(Bw, True, x, y0, alpha, beta))
        assert rel(got, O.mul(ref1d(Bw), x, y0.copy(), alpha, beta, trans=True, ref_semantics=False)) <= TOL64


def test_graph_replay(fe200):
    Bn, _, _ = fe200
    x = torch.rand(Bn.m, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    y_e = [torch.full((Bn.n,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        V.mul_(y_e[0], Bn.T, x)
        V.mul_(y_e[1], Bn.T, x, 0.5, 0.0)
    torch.cuda.synchronize()
    y_g = [torch.full((Bn.n,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        V.mul_(y_g[0], Bn.T, x)
        V.mul_(y_g[1], Bn.T, x, 0.5, 0.0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(y_g, y_e):
        assert torch.equal(a, b) and not torch.isnan(a).any()
