"""Every product path of the C ABI captured into a HIP graph (torch.cuda.CUDAGraph) and replayed.

tests/test_gpu_graph.py captures the SpMV layouts; this file captures the paths that keep state in the handle or go
through more than one kernel: the matrix-core panels and tiles, the fused merge multi-RHS kernel (spmm_ranges and its
carry buffer), the row-major per-column path (strided copies through the column temporaries), the column-major
per-column loop, vbc_mul_ex on strided and converted device operands (gather, product, scatter), the integer kernels
and VBC_MUL_REFERENCE_QUIRKS.

Per case (replayed): the handle is built, the call runs once eagerly on the stream (the warm-up vbc.h asks for), is
captured with the output window filled with NaN (integers: a sentinel), and is replayed three times.  Before each
replay the inputs are overwritten in place with new seeded data and the output is put back to its start (y0 where
beta != 0, NaN otherwise; a canary in every element that is not the operand's); after it the whole output buffer is
compared bit for bit with an eager product of the same inputs on a second handle of the same matrix, the elements
outside the window with the canary, and the window is finite.  Integer results are also compared with numpy's
wrapping Int64 arithmetic, exactly.

Capture before the first use: three paths allocate a cached buffer of the handle the first time they run (the
staging buffers of vbc_mul_ex and of the row-major per-column path, the carry buffer of the fused merge kernel).
Inside a capture the library must notice that before it frees or allocates anything: VBC_INVALID_ARG, a message that
says to run the product once outside the capture, and a capture that stays valid.  Those tests use integer matrix
values and operands, so every partial sum is exact and the eager product equals the float64 oracle bit for bit."""
import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from tests.test_gpu_eltypes import expected, int_matrix
from tests.test_gpu_mfma import _vbc2d_mixed_heights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
CANARY = -7.0
SENTINEL = -(2 ** 31) // 3  # what an integer output holds where a float one holds NaN
REPLAYS = 3
F32_F64 = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
KNOBS = ("VBC_SLOTS", "VBC_SWEEP", "VBC_FWD_T", "VBC_MM_SLOTS", "VBC_FORK", "VBC_SMALL_FUSE", "VBC_PANEL_TILES")
MERGE = {"VBC_SLOTS": "0", "VBC_SWEEP": "0"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.detach().cpu().numpy()
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


_LIVE = []


@pytest.fixture(autouse=True)
def release_handles():
    yield
    for M in _LIVE:
        M.release()
    _LIVE.clear()


def knobs(monkeypatch, kv):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def two(make):
    """Two matrix objects of the same matrix: the captured handle's and the eager reference's."""
    Ms = (make(), make())
    _LIVE.extend(Ms)
    return Ms


def vbr(dt=np.float64):
    """3000 x 2446, stripes 1..6 wide (the matrix of test_gpu_graph.py)."""
    return V.synthetic.vbr_1dvbc(3000, 700, 9000, np.arange(700) % 6 + 1, W=8, dtype=dt, seed=3)


def with_integer_values(B, dt=np.float64, seed=1):
    """B's pattern with integer values in [-8, 8] (tests/test_gpu_operand_views.py: every partial sum exact)."""
    rng = np.random.default_rng(seed)
    val = np.zeros(len(B.val), dt)
    nv = int(B.ofs[-1]) - 1
    val[:nv] = rng.integers(1, 9, nv) * rng.choice([-1, 1], nv)
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, val)


# ---------------------------------------------------------------------------------------------------------------
# operands: a case owns its input tensors and knows the start of its output buffer for every replay
# ---------------------------------------------------------------------------------------------------------------

def uniform(rng, shape, dt):
    """Floats in [-1, 1); integers over the whole range of the eltype (the Int64 kernels wrap)."""
    if dt.kind == "f":
        return rng.uniform(-1, 1, shape).astype(dt)
    return rng.integers(np.iinfo(dt).min, np.iinfo(dt).max + 1, shape).astype(dt)


def small_integers(rng, shape, dt):
    """Integers in [-8, 8]: with integer matrix values every partial sum is exact."""
    return rng.integers(-8, 9, shape).astype(dt)


class MatCase:
    """vbc_mul_mat on device operands.  Row-major: X is nx x ld, Y is ny x ld with ld = nrhs + pad; column-major: X
    is nrhs x (nx + pad), Y is nrhs x (ny + pad).  The pad elements of X hold NaN, those of Y the canary."""

    def __init__(self, M, trans, nrhs, rowmajor, dt, alpha, beta, pad=0, flags=0, seed=0, draw=None):
        self.nx, self.ny = (M.m, M.n) if trans else (M.n, M.m)
        self.trans, self.nrhs, self.rowmajor, self.dt, self.alpha, self.beta = int(trans), nrhs, rowmajor, dt, alpha, beta
        self.flags = flags | (L.VBC_MAT_ROWMAJOR if rowmajor else 0)
        self.seed, self.pad, self.draw = seed, pad, draw or uniform
        self.ldx, self.ldy = (nrhs + pad, nrhs + pad) if rowmajor else (self.nx + pad, self.ny + pad)
        self.ins = [dev(self.new_inputs(0)[0])]

    def _embed(self, A, fill):
        """The nrows x nrhs operand A in its buffer."""
        A = A if self.rowmajor else A.T
        buf = np.full((A.shape[0], A.shape[1] + self.pad), fill, self.dt)
        buf[:, :A.shape[1]] = A
        return buf

    def window(self, buf):
        w = buf[:, :buf.shape[1] - self.pad]
        return w if self.rowmajor else w.T

    def x(self, k):
        return self.draw(np.random.default_rng([self.seed, k, 0]), (self.nx, self.nrhs), np.dtype(self.dt))

    def y0(self, k):
        return self.draw(np.random.default_rng([self.seed, k, 1]), (self.ny, self.nrhs), np.dtype(self.dt))

    def new_inputs(self, k):
        return [self._embed(self.x(k), np.nan)]

    def y_start(self, k, capture=False):
        Y0 = self.y0(k)
        if capture or self.beta == 0:
            Y0[:] = np.nan
        return self._embed(Y0, CANARY)

    def call(self, h, y, stream, flags=None, alpha=None, beta=None):
        L.check(L.lib().vbc_mul_mat(h, self.trans, self.nrhs, self.ins[0].data_ptr(), self.ldx, self.nx, y.data_ptr(),
                                    self.ldy, self.ny, self.alpha if alpha is None else alpha,
                                    self.beta if beta is None else beta, L.VBC_MEM_DEVICE, stream,
                                    self.flags if flags is None else flags), "vbc_mul_mat")


class VecCase:
    """vbc_mul_ex on device operands (contiguous ones of the compute eltype: it hands them to vbc_mul): x of
    eltype xdt strided by incx, y of eltype ydt strided by incy (negative: a reversed view whose first element is
    the buffer's last).  The elements between the strides hold NaN (x; integers: the sentinel) and the canary (y)."""

    def __init__(self, M, trans, xdt, incx, ydt, incy, alpha, beta, flags=0, seed=0, draw=None):
        self.nx, self.ny = (M.m, M.n) if trans else (M.n, M.m)
        self.trans, self.xdt, self.incx, self.ydt, self.incy = int(trans), np.dtype(xdt), incx, np.dtype(ydt), incy
        self.alpha, self.beta, self.flags, self.seed, self.draw = alpha, beta, flags, seed, draw or uniform
        self.ins = [dev(self.new_inputs(0)[0])]
        self.first = 0 if incy > 0 else abs(incy) * self.ny - 1

    def window(self, buf):
        return buf[::self.incy] if self.incy > 0 else buf[::-1][::-self.incy]

    def x(self, k):
        return self.draw(np.random.default_rng([self.seed, k, 0]), self.nx, self.xdt)

    def y0(self, k):
        return self.draw(np.random.default_rng([self.seed, k, 1]), self.ny, self.ydt)

    def new_inputs(self, k):
        buf = np.full(abs(self.incx) * self.nx, np.nan if self.xdt.kind == "f" else SENTINEL, self.xdt)
        buf[::self.incx] = self.x(k)
        return [buf]

    def y_start(self, k, capture=False):
        buf = np.full(abs(self.incy) * self.ny, CANARY, self.ydt)
        w = self.window(buf)
        w[:] = self.y0(k)
        if capture or self.beta == 0:
            w[:] = np.nan if self.ydt.kind == "f" else SENTINEL
        return buf

    def call(self, h, y, stream, flags=None, alpha=None, beta=None):
        alpha, beta = self.alpha if alpha is None else alpha, self.beta if beta is None else beta
        flags = self.flags if flags is None else flags
        yp = y.data_ptr() + self.first * self.ydt.itemsize
        L.check(L.lib().vbc_mul_ex(h, self.trans, self.ins[0].data_ptr(), L.dtype_code(self.xdt), self.incx, self.nx, yp,
                                   L.dtype_code(self.ydt), self.incy, self.ny, float(alpha), float(beta),
                                   L.VBC_MEM_DEVICE, stream, flags), "vbc_mul_ex")


def outside(case, buf):
    """The elements of a y buffer (host array) that are not the operand's."""
    m = np.ones(buf.shape, bool)
    case.window(m)[...] = False
    return buf[m]


def capture(case, h, y, s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        case.call(h, y, torch.cuda.current_stream().cuda_stream)
    return g


def replayed(case, hg, he, extra=None, eager=None):
    """The protocol of the module docstring.  extra(k, window): a further check of replay k's result (host array);
    eager(y, stream): the eager reference call, when it is not simply case.call on the second handle."""
    s = torch.cuda.Stream()
    yg, ye = dev(case.y_start(0)), dev(case.y_start(0))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        case.call(hg, yg, s.cuda_stream)  # warm-up: the first use of every cached buffer of the handle
    torch.cuda.synchronize()
    yg.copy_(dev(case.y_start(0, capture=True)))
    torch.cuda.synchronize()
    g = capture(case, hg, yg, s)
    for k in range(1, REPLAYS + 1):
        for t, a in zip(case.ins, case.new_inputs(k)):
            t.copy_(dev(a))
        start = case.y_start(k)
        yg.copy_(dev(start))
        ye.copy_(dev(start))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        if eager is None:
            case.call(he, ye, stream)
        else:
            eager(ye, stream)
        torch.cuda.synchronize()
        assert np.array_equal(bits(yg), bits(ye)), ("graph replay differs from the eager product", k)
        got = yg.cpu().numpy()
        assert np.array_equal(outside(case, got), outside(case, start)), \
            ("canary overwritten", k)
        win = case.window(got)
        assert np.isfinite(win).all() if win.dtype.kind == "f" else (win != SENTINEL).any(), k
        assert not np.array_equal(win, case.window(start))
        if extra:
            extra(k, win)


# ---------------------------------------------------------------------------------------------------------------
# replayed paths
# ---------------------------------------------------------------------------------------------------------------

@F32_F64
@pytest.mark.parametrize("rowmajor", [True, False], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("nrhs", [5, 70])
def test_panels_transposed(monkeypatch, nrhs, rowmajor, dt):
    """spmm_panel, B'X on a VBC_CREATE_MULTI handle: one pass (5) and a second pass of 6 columns (70)."""
    knobs(monkeypatch, {"VBC_PANEL_TILES": "0"})
    Mg, Me = two(lambda: vbr(dt))
    inf = Mg.info(trans=True, multi=True)
    assert inf["bins_m"] > 0 and not inf["planar_mask"] & 512, inf
    case = MatCase(Mg, True, nrhs, rowmajor, dt, 0.5, -1.25, seed=nrhs)
    replayed(case, Mg.handle(0, True, multi=True), Me.handle(0, True, multi=True))


@F32_F64
@pytest.mark.parametrize("rowmajor", [True, False], ids=["rowmajor", "colmajor"])
def test_panels_forward(monkeypatch, rowmajor, dt):
    """B X on a VBC_CREATE_MULTI_FORWARD handle (the panel layout of the transpose), 17 columns."""
    knobs(monkeypatch, {"VBC_PANEL_TILES": "0"})
    Mg, Me = two(lambda: vbr(dt))
    inf = Mg.info(trans=False, multi=True)
    assert inf["bins_m"] > 0 and not inf["planar_mask"] & 512, inf
    case = MatCase(Mg, False, 17, rowmajor, dt, 0.5, -1.25, seed=17)
    replayed(case, Mg.handle(0, False, multi=True), Me.handle(0, False, multi=True))


@F32_F64
@pytest.mark.parametrize("trans", [True, False], ids=["BtX", "BX"])
def test_tiles(monkeypatch, trans, dt):
    """spmm_tiles (planar_mask bit 9) on block rows of heights 1..4, 16 row-major columns, both directions."""
    knobs(monkeypatch, {"VBC_PANEL_TILES": "1"})
    Mg, Me = two(lambda: _vbc2d_mixed_heights(np.random.default_rng(61), 300, 400, 1200, (3, 1, 4, 2, 3),
                                              (1, 3, 2, 4, 3), dt))
    inf = Mg.info(trans=trans, multi=True)
    assert inf["bins_m"] > 0 and inf["planar_mask"] & 512, inf
    case = MatCase(Mg, trans, 16, True, dt, 0.5, -1.25, seed=16)
    replayed(case, Mg.handle(0, trans, multi=True), Me.handle(0, trans, multi=True))


def merge_fixed(M):
    """Merge bins of compile-time widths alone: row-major B'X runs spmm_ranges / fixup_mm with the carry buffer."""
    assert np.diff(M.Phi.spl).max() <= 8
    inf = M.info(trans=True)
    assert inf["bins_t"] > 0 and inf["slot_bins"] == 0 and inf["sweep_bins"] == 0 and inf["planar_bins"] == 0, inf
    return M.handle(0, True)


@F32_F64
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.5, -1.25)])
@pytest.mark.parametrize("nrhs", [16, 70])
def test_fused_merge(monkeypatch, nrhs, alpha, beta, dt):
    """spmm_ranges<T, 16, K> (16 columns) and <T, 64, K> plus a second chunk of 6 columns (70)."""
    knobs(monkeypatch, MERGE)
    Mg, Me = two(lambda: vbr(dt))
    replayed(MatCase(Mg, True, nrhs, True, dt, alpha, beta, seed=nrhs), merge_fixed(Mg), merge_fixed(Me))


@F32_F64
@pytest.mark.parametrize("trans", [True, False], ids=["BtX-swept", "BX-forward"])
def test_rowmajor_per_column(monkeypatch, trans, dt):
    """Row-major operands on a layout the fused kernels do not read: per column through the column temporaries
    (two strided copies and, since beta != 0, a third).  X and Y are views of wider matrices (ld = nrhs + 2)."""
    knobs(monkeypatch, {"VBC_SWEEP": "1"} if trans else {})
    Mg, Me = two(lambda: vbr(dt))
    inf = Mg.info(trans=trans)
    assert inf["bins_m"] == 0, inf
    if trans:
        assert inf["sweep_bins"] > 0 and not inf["planar_mask"] & (1 << 22), inf
    case = MatCase(Mg, trans, 3, True, dt, 0.5, -1.25, pad=2, seed=3)
    assert case.ldy > case.nrhs
    replayed(case, Mg.handle(0, trans), Me.handle(0, trans))


@F32_F64
@pytest.mark.parametrize("trans", [True, False], ids=["BtX", "BX"])
def test_colmajor_per_column(monkeypatch, trans, dt):
    """Column-major operands without panels: one SpMV per column straight on the caller's columns."""
    knobs(monkeypatch, {})
    Mg, Me = two(lambda: vbr(dt))
    assert Mg.info(trans=trans)["bins_m"] == 0
    case = MatCase(Mg, trans, 3, False, dt, 0.5, -1.25, pad=1, seed=4)
    replayed(case, Mg.handle(0, trans), Me.handle(0, trans))


@pytest.mark.parametrize("incy", [-1, 2])
@pytest.mark.parametrize("trans", [True, False], ids=["Btx", "Bx"])
def test_mul_ex_strided_converted(monkeypatch, trans, incy):
    """vbc_mul_ex on a Float64 handle: Float32 x strided by 3 (convert_gather into d_stage[0]), y reversed or
    strided by 2 with beta != 0 (gathered into d_stage[1], scattered back); the elements of y between the strides
    keep their canary."""
    knobs(monkeypatch, {})
    Mg, Me = two(vbr)
    case = VecCase(Mg, trans, np.float32, 3, np.float64, incy, 0.5, -1.25, seed=5)
    replayed(case, Mg.handle(0, trans), Me.handle(0, trans))


@pytest.mark.parametrize("trans", [True, False], ids=["Btx", "Bx"])
def test_integer_handle(trans):
    """An Int32 matrix computing in Int64 (B x: int_scale and the atomic kernel), x of the full Int32 range
    converted and y stored as Int32 through vbc_mul_ex, (alpha, beta) = (3, -2): every replay equals numpy's
    wrapping Int64 arithmetic truncated to Int32 (test_gpu_eltypes.py::expected), exactly."""
    A = int_matrix(300, 200, "i32", np.random.default_rng(7), 0.05)
    Mg, Me = two(lambda: V.SparseMatrix1DVBC[8](A, V.StrictChunker(8)))
    assert Mg.info(trans=trans, compute=L.VBC_I64)["dtype"] == L.VBC_I64
    case = VecCase(Mg, trans, np.int32, 1, np.int32, 2, 3, -2, seed=6)

    def exact(k, win):
        want = (3 * expected(A, case.x(k), trans, np.int64) - 2 * case.y0(k).astype(np.int64)).astype(np.int32)
        assert np.array_equal(win, want), k

    replayed(case, Mg.handle(0, trans, compute=L.VBC_I64), Me.handle(0, trans, compute=L.VBC_I64), extra=exact)


@pytest.mark.parametrize("trans", [True, False], ids=["Btx", "Bx"])
def test_reference_quirks(monkeypatch, trans):
    """VBC_MUL_REFERENCE_QUIRKS (forward drops alpha, transposed overwrites y) is applied when the call is captured:
    every replay equals the eager quirk product and the plain product with the (alpha, beta) the quirks leave."""
    knobs(monkeypatch, {})
    Mg, Me = two(vbr)
    case = VecCase(Mg, trans, np.float64, 1, np.float64, 1, 0.5, -1.25, flags=L.VBC_MUL_REFERENCE_QUIRKS, seed=8)
    hg, he = Mg.handle(0, trans), Me.handle(0, trans)
    replayed(case, hg, he)
    replayed(case, hg, he, eager=lambda y, stream: case.call(he, y, stream, flags=0, alpha=1.0,
                                                             beta=0.0 if trans else -1.25))


# ---------------------------------------------------------------------------------------------------------------
# capture before the first use
# ---------------------------------------------------------------------------------------------------------------

def oracle_columns(M, case, k):
    """alpha op(M) X + beta Y0 of replay k's operands through the float64 oracle, column by column."""
    R = O.Ref1DVBC(M.m, M.n, M.W, M.Phi.spl, M.pos, M.idx, M.ofs, np.asarray(M.val, np.float64))
    X, Y0 = case.x(k).astype(np.float64), case.y0(k).astype(np.float64)
    vec = X.ndim == 1
    if vec:
        X, Y0 = X[:, None], Y0[:, None]
    cols = [O.mul(R, np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y0[:, j]), case.alpha, case.beta,
                  trans=bool(case.trans), ref_semantics=False) for j in range(X.shape[1])]
    return cols[0] if vec else np.stack(cols, axis=1)


def first_use_in_capture(M, h, case):
    """The first call of a path on a fresh handle, inside a capture: refused before any allocation, the capture
    stays valid; then the same call eagerly (exact against the oracle), captured again and replayed."""
    s = torch.cuda.Stream()
    marker = torch.zeros(4, device=DEV)
    y = dev(case.y_start(0))
    before = bits(y).copy()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        marker.fill_(1)
        with pytest.raises(L.ArgumentError, match="run the product once outside the capture"):
            case.call(h, y, torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    assert (marker == 1).all(), "the capture did not survive the refused call"
    assert np.array_equal(bits(y), before), "the refused call left work in the graph"
    # the same call eagerly: the warm-up the message asks for
    with torch.cuda.stream(s):
        case.call(h, y, s.cuda_stream)
    torch.cuda.synchronize()
    eager = y.clone()
    got = case.window(eager.cpu().numpy())
    assert np.array_equal(got.astype(np.float64), oracle_columns(M, case, 0)), "eager product differs from the oracle"
    # and captured again
    y.copy_(dev(case.y_start(0)))
    torch.cuda.synchronize()
    g2 = capture(case, h, y, s)
    g2.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(y), bits(eager))


def fresh_integer_matrix(dt=np.float64):
    M = with_integer_values(vbr(dt), dt)
    _LIVE.append(M)
    return M


def test_first_use_in_capture_mul_ex_staged(monkeypatch):
    """vbc_mul_ex on strided device operands: d_stage[0] and d_stage[1] do not exist yet."""
    knobs(monkeypatch, {})
    M = fresh_integer_matrix()
    h = M.handle(0, True)
    first_use_in_capture(M, h, VecCase(M, True, np.float64, 3, np.float64, 2, -1.0, 2.0, seed=9, draw=small_integers))


def test_first_use_in_capture_rowmajor_per_column(monkeypatch):
    """vbc_mul_mat on the row-major per-column path: the column temporaries d_stage[2 / 3] do not exist yet."""
    knobs(monkeypatch, {"VBC_SWEEP": "1"})
    M = fresh_integer_matrix()
    inf = M.info(trans=True)
    assert inf["sweep_bins"] > 0 and not inf["planar_mask"] & (1 << 22), inf
    first_use_in_capture(M, M.handle(0, True), MatCase(M, True, 3, True, np.float64, -1.0, 2.0, pad=2, seed=10,
                                                         draw=small_integers))


@pytest.mark.parametrize("nrhs", [16, 70])
def test_first_use_in_capture_fused_merge(monkeypatch, nrhs):
    """vbc_mul_mat on the fused merge kernel: d_carry_mm does not exist yet."""
    knobs(monkeypatch, MERGE)
    M = fresh_integer_matrix()
    first_use_in_capture(M, merge_fixed(M), MatCase(M, True, nrhs, True, np.float64, -1.0, 2.0, seed=11,
                                                    draw=small_integers))
