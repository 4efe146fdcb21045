"""Stream order of products that share a buffer of their handle, asserted rather than hoped for.

A handle carries mutable device state between products: the staging buffers d_stage[0..3] (host-pointer calls, the
device path of vbc_mul_ex for strided or converted operands, the row-major per-column path of vbc_mul_mat, host
values of vbc_update_values), the merge layout's carry slots and the carry buffer of the fused multi-RHS kernel.
ProductOrder (csrc/vbc_device.hip) chains the products that use them by an event, whatever streams they are on.

Every test follows one protocol (run_pair):

  1. both calls run alone, one after the other, each synchronised: the reference bits, and the first use of every
     buffer the calls need (nothing is allocated later);
  2. stream A gets a blocker, torch.cuda._sleep(BLOCKER_CYCLES), then the first call, then the event evA;
  3. the same host thread issues the second call on stream B.  Both streams are torch.cuda.Stream(): non-blocking,
     the null stream orders nothing between them;
  4. sB.synchronize() (a host-pointer call has synchronised already), then evA.query().

Calls that share a buffer must be chained: B waited for A, so evA.query() is True.  Calls that share nothing must not
be: the two controls (the contiguous device vbc_mul on a slotted-only handle, which vbc.h calls lock-free, and the
matrix-core panels) demand evA.query() False -- which also proves, for the whole file, that the blocker outlasts a
product, so a True elsewhere is the event chain's doing.  Finally everything is synchronised and every output of both
calls is compared bit for bit with step 1.  x and y differ between the two calls, so a staging buffer that the other
call overwrote shows in the bits.

The chain is acyclic (B waits on A, A on nothing of B): no case can deadlock.  There are no loops and no repeats.

BLOCKER_CYCLES: _sleep spins on the device's clock64() counter, which an MI355X advances at about 2.4 GHz (10^8 cycles
timed with events: 41.6 ms), so 3.6 * 10^8 cycles are about 150 ms, against products of tens of microseconds at these
shapes (3000 x 2446 and 3000 x 1050, 9000 blocks)."""
import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
BLOCKER_CYCLES = 360_000_000
Y_GAP = -7.0  # elements of a strided y between the strides
TOL = 1e-12   # test_gpu_parity.py TOL64 (every handle here is Float64)

SLOTTED = {"VBC_SLOTS": "1"}
SWEPT = {"VBC_SWEEP": "1"}
MERGE = {"VBC_SLOTS": "0", "VBC_SWEEP": "0"}
KNOBS = ("VBC_SLOTS", "VBC_SWEEP", "VBC_FWD_T", "VBC_MM_SLOTS", "VBC_FORK", "VBC_SMALL_FUSE", "VBC_PANEL_TILES")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pattern(kind):
    """3000 x 2446 with stripes 1..6 wide (the matrix of test_gpu_graph.py); "narrow": stripes 1 and 2 wide, which
    VBC_SLOTS=1 keeps in slotted buckets alone (test_gpu_mm_slots.py "vbr12")."""
    widths = np.arange(700) % 2 + 1 if kind == "narrow" else np.arange(700) % 6 + 1
    return V.synthetic.vbr_1dvbc(3000, 700, 9000, widths, W=8, seed=3)


_LIVE = []


@pytest.fixture(autouse=True)
def release_handles():
    yield
    for M in _LIVE:
        M.release()
    _LIVE.clear()


def matrix(monkeypatch, kind, knobs, updatable=False):
    """A matrix object of its own (the knobs are read when a handle is created)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    M = pattern(kind)
    if updatable:
        M.updatable = True
    _LIVE.append(M)
    return M


def slotted_only(M):
    inf = M.info(trans=True)
    assert inf["slot_bins"] > 0 and inf["bins_t"] == 0 and inf["planar_bins"] == 0 and inf["sweep_bins"] == 0, inf
    assert inf["bins_m"] == 0, inf
    return M.handle(0, True)


def swept(M):
    """A row-swept bucket: row-major B'X is not fused (planar_mask bit 22 clear) and runs one SpMV per column."""
    inf = M.info(trans=True)
    assert inf["sweep_bins"] > 0 and inf["bins_m"] == 0 and not inf["planar_mask"] & (1 << 22), inf
    return M.handle(0, True)


def merge_only(M):
    """Merge bins of compile-time widths alone: carry slots (has_scratch), row-major B'X fused (spmm_ranges)."""
    assert np.diff(M.Phi.spl).max() <= 8
    inf = M.info(trans=True)
    assert inf["bins_t"] > 0 and inf["slot_bins"] == 0 and inf["sweep_bins"] == 0 and inf["planar_bins"] == 0, inf
    assert inf["bins_m"] == 0, inf
    return M.handle(0, True)


def panels(M):
    inf = M.info(trans=True, multi=True)
    assert inf["bins_m"] > 0 and inf["bins_t"] == 0 and inf["slot_bins"] == 0 and inf["sweep_bins"] == 0, inf
    return M.handle(0, True, multi=True)


def bits(a):
    """The raw bits of a tensor or array, on the host."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32).copy()


class Op:
    """One call of the C ABI with operands of its own.  issue(stream) makes the call on the hipStream_t `stream`;
    outs() are the buffers it writes, whole (the gaps of a strided y included); reset() puts them back to their
    start; finish() is what must run after the call has completed before outs() is complete (vbc_update_values: a
    product that shows the stored values); oracle() checks outs() against the oracle."""

    def __init__(self, issue, outs, reset, oracle, finish=None):
        self.issue, self.outs, self.reset, self.oracle, self.finish = issue, outs, reset, oracle, finish


def reference(M, x, y0, alpha, beta):
    R = O.Ref1DVBC(M.m, M.n, M.W, M.Phi.spl, M.pos, M.idx, M.ofs, np.asarray(M.val, np.float64))
    return O.mul(R, np.asarray(x, np.float64), np.asarray(y0, np.float64).copy(), alpha, beta, trans=True,
                 ref_semantics=False)


def close(got, ref):
    return np.linalg.norm(np.asarray(got, np.float64) - ref) <= TOL * np.linalg.norm(ref)


def op_mul(M, h, seed, mem, alpha=0.5, beta=-1.25):
    """vbc_mul, B'x on contiguous operands: device tensors or host arrays."""
    rng = np.random.default_rng(seed)
    xh, y0h = rng.uniform(-1, 1, M.m), rng.uniform(-1, 1, M.n)
    if mem == L.VBC_MEM_DEVICE:
        x, y0, y = dev(xh), dev(y0h), dev(y0h)
        reset = lambda: y.copy_(y0)
    else:
        x, y = xh.copy(), y0h.copy()
        reset = lambda: np.copyto(y, y0h)

    def issue(stream):
        L.check(L.lib().vbc_mul(h, 1, L.ptr(x), M.m, L.ptr(y), M.n, alpha, beta, mem, stream, 0), "vbc_mul")

    def oracle():
        assert close(y.cpu().numpy() if mem == L.VBC_MEM_DEVICE else y, reference(M, xh, y0h, alpha, beta))

    return Op(issue, lambda: [y], reset, oracle)


def op_mul_ex(M, h, seed, xdt=np.float64, incx=3, incy=1, alpha=-0.75, beta=0.5):
    """vbc_mul_ex, B'x on device operands that go through d_stage[0] (x strided by incx and / or of another eltype)
    and, for incy != 1, d_stage[1] (y gathered, since beta != 0, and scattered)."""
    rng = np.random.default_rng(seed)
    xh = rng.uniform(-1, 1, M.m).astype(xdt)
    y0h = rng.uniform(-1, 1, M.n)
    xbuf = torch.full((abs(incx) * M.m,), float("nan"), dtype=getattr(torch, np.dtype(xdt).name), device=DEV)
    xbuf[::incx].copy_(dev(xh))
    ystart = np.full(abs(incy) * M.n, Y_GAP)
    if incy > 0:
        ystart[::incy] = y0h
        first = 0
    else:  # a reversed view: y[1] is the last element of the buffer
        ystart[::-1][::-incy] = y0h
        first = len(ystart) - 1
    y0buf, ybuf = dev(ystart), dev(ystart)
    assert xdt != np.float64 or incx != 1  # (staged: not the contiguous fast path)

    def issue(stream):
        L.check(L.lib().vbc_mul_ex(h, 1, xbuf.data_ptr(), L.dtype_code(np.dtype(xdt)), incx, M.m, ybuf.data_ptr() + 8 * first,
                                   L.VBC_F64, incy, M.n, alpha, beta, L.VBC_MEM_DEVICE, stream, 0), "vbc_mul_ex")

    def oracle():
        got = ybuf.cpu().numpy()
        win = got[::incy] if incy > 0 else got[::-1][::-incy]
        assert close(win, reference(M, xh, y0h, alpha, beta))
        gap = np.ones(len(got), bool)
        (gap if incy > 0 else gap[::-1])[::abs(incy)] = False
        assert (got[gap] == Y_GAP).all()

    return Op(issue, lambda: [ybuf], lambda: ybuf.copy_(y0buf), oracle)


def op_mul_mat(M, h, seed, nrhs, rowmajor, mem=L.VBC_MEM_DEVICE, alpha=1.5, beta=-0.5):
    """vbc_mul_mat, B'X on packed operands (row-major nx x nrhs, or column-major nrhs columns of nx)."""
    rng = np.random.default_rng(seed)
    Xh, Y0h = rng.uniform(-1, 1, (M.m, nrhs)), rng.uniform(-1, 1, (M.n, nrhs))
    lay = lambda a: np.array(a if rowmajor else a.T, order="C")  # (a copy of its own)
    ldx, ldy = (nrhs, nrhs) if rowmajor else (M.m, M.n)
    if mem == L.VBC_MEM_DEVICE:
        X, Y0, Y = dev(lay(Xh)), dev(lay(Y0h)), dev(lay(Y0h))
        reset = lambda: Y.copy_(Y0)
    else:
        X, Y = lay(Xh), lay(Y0h)
        reset = lambda: np.copyto(Y, lay(Y0h))
    flags = L.VBC_MAT_ROWMAJOR if rowmajor else 0

    def issue(stream):
        L.check(L.lib().vbc_mul_mat(h, 1, nrhs, L.ptr(X), ldx, M.m, L.ptr(Y), ldy, M.n, alpha, beta, mem, stream,
                                    flags), "vbc_mul_mat")

    def oracle():
        got = Y.cpu().numpy() if mem == L.VBC_MEM_DEVICE else Y
        got = got if rowmajor else got.T
        for j in range(nrhs):
            assert close(got[:, j], reference(M, Xh[:, j], Y0h[:, j], alpha, beta)), j

    return Op(issue, lambda: [Y], reset, oracle)


def op_update(M, h, seed):
    """vbc_update_values with host values (through d_stage[0]); finish(): a contiguous product on the new values."""
    rng = np.random.default_rng(seed)
    old = np.array(M.val)
    new = old * rng.uniform(0.5, 2.0, len(old))
    xh = rng.uniform(-1, 1, M.m)
    x, y = dev(xh), torch.full((M.n,), float("nan"), dtype=torch.float64, device=DEV)

    def update(val, stream):
        L.check(L.lib().vbc_update_values(h, val.ctypes.data, len(val), L.VBC_F64, L.VBC_MEM_HOST, stream),
                "vbc_update_values")

    def finish():
        L.check(L.lib().vbc_mul(h, 1, x.data_ptr(), M.m, y.data_ptr(), M.n, 1.0, 0.0, L.VBC_MEM_DEVICE,
                                torch.cuda.current_stream().cuda_stream, 0), "vbc_mul")

    def reset():
        update(old, None)
        y.fill_(float("nan"))

    def oracle():
        R = O.Ref1DVBC(M.m, M.n, M.W, M.Phi.spl, M.pos, M.idx, M.ofs, new)
        assert close(y.cpu().numpy(), O.mul(R, xh, np.zeros(M.n), trans=True))

    return Op(lambda stream: update(new, stream), lambda: [y], reset, oracle, finish)


def run_pair(a, b, must_wait, why):
    """The protocol of the module docstring: `a` behind the blocker on stream A, then `b` on stream B."""
    ops = (a, b)
    for op in ops:  # alone, one after the other
        op.issue(None)
        torch.cuda.synchronize()
    for op in ops:
        if op.finish:
            op.finish()
    torch.cuda.synchronize()
    alone = [bits(o) for op in ops for o in op.outs()]
    for op in ops:
        op.oracle()
    for op in ops:
        op.reset()
    torch.cuda.synchronize()
    for o, r in zip([o for op in ops for o in op.outs()], alone):
        assert not np.array_equal(bits(o), r)  # (the start state differs from the result: the comparison below means something)

    sA, sB = torch.cuda.Stream(), torch.cuda.Stream()
    evA = torch.cuda.Event()
    with torch.cuda.stream(sA):
        torch.cuda._sleep(BLOCKER_CYCLES)
    a.issue(sA.cuda_stream)
    evA.record(sA)
    b.issue(sB.cuda_stream)
    sB.synchronize()
    a_done = evA.query()
    torch.cuda.synchronize()
    for op in ops:
        if op.finish:
            op.finish()
    torch.cuda.synchronize()
    print(why, "evA.query() after sB.synchronize():", a_done)
    if must_wait:
        assert a_done, f"the second call did not wait for the first ({why})"
    else:
        assert not a_done, (f"the first call had finished when the second returned ({why}): either the second waited "
                            "for it, or the blocker was too short for this file's assertions to mean anything")
    for o, r in zip([o for op in ops for o in op.outs()], alone):
        assert np.array_equal(bits(o), r), why


def pair(a, b, swap):
    return (b, a) if swap else (a, b)


SWAP = pytest.mark.parametrize("swap", [False, True], ids=["AB", "BA"])


def test_mul_ex_strided_then_host_mul(monkeypatch):
    M = matrix(monkeypatch, "narrow", SLOTTED)
    h = slotted_only(M)
    run_pair(op_mul_ex(M, h, 1, incx=3), op_mul(M, h, 2, L.VBC_MEM_HOST), True,
             "vbc_mul_ex gathers x into d_stage[0]; host vbc_mul copies its x there")


def test_mul_ex_converted_reversed_then_host_mul_mat(monkeypatch):
    M = matrix(monkeypatch, "narrow", SLOTTED)
    h = slotted_only(M)
    run_pair(op_mul_ex(M, h, 3, xdt=np.float32, incx=1, incy=-1), op_mul_mat(M, h, 4, 3, False, L.VBC_MEM_HOST), True,
             "vbc_mul_ex converts x into d_stage[0] and gathers y into d_stage[1]; column-major host vbc_mul_mat "
             "copies X and Y there")


def test_mul_ex_strided_then_host_mul_mat_rowmajor(monkeypatch):
    M = matrix(monkeypatch, "narrow", SLOTTED)
    h = slotted_only(M)
    run_pair(op_mul_ex(M, h, 5, incx=3, incy=2), op_mul_mat(M, h, 6, 3, True, L.VBC_MEM_HOST), True,
             "vbc_mul_ex stages x and y in d_stage[0 / 1]; row-major host vbc_mul_mat copies X and Y there")


@SWAP
def test_two_staged_mul_ex(monkeypatch, swap):
    M = matrix(monkeypatch, "narrow", SLOTTED)
    h = slotted_only(M)
    a, b = pair(op_mul_ex(M, h, 7, incx=3), op_mul_ex(M, h, 8, xdt=np.float32, incx=2, incy=-1), swap)
    run_pair(a, b, True, "two vbc_mul_ex on strided device operands share d_stage[0 / 1]")


def test_mul_ex_strided_then_host_update(monkeypatch):
    M = matrix(monkeypatch, "narrow", SLOTTED, updatable=True)
    h = slotted_only(M)
    run_pair(op_mul_ex(M, h, 9, incx=3), op_update(M, h, 10), True,
             "vbc_mul_ex gathers x into d_stage[0]; vbc_update_values copies host values there")


@SWAP
def test_two_rowmajor_per_column_products(monkeypatch, swap):
    M = matrix(monkeypatch, "wide", SWEPT)
    h = swept(M)
    a, b = pair(op_mul_mat(M, h, 11, 3, True), op_mul_mat(M, h, 12, 5, True), swap)
    run_pair(a, b, True, "row-major per-column vbc_mul_mat products share the column temporaries d_stage[2 / 3]")


@SWAP
def test_two_merge_products(monkeypatch, swap):
    M = matrix(monkeypatch, "wide", MERGE)
    h = merge_only(M)
    a, b = pair(op_mul(M, h, 13, L.VBC_MEM_DEVICE), op_mul(M, h, 14, L.VBC_MEM_DEVICE, alpha=1.0, beta=0.0), swap)
    run_pair(a, b, True, "merge-layout products share the carry slots (has_scratch)")


@SWAP
def test_two_fused_merge_multi_rhs_products(monkeypatch, swap):
    M = matrix(monkeypatch, "wide", MERGE)
    h = merge_only(M)
    a, b = pair(op_mul_mat(M, h, 15, 16, True), op_mul_mat(M, h, 16, 70, True), swap)
    run_pair(a, b, True, "fused row-major B'X products (spmm_ranges, NR = 16 and 64) share d_carry_mm")


def test_control_contiguous_device_products_do_not_wait(monkeypatch):
    """The control of this file: the lock-free path.  Nothing is shared, so B must not wait for A -- and A, behind
    the blocker, must still be running when B has finished."""
    M = matrix(monkeypatch, "narrow", SLOTTED)
    h = slotted_only(M)
    run_pair(op_mul(M, h, 17, L.VBC_MEM_DEVICE), op_mul(M, h, 18, L.VBC_MEM_DEVICE), False,
             "contiguous device vbc_mul on a slotted-only handle shares nothing")


@pytest.mark.parametrize("rowmajor", [True, False], ids=["rowmajor", "colmajor"])
def test_control_panel_products_do_not_wait(monkeypatch, rowmajor):
    """The matrix-core panels hold no shared scratch: two panel products on two streams are not chained."""
    M = matrix(monkeypatch, "wide", {})
    h = panels(M)
    run_pair(op_mul_mat(M, h, 19, 5, rowmajor), op_mul_mat(M, h, 20, 17, rowmajor), False,
             "vbc_mul_mat on the panels of a VBC_CREATE_MULTI handle shares nothing")
