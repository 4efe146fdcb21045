"""Value updates of sharded matrices, the parts that need no GPU: the value plan of the C sharded handle
(vbc_host.h vbcx_sharded_value_plan, the function vbc*_create_sharded builds its shards with), the value index
of the torch.distributed class, its update over gloo with the oracle as each rank's product, and the ABI."""
import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from sparsematrixvbcs_amd import _lib as L
from sparsematrixvbcs_amd import distributed as D

ROOT = Path(__file__).resolve().parent.parent


def mat1d():
    rng = np.random.default_rng(11)  # the matrix of tests/test_gpu_multigpu.py
    return V.synthetic.vbr_1dvbc(9000, 2500, 60000, rng.integers(1, 9, 2500), W=8, seed=12)


def mat2d(seed=3):
    A = sp.random(700, 520, density=0.02, random_state=seed, format="csc", dtype=np.float64)
    A.data = np.random.default_rng(seed).uniform(-1, 1, A.nnz)
    return V.SparseMatrixVBC[4, 4](A, V.AlternatingPacker(V.OverlapChunker(0.9, 4), V.OverlapChunker(0.9, 4)))


def value_plan(B, ngpus, split):
    """(cuts, vbase, run_begin, runs[nruns, 3]) of vbcx_sharded_value_plan."""
    is2d = hasattr(B, "Pi")
    cuts, vbase, rbeg = (np.zeros(ngpus + 1, np.int64) for _ in range(3))
    nruns = C.c_int64(-1)
    kind = L.VBC_SPLIT_STRIPES if split == "stripes" else L.VBC_SPLIT_ROWS
    def call(runs):
        L.check(L.lib().vbcx_sharded_value_plan(
            B.m, B.n, len(B.Pi) if is2d else 0, B.Pi.spl.ctypes.data if is2d else None, len(B.Phi),
            B.Phi.spl.ctypes.data, B.pos.ctypes.data, B.idx.ctypes.data, B.ofs.ctypes.data, B.val.dtype.itemsize,
            ngpus, kind, cuts.ctypes.data, vbase.ctypes.data, rbeg.ctypes.data, C.byref(nruns),
            None if runs is None else runs.ctypes.data, 0 if runs is None else len(runs)), "value plan")
    call(None)  # the count, then the table
    runs = np.full((nruns.value, 3), -1, np.int64)
    call(runs)
    return cuts, vbase, rbeg, runs


def expand(runs):
    """Source element of every destination element of the runs, in dst order."""
    if len(runs) == 0:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(s, s + n) for s, _, n in runs])


@pytest.mark.parametrize("split", ["stripes", "rows"])
@pytest.mark.parametrize("ngpus", [1, 3, 7])
def test_value_plan_1d(split, ngpus):
    B = mat1d()
    nval = int(B.ofs[-1]) - 1
    cuts, vbase, rbeg, runs = value_plan(B, ngpus, split)
    assert vbase[0] == 0 and vbase[-1] == nval and np.all(np.diff(vbase) >= 0)
    if split == "stripes":
        sc = D.stripe_split(B, ngpus)
        assert np.array_equal(cuts, B.Phi.spl[sc] - 1)
        assert len(runs) == 0 and np.all(rbeg == 0)
        for g in range(ngpus):
            S, _ = D.shard(B, int(sc[g]), int(sc[g + 1]))
            nv = int(S.ofs[-1]) - 1
            assert nv == vbase[g + 1] - vbase[g]
            assert np.array_equal(B.val[vbase[g]:vbase[g + 1]], S.val[:nv])
        return
    rc = D.row_split(B, ngpus)
    assert np.array_equal(cuts, rc)
    assert rbeg[0] == 0 and rbeg[-1] == len(runs)
    # ascending in dst, covering [0, nval) exactly once over all shards
    assert np.array_equal(runs[:, 1], np.concatenate([[0], np.cumsum(runs[:, 2])[:-1]]))
    assert runs[:, 2].sum() == nval and np.all(runs[:, 2] >= 1)
    assert np.array_equal(np.sort(expand(runs)), np.arange(nval))
    for g in range(ngpus):
        S = D.row_shard(B, int(rc[g]), int(rc[g + 1]))
        nv = int(S.ofs[-1]) - 1
        mine = runs[rbeg[g]:rbeg[g + 1]]
        assert nv == vbase[g + 1] - vbase[g]
        assert len(mine) == 0 or (mine[0, 1] == vbase[g] and mine[-1, 1] + mine[-1, 2] == vbase[g + 1])
        assert np.array_equal(B.val[expand(mine)], S.val[:nv])
        # adjacent kept blocks are one run: no run continues where the previous one of its shard stopped
        assert not np.any(mine[:-1, 0] + mine[:-1, 2] == mine[1:, 0])
    if ngpus == 1:
        assert len(runs) == 1 and tuple(runs[0]) == (0, 0, nval)


@pytest.mark.parametrize("split", ["stripes", "rows"])
@pytest.mark.parametrize("ngpus", [1, 3, 7])
def test_value_plan_2d(split, ngpus):
    """The 2D format: a run is whole u x w blocks; each shard's values are those of the blocks whose block row
    (row split) or stripe (stripe split) falls in its range, in stored order."""
    B = mat2d()
    nval = int(B.ofs[-1]) - 1
    cuts, vbase, rbeg, runs = value_plan(B, ngpus, split)
    assert vbase[0] == 0 and vbase[-1] == nval
    # every block's value range from the fields themselves
    w = np.repeat(np.diff(B.Phi.spl), np.diff(B.pos))
    u = np.diff(B.Pi.spl)[B.idx - 1]
    bsz = u * w
    bstart = np.concatenate([[0], np.cumsum(bsz)[:-1]])
    assert bsz.sum() == nval
    rows_lo = B.Pi.spl[B.idx - 1] - 1  # first row of each block
    if split == "stripes":
        assert len(runs) == 0
        assert set(cuts.tolist()) <= set((B.Phi.spl - 1).tolist())
        ofs0 = B.ofs - 1
        assert set(vbase.tolist()) <= set(ofs0.tolist())
        stripe_of = np.searchsorted(B.Phi.spl - 1, cuts, side="left")
        assert np.array_equal(vbase, ofs0[stripe_of])
        return
    assert set(cuts.tolist()) <= set((B.Pi.spl - 1).tolist())
    assert np.array_equal(runs[:, 1], np.concatenate([[0], np.cumsum(runs[:, 2])[:-1]]))
    assert np.array_equal(np.sort(expand(runs)), np.arange(nval))
    for g in range(ngpus):
        keep = (rows_lo >= cuts[g]) & (rows_lo < cuts[g + 1])
        want = np.concatenate([np.arange(s, s + n) for s, n in zip(bstart[keep], bsz[keep])] or [np.zeros(0, np.int64)])
        mine = runs[rbeg[g]:rbeg[g + 1]]
        assert np.array_equal(expand(mine), want)
        assert not np.any(mine[:-1, 0] + mine[:-1, 2] == mine[1:, 0])
        # run boundaries are block boundaries
        assert set(mine[:, 0].tolist()) <= set(bstart.tolist())


def dist_matrix(kind):
    if kind == "mesh":  # shards rebased to their rows (stripe split) / trimmed to their stripes (row split)
        return V.SparseMatrix1DVBC[8](V.synthetic.fe_stiffness_3d(3000, 60000), V.StrictChunker(8))
    return V.synthetic.vbr_1dvbc(500, 60, 700, np.arange(60) % 5 + 1, W=8, seed=7)


@pytest.mark.parametrize("split", ["stripes", "rows"])
@pytest.mark.parametrize("kind", ["random", "mesh"])
def test_val_index_world3(split, kind):
    B = dist_matrix(kind)
    seen = []
    for rank in range(3):
        S = D.ShardedSparseMatrix1DVBC(B, rank, 3, local_mul=lambda *a: None, split=split, updatable=True)
        assert S.updatable and S.local.updatable
        nv = int(S.local.ofs[-1]) - 1
        assert isinstance(S.val_index, slice) == (split == "stripes")
        assert np.array_equal(B.val[S.val_index], S.local.val[:nv])
        seen.append(np.arange(len(B.val))[S.val_index])
        v2 = np.arange(len(B.val), dtype=np.float64) + 0.5
        S.update_values(v2)
        assert np.array_equal(S.local.val[:nv], v2[S.val_index]) and np.all(S.local.val[nv:] == 0)
        if nv:
            with pytest.raises(L.DimensionMismatch):
                S.update_values(v2[:int(seen[-1].max())])  # one short of the last element this rank reads
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(int(B.ofs[-1]) - 1))
    with pytest.raises(L.ArgumentError):
        D.ShardedSparseMatrix1DVBC(B, 0, 3, local_mul=lambda *a: None, split=split).update_values(B.val)


def oracle_mul(y, op, x, alpha, beta):
    trans = isinstance(op, V.Adjoint)
    B = op.parent if trans else op
    R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, B.val)
    O.mul(R, np.ascontiguousarray(x.numpy()), y.numpy(), alpha, beta, trans=trans, ref_semantics=False)
    return y


def _two_values(B):
    rng = np.random.default_rng(1)
    n = len(B.val)
    v1 = (rng.integers(1, 9, n) * rng.choice([-1, 1], n)).astype(np.float64)
    v2 = (rng.integers(1, 9, n) * rng.choice([-1, 1], n)).astype(np.float64)
    z = rng.permutation(n)
    v1[z[: n // 10]] = 0
    v2[z[n // 10: 2 * (n // 10)]] = 0
    return v1, v2


def _with_values(B, v):
    return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, v.copy())


def _worker(rank, world, port, q, split):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        B = dist_matrix("mesh")
        v1, v2 = _two_values(B)
        Su = D.ShardedSparseMatrix1DVBC(_with_values(B, v1), rank, world, local_mul=oracle_mul, split=split,
                                        updatable=True)
        Sf = D.ShardedSparseMatrix1DVBC(_with_values(B, v2), rank, world, local_mul=oracle_mul, split=split)
        rng = np.random.default_rng(3)
        xt, xf = torch.from_numpy(rng.uniform(-1, 1, B.m)), torch.from_numpy(rng.uniform(-1, 1, B.n))
        y0t, y0f = torch.from_numpy(rng.uniform(-1, 1, B.n)), torch.from_numpy(rng.uniform(-1, 1, B.m))
        out = []
        for S in (Su, Sf):
            if S is Su:
                before = S.mul_t(y0t.clone(), xt, 1.5, 0.25).numpy().copy()
                S.update_values(v2)
            out.append((S.mul_t(y0t.clone(), xt, 1.5, 0.25).numpy().copy(), S.mul(y0f.clone(), xf, 2.0, 0.5).numpy().copy()))
        q.put((rank, before, out[0][0], out[0][1], out[1][0], out[1][1]))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("split", ["stripes", "rows"])
def test_update_world2_gloo(split):
    """World 2 over gloo, the oracle as each rank's product (no handle alive): after update_values(v2) both
    products equal those of a fresh object built from v2 bit for bit, and differ from the v1 product."""
    from tests.test_distributed import free_port
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, split)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert len(r) == 6, r
        _, before, ut, uf, ft, ff = r
        assert np.array_equal(ut, ft) and np.array_equal(uf, ff)
        assert not np.array_equal(before, ut)


def test_abi_declares_and_exports():
    lib = L.lib()
    vbc_h = (ROOT / "include" / "vbc.h").read_text()
    host_h = (ROOT / "include" / "vbc_host.h").read_text()
    assert re.search(r"VBC_API\s+int\s+vbc_sharded_update_values\s*\(", vbc_h)
    assert re.search(r"VBC_API\s+int\s+vbcx_sharded_value_plan\s*\(", host_h)
    assert re.search(r"#define\s+VBC_CREATE_UPDATABLE_SHARDS\s+0x40u", vbc_h)
    for name in ("vbc_sharded_update_values", "vbcx_sharded_value_plan"):
        assert name in L.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.vbc_version() == 30400
    assert int(re.search(r"#define\s+VBC_VERSION\s+(\d+)", vbc_h).group(1)) == 30400
    assert L.VBC_CREATE_UPDATABLE_SHARDS == 0x40
