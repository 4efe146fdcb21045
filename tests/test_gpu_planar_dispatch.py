"""Every planar bin reaches its own kernel: the case lists of csrc/vbc_planar_launch.inc, family by family and type by
type (f64, f32, and f64n: fp64 compute on Float32 stored values), at shapes of a few chunks of 64 stripes.

Each case forces its layout with the knobs of INTEGRATION.md, checks through vbc_info that it got the layout it means
to test, and runs (alpha, beta) = (1, 0) -- the affine write paths, staged or direct -- and (0.5, 2), the path that
reads y.  Assertions are those of the family's own test (test_gpu_planar.py, test_gpu_lanes.py, test_gpu_narrow_*.py):
fp64 with one wave per chunk equals the oracle bit for bit at (1, 0) and within TOL64 at (0.5, 2); fp32, the forward
row runs and the split products (P partial sums per chunk) within TOL32 / TOL64; a narrow handle equals the handle
created with `B.narrow = True` alone bit for bit.

NOT_BUILT and MULTI_MODES_NOT_BUILT name every case the planner does not build, with the reason; any other case that
comes out in another layout fails.  The matrices are a few chunks each: on an MI355X every parametrised case takes
under half a second (the largest, test_chunk_widths_runs_paths[f64] with its 108 handles, 0.3 s)."""
import numpy as np
import pytest

import sparsematrixvbcs_amd as V
from oracle import oracle as O
from tests.test_gpu_narrow_planar import bitwise, clone, info64, product
from tests.test_gpu_parity import TOL32, TOL64, rel
from tests.test_gpu_planar import expand_runs, sp_blocked

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

AB = ((1.0, 0.0), (0.5, 2.0))
WIDTHS, RUNS = (3, 4, 5, 6, 7, 8), (1, 2, 3)
FWD_WR = [(w, r) for w in (2, 3, 4) for r in (2, 3)]
# fp32 rows of 4 values are one 16-B lane vector: not planar (test_widths_random_x, test_split_chunks,
# test_widths_integer_data_bitwise exempt it)
NOT_BUILT = {(fam, "f32", 4, r) for fam in ("chunk", "lanes", "split") for r in RUNS}
# spmv_planar_split at w = 1, 2: a bucket of 1- or 2-wide stripes is planar only as a bin of the fused small-matrix
# split (vbc_plan_bins.hip slot_planar), and the library always runs such bins through spmv_split_multi: the conditions
# under which vbc_device.hip gives up the fused launch are compressed keys (split bins get them only under the tuning
# knob VBC_SPLIT_KC, which the product library does not read), VBC_DIAG (ablation build), and the masked, lane and pair
# forms, which a split bin never has.  test_fused_split_multi runs those widths through the fused launch.
NOT_BUILT |= {("split", typ, w, r) for typ in ("f64", "f32") for w in (1, 2) for r in RUNS}
# spmv_split_multi's slice loops 1 (pipelined) and 3 (batched non-temporal) come from the tuning knobs VBC_SPLIT_PIPE
# and VBC_SPLIT_NT_MB alone, which only the ablation build reads: the product library selects 0 or 2
MULTI_MODES_NOT_BUILT = {1: "VBC_SPLIT_PIPE (tuning knob)", 3: "VBC_SPLIT_NT_MB (tuning knob)"}

ALL_KNOBS = ("VBC_SLOTS", "VBC_SLOT_PLANAR", "VBC_SLOT_RUNS", "VBC_SLOT_KEYS16", "VBC_SLOT_STAGE", "VBC_PLANAR_SPLIT",
             "VBC_PLANAR_LANES", "VBC_LANES_PAIR", "VBC_PLANAR_PAIR", "VBC_PLANAR_MASK", "VBC_SLOTS_SORT", "VBC_SLOTS_PAD",
             "VBC_SMALL_FUSE")
CHUNK = {"VBC_SLOT_PLANAR": "1", "VBC_SMALL_FUSE": "0", "VBC_PLANAR_SPLIT": "0", "VBC_PLANAR_PAIR": "0",
         "VBC_PLANAR_LANES": "0", "VBC_SLOTS": "1"}
LANES = {"VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "0", "VBC_SLOTS": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0"}
SPLIT = {"VBC_SLOT_PLANAR": "1", "VBC_SMALL_FUSE": "0", "VBC_SLOTS": "1", "VBC_PLANAR_LANES": "0", "VBC_PLANAR_PAIR": "0"}
FWD = {"VBC_PLANAR_PAIR": "0", "VBC_PLANAR_LANES": "0", "VBC_PLANAR_SPLIT": "0"}
PAIR = {"VBC_PLANAR_PAIR": "2", "VBC_SLOTS": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0", "VBC_PLANAR_LANES": "0"}
PAIR_LANES = {"VBC_PLANAR_LANES": "1", "VBC_LANES_PAIR": "1", "VBC_PLANAR_SPLIT": "0", "VBC_SMALL_FUSE": "0"}
FWD_PAIR = {"VBC_PLANAR_PAIR": "2", "VBC_PLANAR_SPLIT": "0"}
# write paths of a chunk form, each in both key forms (VBC_SLOT_KEYS16 = 0: 32-bit keys, 2: int16 delta keys):
# (knobs, masked).  Natural order staged (the default) and direct (VBC_SLOT_STAGE=0); the masked chunk-local order
# (a y-offset table)
KEYS = ("0", "2")
BX_PATHS = [(dict(path, VBC_SLOT_KEYS16=k), masked) for k in KEYS for path, masked in
            (({}, False), ({"VBC_SLOT_STAGE": "0"}, False), ({"VBC_SLOTS_SORT": "2", "VBC_PLANAR_MASK": "1"}, True))]
FWD_PATHS = [(dict(path, VBC_SLOT_KEYS16=k), masked) for k in KEYS for path, masked in
             (({"VBC_PLANAR_MASK": "0", "VBC_SLOTS_PAD": "100"}, False),
              ({"VBC_PLANAR_MASK": "0", "VBC_SLOTS_PAD": "100", "VBC_SLOT_STAGE": "0"}, False),
              ({"VBC_PLANAR_MASK": "1"}, True))]
NARROW = {"chunk": ("planar", 14), "fwd": ("planar", 15), "lanes": ("streams", 18), "pair": ("pairs", 16),
          "pair_lanes": ("pairs", 16), "pair_dot": ("pairs", 17)}
DTYPE = {"f64": np.float64, "f32": np.float32, "f64n": np.float32}  # (f64n: a float32 matrix on a Float64 handle)


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


def runs_matrix(w, run, dtype, q=3000):
    """300 w-wide stripes (five chunks, the last one partial) over 2000 rows, every stored row widened to `run` rows."""
    base = V.synthetic.vbr_1dvbc(2000, 300, q, w, W=8, dtype=dtype, seed=10 * w + run)
    return expand_runs(base, run, seed=w + run) if run > 1 else base


def fwd_matrix(w, R, dtype):
    """Output rows in runs of R with identical lists of w-wide stripes (test_forward_row_runs' construction)."""
    rng = np.random.default_rng(100 * w + R)
    base = V.synthetic.vbr_1dvbc(1500, 400, 6000, w, W=8, dtype=dtype, seed=w + R)
    return V.SparseMatrix1DVBC[8](sp_blocked(base, R, rng, dtype), V.EquiChunker(w))


def products(B, typ, fam, trans, exact, seed):
    """The two products of one handle against the oracle (and, narrow, against the `narrow = True` handle)."""
    R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, B.val.astype(np.float64))
    xdt = np.float32 if typ == "f32" else np.float64
    rng = np.random.default_rng(seed)
    nx, ny = (B.m, B.n) if trans else (B.n, B.m)
    x, y0 = rng.uniform(-1, 1, nx).astype(xdt), rng.uniform(-1, 1, ny).astype(xdt)
    Bn = clone(B, True) if typ == "f64n" else None
    for alpha, beta in AB:
        got = product(B, trans, x, y0, alpha, beta)
        ref = O.mul(R, x.astype(np.float64), y0.astype(np.float64), alpha, beta, trans=trans, ref_semantics=False)
        if Bn is not None:
            assert bitwise(got, product(Bn, trans, x, y0, alpha, beta)), (fam, alpha, beta)
        if exact and typ != "f32" and beta == 0.0:
            assert np.array_equal(got, ref), (fam, alpha, beta)
        else:
            assert rel(got.astype(np.float64), ref) <= (TOL32 if typ == "f32" else TOL64), (fam, alpha, beta)
    if Bn is not None:
        Bn.release()


def handle(B0, typ, fam):
    """A fresh matrix object of the type's handle, and its vbc_info reader."""
    B = clone(B0, NARROW[fam][0] if typ == "f64n" else False)
    return B, (lambda trans: info64(B, trans) if typ == "f64n" else B.info(trans=trans))


class KeyForms:
    """vbc_info has no field for the key form, but int16 delta keys make the layout smaller: of two handles that differ
    in VBC_SLOT_KEYS16 alone, the one under 2 must report fewer bytes."""

    def __init__(self):
        self.bytes = {}

    def note(self, case, path, nbytes):
        rest = tuple(sorted((k, v) for k, v in path.items() if k != "VBC_SLOT_KEYS16"))
        self.bytes.setdefault((case, rest), {})[path["VBC_SLOT_KEYS16"]] = nbytes

    def check(self):
        assert self.bytes
        for case, b in self.bytes.items():
            assert b["2"] < b["0"], (case, b)


def narrow_bit(inf, typ, fam):
    return typ != "f64n" or bool(inf["planar_mask"] & (1 << NARROW[fam][1]))


@pytest.mark.parametrize("typ", ["f64", "f32", "f64n"])
def test_chunk_widths_runs_paths(knobs, typ):
    """spmv_planar<T, w, FASTE, NB, KC, run, MASK, S>: w 3..8 x runs 1..3, every write path."""
    missing, keys = set(), KeyForms()
    for w in WIDTHS:
        for run in RUNS:
            B0 = runs_matrix(w, run, DTYPE[typ])
            for path, masked in BX_PATHS:
                knobs(CHUNK, {"VBC_SLOT_RUNS": "1"}, path)
                B, info = handle(B0, typ, "chunk")
                inf = info(True)
                built = (inf["planar_bins"] == 1 and inf["planar_run"] == run and inf["planar_split"] == 1 and
                         inf["planar_pair"] == 0 and (inf["planar_mask"] & 1) == int(masked) and
                         not inf["planar_mask"] & 4 and narrow_bit(inf, typ, "chunk"))
                print("chunk", typ, w, run, path, {k: inf[k] for k in ("planar_bins", "planar_run", "planar_mask")})
                if not built:
                    missing.add(("chunk", typ, w, run))
                else:
                    keys.note((w, run), path, inf["bytes_t"])
                    products(B, typ, "chunk", True, exact=True, seed=w + run)
                B.release()
    keys.check()
    assert missing == {c for c in NOT_BUILT if c[0] == "chunk" and c[1] == typ}


@pytest.mark.parametrize("typ", ["f64", "f32", "f64n"])
def test_lane_streams_widths_runs(knobs, typ):
    """spmv_planar_lanes<T, w, run, DEEP, RD, 0, S>: w 3..8 x runs 1..3; RD with beta != 0, the plain form without."""
    missing = set()
    for w in WIDTHS:
        for run in RUNS:
            knobs(LANES)
            B, info = handle(runs_matrix(w, run, DTYPE[typ]), typ, "lanes")
            inf = info(True)
            built = (inf["planar_mask"] & 4 and inf["planar_run"] == run and inf["planar_pair"] == 0 and
                     narrow_bit(inf, typ, "lanes"))
            print("lanes", typ, w, run, {k: inf[k] for k in ("planar_bins", "planar_run", "planar_mask")})
            if not built:
                missing.add(("lanes", typ, w, run))
            else:
                products(B, typ, "lanes", True, exact=True, seed=w + run)
            B.release()
    assert missing == {c for c in NOT_BUILT if c[0] == "lanes" and c[1] == typ}


@pytest.mark.parametrize("typ", ["f64", "f32"])
def test_split_widths_runs_waves(knobs, typ):
    """spmv_planar_split<T, w, KC, run, P>: w 1..8 x runs 1..3 x P in {2, 4, 8} (no narrow form); w = 1, 2 are not
    built (NOT_BUILT has the reason)."""
    missing = set()
    for w in range(1, 9):
        for run in RUNS:
            B0 = runs_matrix(w, run, DTYPE[typ], q=9000)
            for P in (2, 4, 8):
                knobs(SPLIT, {"VBC_PLANAR_SPLIT": str(P), "VBC_SLOT_RUNS": "1"})
                B, info = handle(B0, typ, "split")
                inf = info(True)
                built = (inf["planar_bins"] == 1 and inf["planar_split"] == P and inf["planar_run"] == run and
                         not inf["planar_mask"] & 32)
                print("split", typ, w, run, P, {k: inf[k] for k in ("planar_bins", "planar_run", "planar_split", "planar_mask")})
                if not built:
                    missing.add(("split", typ, w, run))
                else:
                    products(B, typ, "split", True, exact=False, seed=w + run + P)
                B.release()
    assert missing == {c for c in NOT_BUILT if c[0] == "split" and c[1] == typ}


def uniform_rows(widths, per, m, dtype, seed):
    """Stripes of the given widths with exactly `per` stored rows each, over m rows."""
    rng = np.random.default_rng(seed)
    widths = np.asarray(widths, np.int64)
    idx = np.concatenate([np.sort(rng.choice(m, per, replace=False)) for _ in widths])
    rows = np.full(len(widths), per, np.int64)
    spl = np.concatenate([[1], 1 + np.cumsum(widths)]).astype(np.int64)
    pos = np.concatenate([[1], 1 + np.cumsum(rows)]).astype(np.int64)
    ofs = np.concatenate([[1], 1 + np.cumsum(rows * widths)]).astype(np.int64)
    val = np.zeros(int(ofs[-1]) + 7, dtype)
    val[:int(ofs[-1]) - 1] = rng.uniform(-1, 1, int(ofs[-1]) - 1)
    return V.SparseMatrix1DVBC(8, m, int(spl[-1] - 1), V.SplitPartition(spl), pos, idx + 1, ofs, val)


@pytest.mark.parametrize("typ", ["f64", "f32"])
def test_fused_split_multi(knobs, typ):
    """spmv_split_multi<T, P, MODE>: P in {2, 4, 8} x the slice loops the product library selects (0 and 2;
    MULTI_MODES_NOT_BUILT names the others).  320 stripes of widths 1 .. 8 in turn (eight buckets of one chunk each)
    run as ONE fused launch (planar_mask bit 5), every width a part of it, rows single and in runs of 3.  vbc_info
    does not report the slice loop; it follows the planner's rule (vbc_plan_bins.hip: batched when a wave's slice
    exceeds two steps of some bin): 2 stored rows per stripe keep every bin's slice within two steps (mode 0), 64 rows
    per stripe put the 8-wide bin's slice (8 rows or more per wave, steps of `run` rows) beyond them at every P
    (mode 2)."""
    assert set(MULTI_MODES_NOT_BUILT) == {1, 3}
    widths = np.arange(320) % 8 + 1
    for per in (2, 64):
        for run in (1, 3):
            base = uniform_rows(widths, per, 1000, DTYPE[typ], seed=per + run)
            B0 = expand_runs(base, run, seed=run) if run > 1 else base
            for P in (2, 4, 8):
                knobs({"VBC_PLANAR_SPLIT": str(P)})
                B, info = handle(B0, typ, "split")
                inf = info(True)
                print("split_multi", typ, per, run, P, {k: inf[k] for k in ("planar_bins", "planar_run", "planar_split", "planar_mask")})
                assert inf["planar_mask"] & 32 and inf["planar_split"] == P and inf["planar_bins"] == 8, inf
                assert inf["planar_run"] == run and inf["bins_t"] == 0 and inf["sweep_bins"] == 0, inf
                products(B, typ, "split_multi", True, exact=False, seed=per + run + P)
                B.release()


@pytest.mark.parametrize("typ", ["f64", "f32", "f64n"])
def test_forward_runs_paths(knobs, typ):
    """spmv_planar_fwd<T, w, R, FASTE, NB, KC, MASK, S>: (w, R) in {2, 3, 4} x {2, 3}, every write path."""
    keys = KeyForms()
    for w, R in FWD_WR:
        B0 = fwd_matrix(w, R, DTYPE[typ])
        for path, masked in FWD_PATHS:
            knobs(FWD, path)
            B, info = handle(B0, typ, "fwd")
            inf = info(False)
            print("fwd", typ, w, R, path, {k: inf[k] for k in ("fwd_run", "planar_mask")})
            assert inf["fwd_run"] == R and ((inf["planar_mask"] >> 1) & 1) == int(masked), (w, R, path, inf)
            assert not inf["planar_mask"] & (8 | 16 | 2048) and narrow_bit(inf, typ, "fwd"), (w, R, path, inf)
            keys.note((w, R), path, inf["bytes_f"])
            products(B, typ, "fwd", False, exact=False, seed=w + R)
            B.release()
    keys.check()


@pytest.mark.parametrize("typ", ["f64", "f32"])
def test_forward_split_waves(knobs, typ):
    """spmv_planar_fwd_split<T, w, R, P>: (w, R) in {2, 3, 4} x {2, 3} x P in {2, 4, 8} (no narrow form)."""
    for w, R in FWD_WR:
        B0 = fwd_matrix(w, R, DTYPE[typ])
        for P in (2, 4, 8):
            knobs({"VBC_PLANAR_PAIR": "0", "VBC_PLANAR_LANES": "0", "VBC_PLANAR_SPLIT": str(P), "VBC_SLOTS_PAD": "100"})
            B, info = handle(B0, typ, "fwd")
            inf = info(False)
            print("fwd_split", typ, w, R, P, {k: inf[k] for k in ("fwd_run", "planar_mask")})
            assert inf["fwd_run"] == R and inf["planar_mask"] & 8, (w, R, P, inf)
            products(B, typ, "fwd", False, exact=False, seed=w + R + P)
            B.release()


@pytest.fixture(scope="module")
def fe3d():
    """The 3-dof stiffness stand-in at its smallest size of test_gpu_planar.py, in both value types."""
    return {dt: V.synthetic.fe_stiffness_3d_1dvbc(30000, 300000, dtype=dt) for dt in (np.float64, np.float32)}


@pytest.mark.parametrize("typ", ["f64", "f64n"])
def test_lane_pairs(knobs, fe3d, typ):
    """spmv_planar_pair<FASTE, NB, KC, MASK, DOT, S> (B'x and the forward DOT form) and spmv_pair_lanes<RD, S>."""
    B0 = fe3d[DTYPE[typ]]
    keys = KeyForms()
    for path, masked in BX_PATHS:
        knobs(PAIR, path)
        B, info = handle(B0, typ, "pair")
        inf = info(True)
        print("pair", typ, path, {k: inf[k] for k in ("planar_bins", "planar_run", "planar_pair", "planar_mask")})
        assert inf["planar_bins"] == 1 and inf["planar_run"] == 3 and inf["planar_pair"] == 1, inf
        assert (inf["planar_mask"] & 1) == int(masked) and not inf["planar_mask"] & 4 and narrow_bit(inf, typ, "pair"), inf
        keys.note("pair", path, inf["bytes_t"])
        products(B, typ, "pair", True, exact=True, seed=3)
        B.release()
    keys.check()
    knobs(PAIR_LANES)
    B, info = handle(B0, typ, "pair_lanes")
    inf = info(True)
    assert inf["planar_mask"] & 4 and inf["planar_pair"] == 1 and narrow_bit(inf, typ, "pair_lanes"), inf
    products(B, typ, "pair_lanes", True, exact=True, seed=4)
    B.release()
    keys = KeyForms()
    for mask in ("0", "1"):
        for k16 in KEYS:
            path = dict({"VBC_PLANAR_MASK": mask, "VBC_SLOT_KEYS16": k16}, **({"VBC_SLOTS_PAD": "100"} if mask == "0" else {}))
            knobs(FWD_PAIR, path)
            B, info = handle(B0, typ, "pair_dot")
            inf = info(False)
            print("pair_dot", typ, path, {k: inf[k] for k in ("fwd_run", "planar_mask")})
            assert inf["planar_mask"] & 2048 and inf["fwd_run"] == 3 and narrow_bit(inf, typ, "pair_dot"), inf
            assert ((inf["planar_mask"] >> 1) & 1) == int(mask), inf
            keys.note("pair_dot", path, inf["bytes_f"])
            products(B, typ, "pair_dot", False, exact=True, seed=5)
            B.release()
    keys.check()
