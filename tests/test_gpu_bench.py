"""bench.py as the driver runs it: `python bench.py --gpus N` with NO torchrun variables must start its
N ranks itself (one process per GPU, rank 0 prints the one JSON line), and N = 1 must print the same
kind of line.  On the one-GPU box the two ranks share cuda:0 over gloo (`--same-device`), which
rehearses the code path (the numbers are not a measurement).  Replaces the reference's threaded
stripe loop as the unit of parallel work (multiply_1DVBC.jl:169-177)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DIST_VARS = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
             "GROUP_RANK", "ROLE_RANK", "TORCHELASTIC_RUN_ID")


def run_bench(*args, timeout=110):
    env = {k: v for k, v in os.environ.items() if k not in DIST_VARS}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]  # exactly one JSON line (rank 0 only)
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    d = run_bench("--gpus", "2", "--backend", "gloo", "--same-device", "--scale", "0.01", "--full", "--no-secondary",
                  "--no-abi-sharded", "--steps", "3", "--warmup", "1")
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["unit"] == "GB/s" and d["scaling"] == "strong"
    assert "stripe split x2" in d["config"]["parallelism"]
    assert d["parity"]["pass"] and d["parity"]["serial_bitwise_equal"]


def test_bench_multi_gpu_line_checks_itself():
    """the N > 1 line proves its numbers: the primary's gathered y, the C3 secondary's B'x
    and its forward all_reduce, and the one-process C-ABI sharded leg (vbc1d_create_sharded, devices
    [0, 0] on a one-GPU box) are all compared with the oracle."""
    d = run_bench("--gpus", "2", "--backend", "gloo", "--same-device", "--scale", "0.01", "--full", "--steps", "3",
                  "--warmup", "1", timeout=300)
    assert d["parity"]["pass"] and len(d["parity"]["slices_bitwise"]) == 2
    c3 = d["secondary"]["c3_ldoor"]
    assert c3["parity"]["pass"] and c3["forward_allreduce"]["parity"]["pass"]
    abi = d["secondary"]["abi_sharded"]
    assert abi["pass"] and abi["devices"] == [0, 0], abi
    for k in ("transposed", "forward"):
        assert abi[k]["parity"]["pass"] and abi[k]["value"] > 0


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run times exactly --steps products and nothing else: the line keeps the headline fields
    and leaves out what --full adds.  --dump-outputs writes the y of the last timed product; the inputs
    are seeded, so the same matrix and x rebuilt here give the oracle's y for it (fp64: 1e-12)."""
    import numpy as np

    import bench
    from oracle import oracle as O
    d = run_bench("--gpus", "1", "--scale", "0.01", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1
    assert d["value"] > 0 and d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["metric"] == bench.METRIC and d["ms_per_step"] > 0
    # value = bytes per product / the time of one timed step (ms_per_step is printed to 1e-5 ms: 1 % of 1 us)
    assert d["value"] == pytest.approx(d["roofline"]["bytes_per_launch"] / (d["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    assert d["cpu_baseline"] is None and d["parity"] is None
    assert not {"secondary", "device", "rel_err"} & set(d)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["y.npy"]
    y = np.load(tmp_path / "y.npy")
    B = bench.build_matrix("fe", np.float64, 0.01)
    assert y.dtype == np.float64 and y.shape == (B.n,) and d["dump"]["y"] == {
        "elements": B.n, "dtype": "float64", "sampled": False}
    x = np.random.default_rng(0xC0FFEE).uniform(-1, 1, B.m)
    R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, B.val)
    ref = O.mul(R, x, np.zeros(B.n), trans=True)
    assert np.linalg.norm(y - ref) / np.linalg.norm(ref) <= 1e-12


def test_bench_plain_two_ranks_dump_their_slices(tmp_path):
    """N > 1 without --full: the timed products only (no e2e leg, parity or secondary); every rank dumps
    its y slice, and the slices in rank order are the single-GPU y (the oracle's, fp64: 1e-12)."""
    import numpy as np

    import bench
    from oracle import oracle as O
    d = run_bench("--gpus", "2", "--backend", "gloo", "--same-device", "--scale", "0.01", "--steps", "3",
                  "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["e2e"] is None and d["parity"] is None and d["secondary"] == {}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["y_rank0.npy", "y_rank1.npy"]
    y = np.concatenate([np.load(tmp_path / f"y_rank{r}.npy") for r in range(2)])
    B = bench.build_matrix("fe", np.float64, 0.01)
    x = np.random.default_rng(0xC0FFEE).uniform(-1, 1, B.m)
    R = O.Ref1DVBC(B.m, B.n, B.W, B.Phi.spl, B.pos, B.idx, B.ofs, B.val)
    ref = O.mul(R, x, np.zeros(B.n), trans=True)
    assert y.dtype == np.float64 and y.shape == ref.shape
    assert np.linalg.norm(y - ref) / np.linalg.norm(ref) <= 1e-12


def test_dump_outputs_samples_a_large_array(tmp_path):
    """An array above its share of the size cap is cut to the same sorted seeded sample every time."""
    import numpy as np
    import torch

    import bench
    t = torch.arange(1000, dtype=torch.float32, device="cuda")
    for sub in ("a", "b"):
        info = bench.dump_outputs(tmp_path / sub, {"y": t, "z": t[:100].double()}, budget=1600)
        assert info["y"] == {"elements": 1000, "dtype": "float32", "sampled": True, "kept": 200, "seed": bench.DUMP_SEED}
        assert info["z"] == {"elements": 100, "dtype": "float64", "sampled": False}
    ya, yb = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert ya.dtype == np.float32 and ya.shape == (200,) and np.array_equal(ya, yb)
    assert np.all(np.diff(ya) > 0) and ya[-1] > 500  # distinct elements in index order, from the whole array
    assert np.array_equal(np.load(tmp_path / "a" / "z.npy"), np.arange(100.0))


def test_bench_single_gpu_line():
    d = run_bench("--scale", "0.01", "--full", "--no-secondary", "--no-cpu-baseline", "--steps", "3", "--warmup", "1")
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert d["roofline"]["frac"] > 0 and d["roofline"]["bound"] == "hbm"
    assert d["parity"]["pass"] and d["parity"]["rel_err"] <= 1e-10
    assert "cache" in d["config"]
