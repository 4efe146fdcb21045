#!/usr/bin/env python3
"""Times a float32 matrix applied to Float64 vectors in three handles -- wide (no flag), 0x80
(VBC_CREATE_NARROW_VALUES: the swept buckets stay wide) and 0x1080 (0x80 | VBC_CREATE_NARROW_SWEPT) -- in the
protocol of tools/narrow_streams_time.py: every handle's product is first checked against the CPU oracle (given
val.astype(float64); normwise relative error <= 1e-12), then warm-up, then K products captured into one HIP graph,
one replay bracketed by events; --procs fresh processes per workload, each building the matrix once and timing the
three handles alternately, --reps replays each, the median kept per process.  The order of the handles (creation and
timing) rotates with the process and with the repetition.  Every process asserts that the three handles' products
are bitwise equal.  The parent reports median and range over the processes, the time ratio beside the byte ratio,
and writes --out.  0x1080 counts as faster on a workload only if its gap to the wide handle exceeds the wide
handle's own process-to-process range (`swept_gain_exceeds_wide_range`); on the control it must keep the 0x80
handle's bytes and bits, and `swept_inside_narrow_range` says whether its median lies inside the 0x80 handle's own
process-to-process range.

Workloads, `name:direction` (direction t = mul!(y, B', x), f = mul!(y, B, x)), all under the default knobs:
  ns:t   bench.py's NS matrix (the reference's costs.jl generator, 10^7 rows, w = 4), B'x: spmv_sweep, kind 0
  ns:f   the same matrix, B x: the forward swept product (kind 1) where the planner picks it
  fe:t   bench.py's FE-2D matrix, B'x: no swept bucket (the control: 0x1080 = 0x80)

Every child process runs under its own time limit (--limit seconds, timeout(1)); a child that fails ends the run.

    python tools/narrow_swept_time.py [--workloads ns:t,ns:f,fe:t --procs 3 --steps 50 --warmup 5 --reps 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HANDLES = (("wide", False), ("narrow", True), ("swept", "1080"))
TAG = "NARROW_SWEPT_TIME "
TOL = 1e-12  # fp64 products: the tolerance of tests/test_gpu_parity.py


def child(args):
    import numpy as np
    import torch

    import bench
    import sparsematrixvbcs_amd as V
    from oracle import oracle as O
    from sparsematrixvbcs_amd import _lib as L

    torch.set_num_threads(min(16, torch.get_num_threads()))
    name, direction = args.child.split(":")
    trans = direction == "t"
    device = torch.device("cuda:0")
    w = bench.build_matrix(name, np.float32, args.scale)
    order = [HANDLES[(i + args.rotate) % 3] for i in range(3)]
    if args.cycle == "rev":  # wide, swept, narrow: every handle follows the other neighbour
        order = [order[0], order[2], order[1]]
    B = {}
    for k, narrow in order:
        M = B[k] = V.SparseMatrix1DVBC(w.W, w.m, w.n, w.Phi, w.pos, w.idx, w.ofs, w.val)  # same arrays, own handles
        if narrow:
            M.narrow = True
        if narrow == "1080":  # exactly VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_SWEPT
            def with_swept(out, dev, flags, compute, create=M._create):
                return create(out, dev, flags | (L.VBC_CREATE_NARROW_SWEPT if flags & L.VBC_CREATE_NARROW_VALUES else 0),
                              compute)
            M._create = with_swept
    rng = np.random.default_rng(0xC0FFEE)
    nx, ny = (w.m, w.n) if trans else (w.n, w.m)
    xh = rng.uniform(-1, 1, nx)
    x = torch.from_numpy(xh).to(device)
    R = O.Ref1DVBC(w.m, w.n, w.W, w.Phi.spl, w.pos, w.idx, w.ofs, w.val.astype(np.float64))
    ref = O.mul(R, xh, np.zeros(ny), 1.0, 0.0, trans=trans, ref_semantics=False)
    del R
    stream = torch.cuda.Stream(device)
    out = {"workload": args.child, "nval": int(w.ofs[-1]) - 1, "order": [k for k, _ in order]}
    bytes_key = "bytes_t" if trans else "bytes_f"
    ys, graphs = {}, {}
    for k, M in B.items():
        A = M.T if trans else M
        y = ys[k] = torch.empty(ny, dtype=torch.float64, device=device)
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                V.mul_(y, A, x)
        torch.cuda.synchronize(device)
        got = y.cpu().numpy()
        err = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
        assert err <= TOL, f"{k}: relative error {err} against the oracle"
        inf = M.info(0, trans, compute=L.VBC_F64)
        out[k] = {f: int(inf[f]) for f in ("device_bytes", "slot_bins", "planar_bins", "sweep_bins", "bins_t", "bins_f",
                                          "planar_mask")}
        out[k]["bytes"] = int(inf[bytes_key])
        out[k]["oracle_rel_err"] = float(f"{err:.3e}")
        for f in ("narrow_t", "narrow_f", "narrow_swept_t", "narrow_swept_f"):
            out[k][f] = bool(inf[f])
        g = graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(args.steps):
                V.mul_(y, A, x)
        torch.cuda.synchronize(device)
    keys = [k for k, _ in order]
    us = {k: [] for k in keys}
    for rep in range(args.reps):
        for i in range(3):  # alternately, the first of the round rotating: a drift of the clocks hits all alike
            k = keys[(i + rep) % 3]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            with torch.cuda.stream(stream):
                e0.record(stream)
                graphs[k].replay()
                e1.record(stream)
            torch.cuda.synchronize(device)
            us[k].append(e0.elapsed_time(e1) / args.steps * 1e3)
    out["bitwise_equal"] = bool(torch.equal(ys["wide"], ys["narrow"]) and torch.equal(ys["wide"], ys["swept"]))
    assert out["bitwise_equal"], "the three handles' products differ"
    assert not torch.isnan(ys["wide"]).any()
    for k in keys:
        out[k]["us"] = round(statistics.median(us[k]), 2)
        out[k]["us_reps"] = [round(t, 2) for t in us[k]]
    print(TAG + json.dumps(out), flush=True)


def summary(runs, key):
    t = [r[key]["us"] for r in runs]
    s = {"median_us": round(statistics.median(t), 2), "min_us": min(t), "max_us": max(t), "per_process_us": t}
    s.update({f: v for f, v in runs[0][key].items() if f not in ("us", "us_reps")})
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="ns:t,ns:f,fe:t")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=300, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "narrow_swept_time.json"))
    ap.add_argument("--note", default="", help="free text stored with the result")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--rotate", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cycle", default="fwd", choices=["fwd", "rev"],
                    help="the cyclic order in which the handles are created and timed: fwd = wide, narrow, swept (each "
                         "handle is always timed after the same neighbour); rev = wide, swept, narrow")
    args = ap.parse_args()
    if args.child:
        return child(args)

    def fresh(wl, rotate):
        env = dict(os.environ)
        for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
            env[k] = str(min(16, int(env.get(k, "16") or 16)))
        p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--child", wl, "--rotate",
                            str(rotate), "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps),
                            "--scale", str(args.scale), "--cycle", args.cycle], capture_output=True, text=True, env=env)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"narrow_swept_time: the {wl} process failed (exit {p.returncode}); nothing further is run")
        return json.loads(line[0][len(TAG):])

    result = {"tool": "tools/narrow_swept_time.py", "product": "float32 values, Float64 x / y", "steps": args.steps,
              "warmup": args.warmup, "reps": args.reps, "procs": args.procs, "scale": args.scale, "cycle": args.cycle,
              "note": args.note,
              "workloads": {}}
    for wl in args.workloads.split(","):
        runs = []
        for i in range(args.procs):  # one fresh process after another (never two on the GPU at once)
            runs.append(fresh(wl, i))
            print(f"{wl} process {i}: " + "  ".join(f"{k} {runs[-1][k]['us']}" for k, _ in HANDLES), flush=True)
        s = {k: summary(runs, k) for k, _ in HANDLES}
        r = {"nval": runs[0]["nval"], "orders": [q["order"] for q in runs], **s,
             "bitwise_equal": all(q["bitwise_equal"] for q in runs),
             "wide_range_us": round(s["wide"]["max_us"] - s["wide"]["min_us"], 2)}
        for k in ("narrow", "swept"):
            r[k + "_time_ratio"] = round(s[k]["median_us"] / s["wide"]["median_us"], 4)
            r[k + "_byte_ratio"] = round(s[k]["bytes"] / s["wide"]["bytes"], 4)
            r[k + "_gain_us"] = round(s["wide"]["median_us"] - s[k]["median_us"], 2)
            r[k + "_gain_exceeds_wide_range"] = r[k + "_gain_us"] > r["wide_range_us"]
        r["swept_keeps_narrow_bytes_and_bits"] = all(s["swept"][f] == s["narrow"][f] for f in ("bytes", "device_bytes", "planar_mask"))
        r["swept_inside_narrow_range"] = s["narrow"]["min_us"] <= s["swept"]["median_us"] <= s["narrow"]["max_us"]
        result["workloads"][wl] = r
        print(f"{wl}: " + "  ".join(f"{k} {s[k]['median_us']} us [{s[k]['min_us']}, {s[k]['max_us']}]" for k, _ in HANDLES) +
              f"  swept time ratio {r['swept_time_ratio']} byte ratio {r['swept_byte_ratio']}  faster "
              f"{'yes' if r['swept_gain_exceeds_wide_range'] else 'not shown'}  "
              f"bits 20/21 {s['swept']['narrow_swept_t']}/{s['swept']['narrow_swept_f']}  sweep_bins {s['swept']['sweep_bins']}  "
              f"bitwise {r['bitwise_equal']}", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")  # (kept after every workload)


if __name__ == "__main__":
    main()
