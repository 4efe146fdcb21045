#!/usr/bin/env python3
"""Times a float32 matrix applied to Float64 vectors in three handles -- wide (no flag), `B.narrow = True`
(vbc.h VBC_CREATE_NARROW_VALUES) and `B.narrow = "planar"` (VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_PLANAR) --
in the protocol of tools/narrow_time.py: warm-up, then K products captured into one HIP graph, one replay
bracketed by events; --procs fresh processes per workload, each building the matrix once and timing the three
handles alternately, --reps replays each, the median kept per process.  The parent reports median and range over
the processes and writes --out.

Workloads, `name:direction` (direction t = mul!(y, B', x), f = mul!(y, B, x)):
  fe:f     bench.py's FE-2D matrix, forward product: one forward planar bucket (spmv_planar_fwd, 2 x 2 blocks)
  fe4:t    the same 5-point mesh with 4 unknowns per node at the same 1.0e8 values (N = 1118): B'x runs one
           chunk-planar bucket of 4-wide stripes with row runs of 2 under the default knobs (spmv_planar) -- the
           smallest width whose Float32 row is one full 16-B group
  ldoor:t  the GHS_psdef/ldoor stand-in: lane-pair buckets, which keep Float64 values (the control)

    python tools/narrow_planar_time.py [--workloads fe:f,fe4:t,ldoor:t --procs 3 --steps 50 --warmup 5 --reps 5]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HANDLES = (("wide", False), ("narrow", True), ("planar", "planar"))


def child(args):
    import numpy as np
    import torch

    import bench
    import sparsematrixvbcs_amd as V
    from sparsematrixvbcs_amd import _lib as L

    name, direction = args.child.split(":")
    trans = direction == "t"
    device = torch.device("cuda:0")
    if name == "fe4":
        w = V.synthetic.fe_grid_2d(int(round(1118 * args.scale ** 0.5)), dof=4, dtype=np.float32)
    else:
        w = bench.build_matrix(name, np.float32, args.scale)
    B = {}
    for k, narrow in HANDLES:
        B[k] = V.SparseMatrix1DVBC(w.W, w.m, w.n, w.Phi, w.pos, w.idx, w.ofs, w.val)  # same arrays, own handles
        if narrow:
            B[k].narrow = narrow
    rng = np.random.default_rng(0xC0FFEE)
    nx, ny = (w.m, w.n) if trans else (w.n, w.m)
    x = torch.from_numpy(rng.uniform(-1, 1, nx)).to(device)
    stream = torch.cuda.Stream(device)
    out = {"workload": args.child, "nval": int(w.ofs[-1]) - 1}
    bytes_key = "bytes_t" if trans else "bytes_f"
    ys, graphs = {}, {}
    for k, M in B.items():
        A = M.T if trans else M
        y = ys[k] = torch.empty(ny, dtype=torch.float64, device=device)
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                V.mul_(y, A, x)
        torch.cuda.synchronize(device)
        inf = M.info(0, trans, compute=L.VBC_F64)
        out[k] = {f: int(inf[f]) for f in ("device_bytes", "slot_bins", "planar_bins", "bins_t", "bins_f", "planar_mask",
                                          "planar_run", "planar_pair", "planar_split", "fwd_run")}
        out[k]["bytes"] = int(inf[bytes_key])
        for f in ("narrow_t", "narrow_f", "narrow_planar_t", "narrow_planar_f"):
            out[k][f] = bool(inf[f])
        g = graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(args.steps):
                V.mul_(y, A, x)
        torch.cuda.synchronize(device)
    out["bitwise_equal"] = bool(torch.equal(ys["wide"], ys["narrow"]) and torch.equal(ys["wide"], ys["planar"]))
    us = {k: [] for k in B}
    for _ in range(args.reps):
        for k in B:  # alternately: a drift of the clocks hits all alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            with torch.cuda.stream(stream):
                e0.record(stream)
                graphs[k].replay()
                e1.record(stream)
            torch.cuda.synchronize(device)
            us[k].append(e0.elapsed_time(e1) / args.steps * 1e3)
    for k in B:
        out[k]["us"] = round(statistics.median(us[k]), 2)
        out[k]["us_reps"] = [round(t, 2) for t in us[k]]
    print("NARROW_PLANAR_TIME " + json.dumps(out), flush=True)


def summary(runs, key):
    t = [r[key]["us"] for r in runs]
    s = {"median_us": round(statistics.median(t), 2), "min_us": min(t), "max_us": max(t), "per_process_us": t}
    s.update({f: v for f, v in runs[0][key].items() if f not in ("us", "us_reps")})
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="fe:f,fe4:t,ldoor:t")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "narrow_planar_time.json"))
    ap.add_argument("--note", default="", help="free text stored with the result")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"tool": "tools/narrow_planar_time.py", "product": "float32 values, Float64 x / y", "steps": args.steps,
              "warmup": args.warmup, "reps": args.reps, "procs": args.procs, "scale": args.scale, "note": args.note,
              "workloads": {}}
    for wl in args.workloads.split(","):
        runs = []
        for _ in range(args.procs):  # one fresh process after another (never two on the GPU at once)
            p = subprocess.run([sys.executable, __file__, "--child", wl, "--steps", str(args.steps), "--warmup",
                                str(args.warmup), "--reps", str(args.reps), "--scale", str(args.scale)],
                               capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("NARROW_PLANAR_TIME ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"narrow_planar_time: the {wl} process failed (exit {p.returncode}); nothing further is run")
            runs.append(json.loads(line[0][len("NARROW_PLANAR_TIME "):]))
        s = {k: summary(runs, k) for k, _ in HANDLES}
        r = {"nval": runs[0]["nval"], **s, "bitwise_equal": all(q["bitwise_equal"] for q in runs),
             "wide_range_us": round(s["wide"]["max_us"] - s["wide"]["min_us"], 2)}
        for k in ("narrow", "planar"):
            r[k + "_time_ratio"] = round(s[k]["median_us"] / s["wide"]["median_us"], 4)
            r[k + "_byte_ratio"] = round(s[k]["bytes"] / s["wide"]["bytes"], 4)
            r[k + "_gain_us"] = round(s["wide"]["median_us"] - s[k]["median_us"], 2)
            r[k + "_gain_exceeds_wide_range"] = r[k + "_gain_us"] > r["wide_range_us"]
        result["workloads"][wl] = r
        print(f"{wl}: " + "  ".join(f"{k} {s[k]['median_us']} us [{s[k]['min_us']}, {s[k]['max_us']}]" for k, _ in HANDLES) +
              f"  planar time ratio {r['planar_time_ratio']} byte ratio {r['planar_byte_ratio']}  "
              f"bits 14/15 {s['planar']['narrow_planar_t']}/{s['planar']['narrow_planar_f']}  bitwise {r['bitwise_equal']}",
              flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")  # (kept after every workload)


if __name__ == "__main__":
    main()
