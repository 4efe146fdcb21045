#!/usr/bin/env python3
"""Times mul!(y, B', x) of a float32 matrix on Float64 vectors with and without narrow value storage
(vbc.h VBC_CREATE_NARROW_VALUES, `B.narrow = True`), the way bench.py's measure() times its products: warm-up,
then K products captured into one HIP graph, one replay bracketed by events.

Workloads (bench.py build_matrix): `fe`, the FE-2D headline matrix (one slotted bucket: the narrow kernel), and
`ldoor`, the GHS_psdef/ldoor stand-in (no slotted bucket: the control, no change expected).  Every workload runs
in --procs fresh processes; each builds the matrix once and times the wide and the narrow handle alternately,
--reps replays each, keeping the median per process.  The parent reports median and range over the processes and
writes --out (profiles/narrow_fe2d.json).

    python tools/narrow_time.py [--workloads fe,ldoor --procs 3 --steps 50 --warmup 5 --reps 5 --scale 1.0]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def child(args):
    import numpy as np
    import torch

    import bench
    import sparsematrixvbcs_amd as V
    from sparsematrixvbcs_amd import _lib as L

    device = torch.device("cuda:0")
    B = {"wide": bench.build_matrix(args.child, np.float32, args.scale)}
    w = B["wide"]
    B["narrow"] = V.SparseMatrix1DVBC(w.W, w.m, w.n, w.Phi, w.pos, w.idx, w.ofs, w.val)  # same arrays, own handles
    B["narrow"].narrow = True
    rng = np.random.default_rng(0xC0FFEE)
    x = torch.from_numpy(rng.uniform(-1, 1, w.m)).to(device)
    stream = torch.cuda.Stream(device)
    out = {"workload": args.child, "nval": int(w.ofs[-1]) - 1}
    ys, graphs = {}, {}
    for k, M in B.items():
        y = ys[k] = torch.empty(w.n, dtype=torch.float64, device=device)
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                V.mul_(y, M.T, x)
        torch.cuda.synchronize(device)
        inf = M.info(0, True, compute=L.VBC_F64)
        out[k] = {f: int(inf[f]) for f in ("bytes_t", "device_bytes", "slot_bins", "planar_bins", "bins_t", "planar_mask")}
        out[k]["narrow_t"] = bool(inf["narrow_t"])
        g = graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(args.steps):
                V.mul_(y, M.T, x)
        torch.cuda.synchronize(device)
    out["bitwise_equal"] = bool(torch.equal(ys["wide"], ys["narrow"]))
    us = {k: [] for k in B}
    for _ in range(args.reps):
        for k in B:  # alternately: a drift of the clocks hits both alike
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
    print("NARROW_TIME " + json.dumps(out), flush=True)


def summary(runs, key):
    t = [r[key]["us"] for r in runs]
    return {"median_us": round(statistics.median(t), 2), "min_us": min(t), "max_us": max(t), "per_process_us": t,
            "bytes_t": runs[0][key]["bytes_t"], "device_bytes": runs[0][key]["device_bytes"],
            "narrow_t": runs[0][key]["narrow_t"], "slot_bins": runs[0][key]["slot_bins"],
            "planar_bins": runs[0][key]["planar_bins"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="fe,ldoor")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "narrow_fe2d.json"))
    ap.add_argument("--note", default="", help="free text stored with the result (which variant was timed)")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"tool": "tools/narrow_time.py", "product": "mul!(y, B', x), float32 values, Float64 x / y",
              "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "procs": args.procs, "scale": args.scale,
              "note": args.note, "workloads": {}}
    for wl in args.workloads.split(","):
        runs = []
        for _ in range(args.procs):  # one fresh process after another (never two on the GPU at once)
            p = subprocess.run([sys.executable, __file__, "--child", wl, "--steps", str(args.steps), "--warmup",
                                str(args.warmup), "--reps", str(args.reps), "--scale", str(args.scale)],
                               capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("NARROW_TIME ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"narrow_time: the {wl} process failed (exit {p.returncode}); nothing further is run")
            runs.append(json.loads(line[0][len("NARROW_TIME "):]))
        wide, narrow = summary(runs, "wide"), summary(runs, "narrow")
        r = {"nval": runs[0]["nval"], "wide": wide, "narrow": narrow,
             "bitwise_equal": all(q["bitwise_equal"] for q in runs),
             "time_ratio": round(narrow["median_us"] / wide["median_us"], 4),
             "byte_ratio": round(narrow["bytes_t"] / wide["bytes_t"], 4),
             "wide_range_us": round(wide["max_us"] - wide["min_us"], 2),
             "gain_us": round(wide["median_us"] - narrow["median_us"], 2)}
        r["gain_exceeds_wide_range"] = r["gain_us"] > r["wide_range_us"]
        result["workloads"][wl] = r
        print(f"{wl}: wide {wide['median_us']} us [{wide['min_us']}, {wide['max_us']}]  narrow {narrow['median_us']} us "
              f"[{narrow['min_us']}, {narrow['max_us']}]  time ratio {r['time_ratio']}  byte ratio {r['byte_ratio']}  "
              f"bitwise {r['bitwise_equal']}", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
