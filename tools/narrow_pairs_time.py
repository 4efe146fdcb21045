#!/usr/bin/env python3
"""Times a float32 matrix applied to Float64 vectors in three handles -- wide (no flag), `B.narrow = "planar"`
(vbc.h VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_PLANAR, 0x180: lane-pair buckets stay wide) and
`B.narrow = "pairs"` (0x180 | VBC_CREATE_NARROW_PAIRS, 0x580) -- in the protocol of tools/narrow_planar_time.py:
warm-up, then K products captured into one HIP graph, one replay bracketed by events; --procs fresh processes per
workload, each building the matrix once and timing the three handles alternately, --reps replays each, the median
kept per process.  The parent reports median and range over the processes, the time ratio beside the byte ratio,
and writes --out.  0x580 counts as faster on a workload only if its gap to the wide handle exceeds the wide
handle's own process-to-process range (`pairs_gain_exceeds_wide_range`); otherwise the gain is not shown.

Workloads, `name:direction` (direction t = mul!(y, B', x), f = mul!(y, B, x)):
  ldoor:t  the GHS_psdef/ldoor stand-in, B'x: spmv_planar_pair
  ldoor:f  the same matrix, B x: spmv_planar_pair in its forward (DOT) form
  fe3d:t   bench.py's FE-3D matrix, B'x under the default knobs: plain lane streams (spmv_planar_lanes), which keep
           Float64 values (the control)
  fe3dp:t  the same under VBC_LANES_PAIR=1: lane-pair streams, spmv_pair_lanes

--forms-lib LIB compares the two arrangements of a narrow run-row (vbc_kernels.h VBC_PAIR_FORM) instead: LIB is the
library built with the other arrangement (make -C sparsematrixvbcs.jl_amd pair_form_alt).  For each workload it runs
--procs rounds of two fresh processes, this library then LIB (alternating, never two on the GPU at once), each process
as above, and writes both forms' times side by side (default --out profiles/narrow_pairs_forms.json).

    python tools/narrow_pairs_time.py --forms-lib tools/exp/libs/libvbc_pair_form0.so --workloads ldoor:t
    python tools/narrow_pairs_time.py [--workloads ldoor:t,ldoor:f,fe3d:t,fe3dp:t --procs 3 --steps 50 --warmup 5 --reps 5]
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
HANDLES = (("wide", False), ("planar", "planar"), ("pairs", "pairs"))


def child(args):
    import numpy as np
    import torch

    import bench
    import sparsematrixvbcs_amd as V
    from sparsematrixvbcs_amd import _lib as L

    name, direction = args.child.split(":")
    trans = direction == "t"
    device = torch.device("cuda:0")
    if name == "fe3dp":  # (the knobs are read when a handle is created)
        os.environ["VBC_LANES_PAIR"] = "1"
    w = bench.build_matrix("fe3d" if name == "fe3dp" else name, np.float32, args.scale)
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
        out[k]["bytes_t"], out[k]["bytes_f"] = int(inf["bytes_t"]), int(inf["bytes_f"])
        for f in ("narrow_planar_t", "narrow_planar_f", "narrow_pair_t", "narrow_pair_f"):
            out[k][f] = bool(inf[f])
        g = graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(args.steps):
                V.mul_(y, A, x)
        torch.cuda.synchronize(device)
    out["bitwise_equal"] = bool(torch.equal(ys["wide"], ys["planar"]) and torch.equal(ys["wide"], ys["pairs"]))
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
    print("NARROW_PAIRS_TIME " + json.dumps(out), flush=True)


def summary(runs, key):
    t = [r[key]["us"] for r in runs]
    s = {"median_us": round(statistics.median(t), 2), "min_us": min(t), "max_us": max(t), "per_process_us": t}
    s.update({f: v for f, v in runs[0][key].items() if f not in ("us", "us_reps")})
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="ldoor:t,ldoor:f,fe3d:t,fe3dp:t")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--forms-lib", default="", help="the library built with the other run-row arrangement")
    ap.add_argument("--note", default="", help="free text stored with the result")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    args.out = args.out or str(ROOT / "profiles" / ("narrow_pairs_forms.json" if args.forms_lib else "narrow_pairs_time.json"))

    def fresh(wl, lib=None):
        env = dict(os.environ)
        if lib:
            env["VBC_LIBRARY"] = str(Path(lib).resolve())
        p = subprocess.run([sys.executable, __file__, "--child", wl, "--steps", str(args.steps), "--warmup",
                            str(args.warmup), "--reps", str(args.reps), "--scale", str(args.scale)],
                           capture_output=True, text=True, env=env)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("NARROW_PAIRS_TIME ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"narrow_pairs_time: the {wl} process failed (exit {p.returncode}); nothing further is run")
        return json.loads(line[0][len("NARROW_PAIRS_TIME "):])

    if args.forms_lib:
        result = {"tool": "tools/narrow_pairs_time.py --forms-lib", "product": "float32 values, Float64 x / y",
                  "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "procs": args.procs, "note": args.note,
                  "forms": {"this": "this library (VBC_PAIR_FORM as built)", "other": Path(args.forms_lib).name},
                  "workloads": {}}
        for wl in args.workloads.split(","):
            runs = {"this": [], "other": []}
            for _ in range(args.procs):
                runs["this"].append(fresh(wl))
                runs["other"].append(fresh(wl, args.forms_lib))
            r = {"bitwise_equal": all(q["bitwise_equal"] for f in runs for q in runs[f])}
            for f in runs:
                r[f] = {k: summary(runs[f], k) for k in ("wide", "pairs")}
                r[f]["time_ratio"] = round(r[f]["pairs"]["median_us"] / r[f]["wide"]["median_us"], 4)
                r[f]["byte_ratio"] = round(r[f]["pairs"]["bytes"] / r[f]["wide"]["bytes"], 4)
            gap = round(r["this"]["pairs"]["median_us"] - r["other"]["pairs"]["median_us"], 2)
            spread = round(max(r[f]["pairs"]["max_us"] - r[f]["pairs"]["min_us"] for f in runs), 2)
            r["other_minus_this_us"], r["pairs_range_us"] = -gap, spread
            r["faster"] = ("other" if gap > 0 else "this") if abs(gap) > spread else "not shown"
            result["workloads"][wl] = r
            print(f"{wl}: " + "  ".join(f"{f}: wide {r[f]['wide']['median_us']} pairs {r[f]['pairs']['median_us']} us "
                                        f"[{r[f]['pairs']['min_us']}, {r[f]['pairs']['max_us']}] ratio {r[f]['time_ratio']}"
                                        for f in runs) + f"  faster: {r['faster']}  bitwise {r['bitwise_equal']}", flush=True)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
        return
    result = {"tool": "tools/narrow_pairs_time.py", "product": "float32 values, Float64 x / y", "steps": args.steps,
              "warmup": args.warmup, "reps": args.reps, "procs": args.procs, "scale": args.scale, "note": args.note,
              "workloads": {}}
    for wl in args.workloads.split(","):
        runs = []
        for _ in range(args.procs):  # one fresh process after another (never two on the GPU at once)
            runs.append(fresh(wl))
        s = {k: summary(runs, k) for k, _ in HANDLES}
        r = {"nval": runs[0]["nval"], **s, "bitwise_equal": all(q["bitwise_equal"] for q in runs),
             "wide_range_us": round(s["wide"]["max_us"] - s["wide"]["min_us"], 2)}
        for k in ("planar", "pairs"):
            r[k + "_time_ratio"] = round(s[k]["median_us"] / s["wide"]["median_us"], 4)
            r[k + "_byte_ratio"] = round(s[k]["bytes"] / s["wide"]["bytes"], 4)
            r[k + "_gain_us"] = round(s["wide"]["median_us"] - s[k]["median_us"], 2)
            r[k + "_gain_exceeds_wide_range"] = r[k + "_gain_us"] > r["wide_range_us"]
        result["workloads"][wl] = r
        print(f"{wl}: " + "  ".join(f"{k} {s[k]['median_us']} us [{s[k]['min_us']}, {s[k]['max_us']}]" for k, _ in HANDLES) +
              f"  pairs time ratio {r['pairs_time_ratio']} byte ratio {r['pairs_byte_ratio']}  faster "
              f"{'yes' if r['pairs_gain_exceeds_wide_range'] else 'not shown'}  "
              f"bits 16/17 {s['pairs']['narrow_pair_t']}/{s['pairs']['narrow_pair_f']}  bitwise {r['bitwise_equal']}",
              flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")  # (kept after every workload)


if __name__ == "__main__":
    main()
