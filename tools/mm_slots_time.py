#!/usr/bin/env python3
"""Times the row-major multi-RHS product Y = B'X of the FE-2D headline matrix (bench.py build_matrix "fe": one
slotted bucket) the way bench.py's measure() times its products: warm-up, then K products captured into one HIP
graph, one replay bracketed by events.

Forms: `f64`, `f32`, and `narrow` (float32 values on Float64 vectors, `B.narrow = True`).  For every form and
nrhs in --nrhs it measures

  fused      mulmat_(Y, B', X, engine="vector"): spmm_slots (vbc.h planar_mask bit 22)
  percol     the same call on a handle created under VBC_MM_SLOTS=0: one SpMV per column through the handle's
             column temporaries, the path before spmm_slots
  nrhs_x_mul nrhs times the handle's single-vector mul_(y, B', x): code spmm_slots does not touch and a lower
             bound of `percol`, which adds the strided copies -- the baseline of the acceptance rule
  mfma       mulmat_(Y, B', X, engine="mfma") with its bytes_m and the device_bytes of the handle that holds the
             panel layout (a second copy of the matrix)

Every form runs in --procs fresh processes; each builds the matrix once and times the variants alternately, --reps
replays each, keeping the median per process.  The parent reports median and range over the processes, the
smallest nrhs at which `fused` beats `nrhs_x_mul` by more than the recorded spread in every form (and the nrhs at
which it does not), and writes --out.

    python tools/mm_slots_time.py [--forms f64,f32,narrow --nrhs 2,4,8,16 --procs 3 --steps 20 --warmup 3 --reps 5]
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

FORMS = {"f64": ("float64", "float64", False), "f32": ("float32", "float32", False),
         "narrow": ("float32", "float64", True)}  # value dtype, vector dtype, B.narrow
BIT22 = 1 << 22


def child(args):
    import numpy as np
    import torch

    import bench
    import sparsematrixvbcs_amd as V
    from sparsematrixvbcs_amd import _lib as L

    vdt, xdt, narrow = FORMS[args.child]
    vdt, xdt = np.dtype(vdt), np.dtype(xdt)
    device = torch.device("cuda:0")
    code = L.dtype_code(xdt)
    base = bench.build_matrix("fe", vdt.type, args.scale)

    def handle_of(knob):
        M = V.SparseMatrix1DVBC(base.W, base.m, base.n, base.Phi, base.pos, base.idx, base.ofs, base.val)
        M.narrow = narrow
        if knob is not None:
            os.environ["VBC_MM_SLOTS"] = knob
        M.handle(0, True, compute=code)  # (the knob is read when the handle is created)
        os.environ.pop("VBC_MM_SLOTS", None)
        return M

    B = {"fused": handle_of(None), "percol": handle_of("0")}
    inf = {k: M.info(0, True, compute=code) for k, M in B.items()}
    assert inf["fused"]["planar_mask"] & BIT22 and not inf["percol"]["planar_mask"] & BIT22, inf
    out = {"form": args.child, "nval": int(base.ofs[-1]) - 1, "m": int(base.m), "n": int(base.n),
           "bytes_t": int(inf["fused"]["bytes_t"]), "device_bytes": int(inf["fused"]["device_bytes"]),
           "slot_bins": int(inf["fused"]["slot_bins"]), "nrhs": {}}
    rng = np.random.default_rng(0xC0FFEE)
    stream = torch.cuda.Stream(device)
    tt = getattr(torch, xdt.name)

    def timed(fn, steps):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize(device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(steps):
                fn()
        torch.cuda.synchronize(device)
        return g

    def replay_us(g, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(device)
        with torch.cuda.stream(stream):
            e0.record(stream)
            g.replay()
            e1.record(stream)
        torch.cuda.synchronize(device)
        return e0.elapsed_time(e1) / steps * 1e3

    x = torch.from_numpy(rng.uniform(-1, 1, base.m).astype(xdt)).to(device)
    y = torch.empty(base.n, dtype=tt, device=device)
    for k in [int(s) for s in args.nrhs.split(",")]:
        X = torch.from_numpy(rng.uniform(-1, 1, (base.m, k)).astype(xdt)).to(device)
        Y = {v: torch.empty((base.n, k), dtype=tt, device=device) for v in ("fused", "percol", "mfma")}
        steps = max(2, args.steps // k)
        graphs = {
            "fused": (timed(lambda: V.mulmat_(Y["fused"], B["fused"].T, X, engine="vector"), steps), steps, 1),
            "percol": (timed(lambda: V.mulmat_(Y["percol"], B["percol"].T, X, engine="vector"), steps), steps, 1),
            "nrhs_x_mul": (timed(lambda: V.mul_(y, B["fused"].T, x), args.steps), args.steps, k),
            "mfma": (timed(lambda: V.mulmat_(Y["mfma"], B["fused"].T, X, engine="mfma"), steps), steps, 1),
        }
        us = {v: [] for v in graphs}
        for _ in range(args.reps):
            for v, (g, st, mult) in graphs.items():  # alternately: a drift of the clocks hits all alike
                us[v].append(replay_us(g, st) * mult)
        im = B["fused"].info(0, True, multi=True, compute=code)
        r = {v: {"us": round(statistics.median(t), 2), "us_reps": [round(q, 2) for q in t]} for v, t in us.items()}
        r["mfma"]["bytes_m"] = int(im["bytes_m"])
        r["mfma"]["mfma_handle_device_bytes"] = int(im["device_bytes"])
        r["fused_equals_percol_bitwise"] = bool(torch.equal(Y["fused"], Y["percol"]))
        ref = Y["percol"].double()
        r["mfma_max_rel_diff"] = float(((Y["mfma"].double() - ref).abs().max() / ref.abs().max()).item())
        out["nrhs"][str(k)] = r
        del graphs
    print("MM_SLOTS_TIME " + json.dumps(out), flush=True)


VARIANTS = ("fused", "percol", "nrhs_x_mul", "mfma")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--forms", default="f64,f32,narrow")
    ap.add_argument("--nrhs", default="2,4,8,16")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mm_slots_time.json"))
    ap.add_argument("--note", default="", help="free text stored with the result")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"tool": "tools/mm_slots_time.py", "product": "mulmat_(Y, B', X) row-major, FE-2D (bench.py 'fe')",
              "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "procs": args.procs, "scale": args.scale,
              "note": args.note, "forms": {}}
    wins = {}
    for form in args.forms.split(","):
        runs = []
        for _ in range(args.procs):  # one fresh process after another (never two on the GPU at once)
            p = subprocess.run([sys.executable, __file__, "--child", form, "--nrhs", args.nrhs, "--steps", str(args.steps),
                                "--warmup", str(args.warmup), "--reps", str(args.reps), "--scale", str(args.scale)],
                               capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("MM_SLOTS_TIME ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"mm_slots_time: the {form} process failed (exit {p.returncode}); nothing further is run")
            runs.append(json.loads(line[0][len("MM_SLOTS_TIME "):]))
            print(f"{form}: process {len(runs)} of {args.procs} done", flush=True)
        f = {k: runs[0][k] for k in ("nval", "m", "n", "bytes_t", "device_bytes", "slot_bins")}
        f["nrhs"] = {}
        for k in runs[0]["nrhs"]:
            r = {}
            for v in VARIANTS:
                t = [q["nrhs"][k][v]["us"] for q in runs]
                r[v] = {"median_us": round(statistics.median(t), 2), "min_us": min(t), "max_us": max(t), "per_process_us": t}
            r["mfma"]["bytes_m"] = runs[0]["nrhs"][k]["mfma"]["bytes_m"]
            r["mfma"]["mfma_handle_device_bytes"] = runs[0]["nrhs"][k]["mfma"]["mfma_handle_device_bytes"]
            r["fused_equals_percol_bitwise"] = all(q["nrhs"][k]["fused_equals_percol_bitwise"] for q in runs)
            r["mfma_max_rel_diff"] = max(q["nrhs"][k]["mfma_max_rel_diff"] for q in runs)
            spread = max(r[v]["max_us"] - r[v]["min_us"] for v in ("fused", "nrhs_x_mul"))
            r["gain_us"] = round(r["nrhs_x_mul"]["median_us"] - r["fused"]["median_us"], 2)
            r["spread_us"] = round(spread, 2)
            r["fused_wins"] = r["gain_us"] > r["spread_us"]
            wins.setdefault(int(k), []).append(r["fused_wins"])
            f["nrhs"][k] = r
            print(f"{form} nrhs {k}: fused {r['fused']['median_us']} us  percol {r['percol']['median_us']}  "
                  f"nrhs x mul {r['nrhs_x_mul']['median_us']}  mfma {r['mfma']['median_us']}  gain {r['gain_us']} "
                  f"(spread {r['spread_us']})  bitwise {r['fused_equals_percol_bitwise']}", flush=True)
        result["forms"][form] = f
    ks = sorted(wins)
    ok = [k for k in ks if all(wins[k])]
    result["fused_default_from_nrhs"] = ok[0] if ok else None  # smallest nrhs it wins at in every form; None: never
    result["nrhs_not_won_in_every_form"] = [k for k in ks if not all(wins[k])]
    print("fused wins in every form at nrhs =", ok, "not at", result["nrhs_not_won_in_every_form"], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
