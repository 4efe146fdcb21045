#!/usr/bin/env python3
"""Times the column-major multi-RHS forward product Y = B X of the two workloads whose forward layouts the fused
kernels cover by themselves -- FE-2D (bench.py build_matrix "fe": forward row runs, spmm_planar_fwd_col) and the ldoor
stand-in ("ldoor": forward lane pairs, spmm_pair_col with DOT) -- the way tools/mm_planar_col_time.py times B'X:
warm-up, then K products captured into one HIP graph, one replay bracketed by events.

Forms: `fe-f64`, `fe-f32`, `fe-narrow` (float32 values on Float64 vectors, `B.narrow = "planar"`), `ldoor-f64` and
`ldoor-narrow` (`B.narrow = "pairs"`).  For every form and nrhs in --nrhs it measures

  fused      mulmat_(Y, B, X, engine="vector") on column-major operands (vbc.h planar_mask bit 25), in chunks of
             kMmFwdColChunk columns (csrc/vbc_handle.h; recorded as `chunk_cap`)
  fused_by2  nrhs > 2 only: the same product as calls of 2 columns each, i.e. what a chunk cap of 2 launches
             (NR = 2 instances only)
  nrhs_x_mul nrhs times the handle's single-vector mul_(y, B, x): code the fused kernels do not touch and exactly
             what a column-major forward product ran before -- the baseline of the acceptance rule
  mfma       mulmat_(Y, B, X, engine="mfma") on the column-major operands (a second copy of the matrix)

and compares the fused product with the product of a handle created under VBC_MM_FWD_COL=0 bit for bit.

Every form runs in --procs fresh processes, each under its own time limit; a failed process ends the run.  The
parent reports median and range over the processes, the smallest nrhs from which `fused` beats `nrhs_x_mul` by more
than the recorded spread in every form (and the nrhs at which it does not), the same for `fused_by2`, the sums over
the forms at nrhs = 8 that decide the chunk cap, and writes --out.  --append keeps the forms an existing --out
already holds (the workloads may be timed in separate runs) and recomputes the decisions over all of them.

    python tools/mm_fwd_col_time.py [--forms fe-f64,... --nrhs 2,4,8,16 --procs 3 --steps 20 --warmup 3 --reps 5]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# workload, value dtype, vector dtype, B.narrow
FORMS = {"fe-f64": ("fe", "float64", "float64", False), "fe-f32": ("fe", "float32", "float32", False),
         "fe-narrow": ("fe", "float32", "float64", "planar"), "ldoor-f64": ("ldoor", "float64", "float64", False),
         "ldoor-narrow": ("ldoor", "float32", "float64", "pairs")}
BIT25 = 1 << 25
TAG = "MM_FWD_COL_TIME "


def child(args):
    import numpy as np
    import torch

    import bench
    import sparsematrixvbcs_amd as V
    from sparsematrixvbcs_amd import _lib as L

    workload, vdt, xdt, narrow = FORMS[args.child]
    vdt, xdt = np.dtype(vdt), np.dtype(xdt)
    device = torch.device("cuda:0")
    code = L.dtype_code(xdt)
    base = bench.build_matrix(workload, vdt.type, args.scale)

    def handle_of(knob):
        M = V.SparseMatrix1DVBC(base.W, base.m, base.n, base.Phi, base.pos, base.idx, base.ofs, base.val)
        if narrow:
            M.narrow = narrow
        os.environ["VBC_MM_FWD_COL"] = knob
        M.handle(0, False, compute=code)  # (the knob is read when the handle is created)
        os.environ.pop("VBC_MM_FWD_COL", None)
        return M

    B = {"fused": handle_of("1"), "off": handle_of("0")}
    inf = {k: M.info(0, False, compute=code) for k, M in B.items()}
    assert inf["fused"]["planar_mask"] & BIT25, inf
    assert not inf["off"]["planar_mask"] & BIT25, inf
    assert inf["fused"]["planar_mask"] | BIT25 == inf["off"]["planar_mask"] | BIT25, inf
    out = {"form": args.child, "nval": int(base.ofs[-1]) - 1, "m": int(base.m), "n": int(base.n),
           "bytes_f": int(inf["fused"]["bytes_f"]), "device_bytes": int(inf["fused"]["device_bytes"]),
           "slot_bins": int(inf["fused"]["slot_bins"]), "fwd_run": int(inf["fused"]["fwd_run"]),
           "planar_mask": int(inf["fused"]["planar_mask"]), "nrhs": {}}
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

    def colmajor(rows, k):  # rows x k, column stride = rows (a Julia Matrix)
        return torch.empty((k, rows), dtype=tt, device=device).T

    def raw_equal(a, b):  # the raw bits of two column-major matrices (their transposes are contiguous)
        return bool(torch.equal(a.T.contiguous().view(torch.uint8), b.T.contiguous().view(torch.uint8)))

    x = torch.from_numpy(rng.uniform(-1, 1, base.n).astype(xdt)).to(device)
    y = torch.empty(base.m, dtype=tt, device=device)
    for k in [int(s) for s in args.nrhs.split(",")]:
        Xc = colmajor(base.n, k)
        Xc.copy_(torch.from_numpy(rng.uniform(-1, 1, (base.n, k)).astype(xdt)).to(device))
        Y = {v: colmajor(base.m, k) for v in ("fused", "fused_by2", "off", "mfma")}

        def by2():
            for c in range(0, k, 2):
                V.mulmat_(Y["fused_by2"][:, c:c + 2], B["fused"], Xc[:, c:c + 2], engine="vector")

        steps = max(2, args.steps // k)
        graphs = {
            "fused": (timed(lambda: V.mulmat_(Y["fused"], B["fused"], Xc, engine="vector"), steps), steps, 1),
            "nrhs_x_mul": (timed(lambda: V.mul_(y, B["fused"], x), args.steps), args.steps, k),
            "mfma": (timed(lambda: V.mulmat_(Y["mfma"], B["fused"], Xc, engine="mfma"), steps), steps, 1),
        }
        if k > 2 and k % 2 == 0:
            graphs["fused_by2"] = (timed(by2, steps), steps, 1)
        us = {v: [] for v in graphs}
        for _ in range(args.reps):
            for v, (g, st, mult) in graphs.items():  # alternately: a drift of the clocks hits all alike
                us[v].append(replay_us(g, st) * mult)
        with torch.cuda.stream(stream):
            V.mulmat_(Y["off"], B["off"], Xc, engine="vector")  # one SpMV per column: the product before
        torch.cuda.synchronize(device)
        im = B["fused"].info(0, False, multi=True, compute=code)
        r = {v: {"us": round(statistics.median(t), 2), "us_reps": [round(q, 2) for q in t]} for v, t in us.items()}
        r["mfma"]["bytes_m"] = int(im["bytes_m"])
        r["mfma"]["mfma_handle_device_bytes"] = int(im["device_bytes"])
        r["fused_equals_knob_off_bitwise"] = raw_equal(Y["fused"], Y["off"])
        if "fused_by2" in graphs:
            r["fused_by2_equals_knob_off_bitwise"] = raw_equal(Y["fused_by2"], Y["off"])
        ref = Y["off"].double()
        r["mfma_max_rel_diff"] = float(((Y["mfma"].double() - ref).abs().max() / ref.abs().max()).item())
        out["nrhs"][str(k)] = r
        del graphs
    print(TAG + json.dumps(out), flush=True)


VARIANTS = ("fused", "fused_by2", "nrhs_x_mul", "mfma")


def constant(name):
    src = (ROOT / "sparsematrixvbcs.jl_amd" / "csrc" / "vbc_handle.h").read_text()
    return int(re.search(name + r" = (\d+)", src).group(1))


def decide(result):
    """The decisions over every form the result holds (the rules of the kMmFwdCol* constants)."""
    wins, wins2 = {}, {}
    for f in result["forms"].values():
        for k, r in f["nrhs"].items():
            for v, w in (("fused", wins), ("fused_by2", wins2)):
                if v + "_wins" in r:
                    w.setdefault(int(k), []).append(r[v + "_wins"])
    ks = sorted(wins)
    lost = [k for k in ks if not all(wins[k])]
    from_k = [k for k in ks if all(all(wins[q]) for q in ks if q >= k)]
    result["fused_default_from_nrhs"] = from_k[0] if from_k else None  # smallest nrhs from which it wins in every form
    result["nrhs_not_won_in_every_form"] = lost
    result["fused_by2_nrhs_not_won_in_every_form"] = [k for k in sorted(wins2) if not all(wins2[k])]
    if all("8" in f["nrhs"] and "fused_by2" in f["nrhs"]["8"] for f in result["forms"].values()):
        result["nrhs8_sum_over_forms_us"] = {
            "chunk_cap_%d" % result["chunk_cap"]: round(sum(f["nrhs"]["8"]["fused"]["median_us"] for f in result["forms"].values()), 2),
            "chunk_cap_2": round(sum(f["nrhs"]["8"]["fused_by2"]["median_us"] for f in result["forms"].values()), 2)}
    print("forms", sorted(result["forms"]), "| fused wins in every form from nrhs =", result["fused_default_from_nrhs"],
          "not at", lost, "| by2 not at", result["fused_by2_nrhs_not_won_in_every_form"], "| nrhs 8 sums",
          result.get("nrhs8_sum_over_forms_us"), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--nrhs", default="2,4,8,16")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=360, help="time limit of one process, seconds")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mm_fwd_col_time.json"))
    ap.add_argument("--append", action="store_true", help="keep the forms --out already holds")
    ap.add_argument("--note", default="", help="free text stored with the result")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"tool": "tools/mm_fwd_col_time.py",
              "product": "mulmat_(Y, B, X) column-major forward, FE-2D and the ldoor stand-in (bench.py 'fe', 'ldoor')",
              "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "procs": args.procs, "scale": args.scale,
              "chunk_cap": constant("kMmFwdColChunk"), "min_rhs": constant("kMmFwdColMinRhs"), "note": args.note,
              "forms": {}}
    if args.append and Path(args.out).exists():
        old = json.loads(Path(args.out).read_text())
        for key in ("steps", "warmup", "reps", "procs", "scale", "chunk_cap"):
            if old[key] != result[key]:
                raise SystemExit(f"mm_fwd_col_time: --append onto a record with another {key}")
        result["forms"] = old["forms"]
    for form in args.forms.split(","):
        runs = []
        for _ in range(args.procs):  # one fresh process after another (never two on the GPU at once)
            cmd = [sys.executable, __file__, "--child", form, "--nrhs", args.nrhs, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--reps", str(args.reps), "--scale", str(args.scale)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"mm_fwd_col_time: the {form} process passed its time limit; nothing further is run")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"mm_fwd_col_time: the {form} process failed (exit {p.returncode}); nothing further is run")
            runs.append(json.loads(line[0][len(TAG):]))
            print(f"{form}: process {len(runs)} of {args.procs} done", flush=True)
        f = {k: runs[0][k] for k in ("nval", "m", "n", "bytes_f", "device_bytes", "slot_bins", "fwd_run", "planar_mask")}
        f["nrhs"] = {}
        for k in runs[0]["nrhs"]:
            r = {}
            for v in VARIANTS:
                if v not in runs[0]["nrhs"][k]:
                    continue
                t = [q["nrhs"][k][v]["us"] for q in runs]
                r[v] = {"median_us": round(statistics.median(t), 2), "min_us": min(t), "max_us": max(t), "per_process_us": t}
            r["mfma"]["bytes_m"] = runs[0]["nrhs"][k]["mfma"]["bytes_m"]
            r["mfma"]["mfma_handle_device_bytes"] = runs[0]["nrhs"][k]["mfma"]["mfma_handle_device_bytes"]
            for key in ("fused_equals_knob_off_bitwise", "fused_by2_equals_knob_off_bitwise"):
                if key in runs[0]["nrhs"][k]:
                    r[key] = all(q["nrhs"][k][key] for q in runs)
            r["mfma_max_rel_diff"] = max(q["nrhs"][k]["mfma_max_rel_diff"] for q in runs)
            for v in ("fused", "fused_by2"):
                if v not in r:
                    continue
                spread = max(r[q]["max_us"] - r[q]["min_us"] for q in (v, "nrhs_x_mul"))
                gain = round(r["nrhs_x_mul"]["median_us"] - r[v]["median_us"], 2)
                r[v + "_gain_us"], r[v + "_spread_us"], r[v + "_wins"] = gain, round(spread, 2), gain > spread
            f["nrhs"][k] = r
            print(f"{form} nrhs {k}: fused {r['fused']['median_us']} us  by2 {r.get('fused_by2', {}).get('median_us')}  "
                  f"nrhs x mul {r['nrhs_x_mul']['median_us']}  "
                  f"mfma {r['mfma']['median_us']}  gain {r['fused_gain_us']} (spread {r['fused_spread_us']})  "
                  f"bitwise {r['fused_equals_knob_off_bitwise']}", flush=True)
        result["forms"][form] = f
        decide(result)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")  # (after every form: a later failure keeps it)


if __name__ == "__main__":
    main()
