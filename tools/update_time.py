"""What a value update costs (vbc.h vbc_update_values) against the only other route, destroy + create.

For one workload per process (a fresh process per matrix, as bench.py measures), B'x handle:
  (a) vbc_update_values from a device val: events around a HIP graph of K updates, after warm-up;
  (b) the same from a host val (staging copy + kernel + synchronise; wall clock);
  (c) destroy + create with the new values, not updatable (wall clock);
  (d) create with and without VBC_CREATE_UPDATABLE (wall clock);
  (e) one product (events around a graph of K products).
The update moves about slots x (2 esz + 4) bytes (source value, stored value, map entry); slots is taken from
the map's size, (device_bytes with the flag - device_bytes without) / 4.  (a) is also given as the fraction of
8 TB/s that traffic reaches.  One JSON line; --out writes it to a file as well.

    python tools/update_time.py --workload fe|ldoor [--scale 1.0] [--steps 20] [--warmup 5] [--out FILE]

--shards N --split stripes|rows measures the sharded handle instead (vbc.h vbc_sharded_update_values,
devices = [0] * N: every shard on one GPU, no communicator), with the same protocols:
  (a) the sharded update from a device val (graph of K updates);
  (a') row split: the update without its pack kernel -- the N shard updates on slices of an already packed
       val -- and the pack kernel alone as the difference of the two graph times;
  (c) destroy + create of the sharded handle with new values, not updatable (wall clock);
  (d) create with and without VBC_CREATE_UPDATABLE_SHARDS; (e) one B'x product.

--narrow [--processes 3] measures the update of a narrow handle (vbc.h VBC_CREATE_NARROW_UPDATABLE): the bench's
FE-2D matrix as float32 on Float64 B'x handles, a device val of float32, in `--processes` fresh processes that each
time both handles alternately (events around a graph of K updates, median of 5, twice each):
  (a) the wide updatable handle (VBC_CREATE_UPDATABLE, float32 val widened by the kernel);
  (b) the VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_UPDATABLE handle;
and one B'x product of (b) against the narrow handle that is not updatable (the same kernel on the same bytes).
(b) counts as faster only if the gap of the medians exceeds (a)'s own process-to-process range.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def graph_time_us(torch, s, fn, steps, warmup, reps=5):
    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(steps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            g.replay()
            e1.record(s)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / steps)
    return float(np.median(times)), [round(t, 2) for t in times]


def wall_ms(torch, fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 1) for t in times]


def sharded_main(args, torch, V, B):
    import ctypes as C
    D, L, lib = V.distributed, V._lib, V._lib.lib()
    N, devices = args.shards, [0] * args.shards
    esz = B.val.dtype.itemsize
    nval = int(B.ofs[-1]) - 1
    rng = np.random.default_rng(7)
    v2 = rng.uniform(-1, 1, len(B.val))
    d2 = torch.from_numpy(v2).cuda()

    def with_values(v):
        return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, v)

    def make(v, upd):
        return D.MultiGPUSparseMatrix1DVBC(with_values(v), devices=devices, split=args.split, forward=False,
                                           updatable=upd)
    hold = {}
    create_plain, _ = wall_ms(torch, lambda: hold.__setitem__("P", make(B.val, False)), 1)
    create_upd, _ = wall_ms(torch, lambda: hold.__setitem__("U", make(B.val, True)), 1)
    P, U = hold["P"], hold["U"]
    slots = sum(U.shard_info(g)["device_bytes"] - P.shard_info(g)["device_bytes"] for g in range(N)) // 4
    traffic = slots * (2 * esz + 4)

    def recreate():
        hold["P"].release()
        hold["P"] = make(v2, False)
    recreate_ms, recreate_all = wall_ms(torch, recreate, 2)
    P = hold["P"]

    s = torch.cuda.Stream()
    x = torch.from_numpy(rng.uniform(-1, 1, B.m)).cuda()
    y = torch.empty(B.n, dtype=torch.float64, device="cuda")

    def update_dev():
        L.check(lib.vbc_sharded_update_values(U._h, d2.data_ptr(), len(v2), L.VBC_F64, L.VBC_MEM_DEVICE, s.cuda_stream))
    upd_us, upd_all = graph_time_us(torch, s, update_dev, args.steps, args.warmup)
    out = {"tool": "update_time", "workload": args.workload, "scale": args.scale, "dtype": "float64", "shards": N,
           "split": args.split, "devices": devices, "m": B.m, "n": B.n, "nval": nval, "value_slots": int(slots),
           "update_device_us": round(upd_us, 2), "update_device_us_all": upd_all,
           "update_traffic_bytes": int(traffic)}
    if args.split == "rows" and N > 1:  # the shard updates alone, on slices of a val packed beforehand
        kind = L.VBC_SPLIT_ROWS
        vbase = np.zeros(N + 1, np.int64)
        nruns = C.c_int64()
        plan = lambda runs: L.check(lib.vbcx_sharded_value_plan(
            B.m, B.n, 0, None, len(B.Phi), B.Phi.spl.ctypes.data, B.pos.ctypes.data, B.idx.ctypes.data,
            B.ofs.ctypes.data, esz, N, kind, None, vbase.ctypes.data, None, C.byref(nruns),
            None if runs is None else runs.ctypes.data, 0 if runs is None else len(runs)))
        plan(None)
        runs = np.zeros((nruns.value, 3), np.int64)
        plan(runs)
        src = np.repeat(runs[:, 0] - runs[:, 1], runs[:, 2]) + np.arange(nval)
        packed = d2[torch.from_numpy(src).cuda()].contiguous()
        hs = [U.shard_handle(g) for g in range(N)]

        def shards_only():
            for g in range(N):
                cnt = int(vbase[g + 1] - vbase[g])
                if cnt:
                    L.check(lib.vbc_update_values(hs[g], packed.data_ptr() + int(vbase[g]) * esz, cnt, L.VBC_F64,
                                                  L.VBC_MEM_DEVICE, s.cuda_stream))
        only_us, only_all = graph_time_us(torch, s, shards_only, args.steps, args.warmup)
        pack_us = upd_us - only_us
        out.update({"runs": int(nruns.value), "mean_run_elements": round(nval / max(nruns.value, 1), 1),
                    "shard_updates_only_us": round(only_us, 2), "shard_updates_only_us_all": only_all,
                    "pack_us": round(pack_us, 2), "pack_traffic_bytes": int(2 * nval * esz + 16 * nruns.value),
                    "pack_TBs": round((2 * nval * esz + 16 * nruns.value) / (pack_us * 1e-6) / 1e12, 3)})
        update_dev()  # leave U holding v2 again
    prod_us, prod_all = graph_time_us(torch, s, lambda: V.mul_(y, U.T, x), args.steps, args.warmup)
    y2 = torch.empty_like(y)
    V.mul_(y2, P.T, x)
    V.mul_(y, U.T, x)
    torch.cuda.synchronize()
    out.update({"update_frac_of_8TBs": round(traffic / (upd_us * 1e-6) / 8e12, 3),
                "recreate_ms": round(recreate_ms, 1), "recreate_ms_all": recreate_all,
                "create_ms": round(create_plain, 1), "create_updatable_ms": round(create_upd, 1),
                "product_us": round(prod_us, 2), "product_us_all": prod_all,
                "update_below_recreate": bool(upd_us * 1e-3 < recreate_ms),
                "bitwise_equal_to_recreated": bool(torch.equal(y, y2)),
                "single_handle_update_us": 278, "single_handle_recreate_ms": 489,
                "steps": args.steps, "warmup": args.warmup})
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if out["update_below_recreate"] and out["bitwise_equal_to_recreated"] else 1


def narrow_child(args, torch, V):
    """One fresh process of --narrow: both updatable handles timed alternately, then the two narrow products."""
    import bench
    L, lib = V._lib, V._lib.lib()
    B = bench.build_matrix("fe", np.float32, args.scale)
    rng = np.random.default_rng(7)
    v2 = rng.uniform(-1, 1, len(B.val)).astype(np.float32)
    d2 = torch.from_numpy(v2).cuda()

    def make(narrow, updatable, val=None):
        M = V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, B.val if val is None else val)
        M.narrow, M.updatable = narrow, updatable
        return M, M.handle(0, True, compute=L.VBC_F64)
    (A, ha), (Nu, hb), (Nn, _) = make(False, True), make(True, "narrow"), make(True, False, v2)
    ia, ib, inn = (M.info(trans=True, compute=L.VBC_F64) for M in (A, Nu, Nn))
    assert ib["narrow_t"] and not ia["narrow_t"]
    s = torch.cuda.Stream()

    def update(h):
        return lambda: L.check(lib.vbc_update_values(h, d2.data_ptr(), len(v2), L.VBC_F32, L.VBC_MEM_DEVICE, s.cuda_stream))
    ta, tb = [], []
    for _ in range(2):  # alternately
        ta += graph_time_us(torch, s, update(ha), args.steps, args.warmup)[1]
        tb += graph_time_us(torch, s, update(hb), args.steps, args.warmup)[1]
    x = torch.from_numpy(rng.uniform(-1, 1, B.m)).cuda()
    y, y2 = (torch.empty(B.n, dtype=torch.float64, device="cuda") for _ in range(2))
    pu, pn = [], []
    for _ in range(2):
        pu += graph_time_us(torch, s, lambda: V.mul_(y, Nu.T, x), args.steps, args.warmup)[1]
        pn += graph_time_us(torch, s, lambda: V.mul_(y2, Nn.T, x), args.steps, args.warmup)[1]
    torch.cuda.synchronize()
    slots_b = (ib["device_bytes"] - inn["device_bytes"]) // 4  # the map's size (and the chunk table)
    print(json.dumps({"wide_updatable_us": round(float(np.median(ta)), 2), "wide_updatable_us_all": ta,
                      "narrow_updatable_us": round(float(np.median(tb)), 2), "narrow_updatable_us_all": tb,
                      "product_narrow_updatable_us": round(float(np.median(pu)), 2), "product_narrow_updatable_us_all": pu,
                      "product_narrow_us": round(float(np.median(pn)), 2), "product_narrow_us_all": pn,
                      "bitwise_equal_to_created": bool(torch.equal(y, y2)),
                      "m": B.m, "n": B.n, "nval": int(B.ofs[-1]) - 1, "value_slots_narrow": int(slots_b),
                      "device_bytes": {"wide_updatable": ia["device_bytes"], "narrow_updatable": ib["device_bytes"],
                                       "narrow": inn["device_bytes"]}}))
    return 0


def narrow_main(args):
    """--narrow: `--processes` fresh processes, one after the other, each timing both handles; this process only
    starts them and gathers their lines (it never opens the GPU)."""
    import subprocess
    runs = []
    for _ in range(args.processes):
        r = subprocess.run([sys.executable, __file__, "--narrow", "--child", "--scale", str(args.scale), "--steps",
                            str(args.steps), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            return 1
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))

    def summary(key):
        v = [p[key] for p in runs]
        return {"per_process_median_us": v, "median_us": round(float(np.median(v)), 2), "min_us": min(v), "max_us": max(v)}
    a, b = summary("wide_updatable_us"), summary("narrow_updatable_us")
    pu, pn = summary("product_narrow_updatable_us"), summary("product_narrow_us")
    gap = a["median_us"] - b["median_us"]
    out = {"tool": "update_time", "mode": "narrow", "workload": "fe", "scale": args.scale, "values": "float32",
           "compute": "float64", "product": "B'x", "processes": args.processes, "steps": args.steps, "warmup": args.warmup,
           "update_wide_updatable_0x20": a, "update_narrow_updatable_0x80_0x200": b, "gap_us": round(gap, 2),
           "wide_process_range_us": round(a["max_us"] - a["min_us"], 2),
           # (b) counts as faster only if the gap exceeds (a)'s own process-to-process range
           "narrow_update_faster": bool(gap > a["max_us"] - a["min_us"]),
           "bytes_per_slot_model": {"wide": 16, "narrow": 12},
           "product_narrow_updatable": pu, "product_narrow_not_updatable": pn,
           "product_ranges_overlap": bool(pu["min_us"] <= pn["max_us"] and pn["min_us"] <= pu["max_us"]),
           "bitwise_equal_to_created": all(p["bitwise_equal_to_created"] for p in runs), "runs": runs}
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if out["bitwise_equal_to_created"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--narrow", action="store_true",
                    help="FE-2D as float32 on Float64 handles: the wide updatable handle against the narrow-updatable one")
    ap.add_argument("--processes", type=int, default=3, help="--narrow: fresh processes, each timing both handles")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--workload", default="fe", choices=["fe", "ldoor"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shards", type=int, default=0, help="N > 0: the sharded handle on devices = [0] * N")
    ap.add_argument("--split", default="stripes", choices=["stripes", "rows"])
    args = ap.parse_args()
    if args.narrow and not args.child:
        return narrow_main(args)
    import torch

    import bench
    import sparsematrixvbcs_amd as V

    if args.narrow:
        return narrow_child(args, torch, V)

    B = bench.build_matrix(args.workload, np.float64, args.scale)
    if args.shards > 0:
        return sharded_main(args, torch, V, B)
    esz = B.val.dtype.itemsize
    rng = np.random.default_rng(7)
    v2 = rng.uniform(-1, 1, len(B.val))
    d2 = torch.from_numpy(v2).cuda()

    def plain():
        return V.SparseMatrix1DVBC(B.W, B.m, B.n, B.Phi, B.pos, B.idx, B.ofs, B.val)

    # (d) create, with and without the flag (one each: the host build dominates and is deterministic work)
    P = plain()
    create_plain, _ = wall_ms(torch, lambda: P.handle(0, True), 1)
    U = plain()
    U.updatable = True
    create_upd, _ = wall_ms(torch, lambda: U.handle(0, True), 1)
    inf_p, inf_u = P.info(), U.info()
    slots = (inf_u["device_bytes"] - inf_p["device_bytes"]) // 4
    traffic = slots * (2 * esz + 4)

    # (c) destroy + create with new values: what a caller without the flag has to do
    def recreate():
        P.release()
        P.val = v2
        P.handle(0, True)
    recreate_ms, recreate_all = wall_ms(torch, recreate, 2)

    s = torch.cuda.Stream()
    x = torch.from_numpy(rng.uniform(-1, 1, B.m)).cuda()
    y = torch.empty(B.n, dtype=torch.float64, device="cuda")
    h = U.handle(0, True)
    lib, L = V._lib.lib(), V._lib

    def update_dev():
        L.check(lib.vbc_update_values(h, d2.data_ptr(), len(v2), L.VBC_F64, L.VBC_MEM_DEVICE, s.cuda_stream))
    upd_us, upd_all = graph_time_us(torch, s, update_dev, args.steps, args.warmup)
    # (b) host val
    host_ms, host_all = wall_ms(torch, lambda: L.check(lib.vbc_update_values(h, v2.ctypes.data, len(v2), L.VBC_F64,
                                                                              L.VBC_MEM_HOST, None)), 3)
    prod_us, prod_all = graph_time_us(torch, s, lambda: V.mul_(y, U.T, x), args.steps, args.warmup)
    # the updated handle computes what the re-created one computes
    y2 = torch.empty_like(y)
    V.mul_(y2, P.T, x)
    V.mul_(y, U.T, x)
    torch.cuda.synchronize()
    out = {
        "tool": "update_time", "workload": args.workload, "scale": args.scale, "dtype": "float64",
        "m": B.m, "n": B.n, "nval": int(B.ofs[-1]) - 1, "value_slots": int(slots), "map_bytes": int(slots * 4),
        "arena_bytes": inf_p["device_bytes"],
        "update_device_us": round(upd_us, 2), "update_device_us_all": upd_all,
        "update_traffic_bytes": int(traffic), "update_frac_of_8TBs": round(traffic / (upd_us * 1e-6) / 8e12, 3),
        "update_host_ms": round(host_ms, 2), "update_host_ms_all": host_all,
        "recreate_ms": round(recreate_ms, 1), "recreate_ms_all": recreate_all,
        "create_ms": round(create_plain, 1), "create_updatable_ms": round(create_upd, 1),
        "product_us": round(prod_us, 2), "product_us_all": prod_all,
        "update_below_recreate": bool(upd_us * 1e-3 < recreate_ms),
        "bitwise_equal_to_recreated": bool(torch.equal(y, y2)),
        "steps": args.steps, "warmup": args.warmup,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0 if out["update_below_recreate"] and out["bitwise_equal_to_recreated"] else 1


if __name__ == "__main__":
    sys.exit(main())
