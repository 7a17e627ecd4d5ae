#!/usr/bin/env python3
"""A/B of the fused residual update + restriction for solves that CARRY the solution (csgpu_opts.fused_restrict = 1 against
-1; csrc/lattice.h, the XUP form of lattice_rupd_restrict_kernel). Workload: the reference's main product -- cumulative and
maximum current maps of a list of pairs (csgpu_solve_pairs_currents with cum / mx, no n x npairs array crosses the
boundary) -- on a square all-valid raster in double precision, at batch 32 and 16.

Size: the largest square raster (a multiple of 500 cells a side) whose work arena at batch 32 WITH the second residual
buffer fits the device: r, r2 (both with the level-1 tail), p, p2, z, x, b, A p, the node currents, the CSR and lattice
forms of the matrix and the hierarchy -- about (9.3 * 8 * 32 + 350) bytes per cell, against 85 % of the free memory.
The same size is used at batch 16. One handle is resident at a time (two arenas of that size do not fit): the variants
alternate -1, 1, -1, 1, ... -- each visit builds its handle, runs one warm-up call and then `--calls` timed calls of
`--batches` full batches each -- so that drift of the shared box hits both alike; the spread of a variant over its visits
is the run-to-run figure a difference has to beat.

Per variant and batch width: device ms per batch (median and min - max over all timed calls), resid_ms / resid_calls and
cg_spmv_ms / cg_spmv_calls (HIP events of the library, csgpu_stats), iterations, device_bytes with the arena in place,
whether the fused pass ran (resid_fused, fused_restrict_solves), and a bit-for-bit comparison of the maps of the two
variants. One JSON document on stdout and in --out.

    ab_fused_solution.py [--size N] [--visits 3] [--calls 2] [--batches 2] [--widths 32,16] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import circuitscape_jl_amd  # noqa: F401,E402
from circuitscape_jl_amd import lib  # noqa: E402

BYTES_PER_CELL_K32 = 9.3 * 8 * 32 + 350


def pick_size(free_bytes):
    side = int(np.sqrt(0.85 * free_bytes / BYTES_PER_CELL_K32))
    return max(500, side // 500 * 500)


def spread(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--visits", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--widths", default="32,16")
    ap.add_argument("--out", default="")
    ap.add_argument("--lib", default=os.environ.get("CSGPU_LIB"))
    args = ap.parse_args()
    lib.load(args.lib)
    assert lib.device_count() >= 1, "no HIP device visible"   # (no fallback: a timing needs the device)
    size = args.size
    if size <= 0:
        import torch
        free, total = torch.cuda.mem_get_info(0)
        size = pick_size(free)
    rng = np.random.default_rng(20240)
    g = np.exp(0.5 * rng.standard_normal((size, size)))
    n = size * size
    doc = {"workload": "csgpu_solve_pairs_currents, cum + mx, fp64, %d x %d raster" % (size, size), "size": size,
           "visits": args.visits, "calls_per_visit": args.calls, "batches_per_call": args.batches, "results": []}
    for width in [int(w) for w in args.widths.split(",")]:
        npairs = width * args.batches
        cells = rng.choice(n, size=2 * npairs, replace=False)
        src, dst = [int(c) for c in cells[:npairs]], [int(c) for c in cells[npairs:]]
        rec = {m: {"ms_per_batch": [], "resid_ms": [], "spmv_ms": [], "iters": [], "device_bytes": 0, "resid_fused": 0,
                   "fused_restrict_solves": 0, "resid_bytes": 0} for m in (-1, 1)}
        maps = {}
        for visit in range(args.visits):
            for m in (-1, 1):
                with lib.raster_setup(g, lib.default_opts(batch=width, precond_bytes=0, fixed_k=1, stream=-1,
                                                          fused_restrict=m)) as h:
                    cum, mx = np.zeros(n), np.zeros(n)
                    h.solve_pairs_currents(src, dst, want_currents=False, cum=cum, mx=mx)   # warm-up (arena, code objects)
                    if visit == 0:
                        maps[m] = (cum.copy(), mx.copy())
                    for _ in range(args.calls):
                        R, _, _, st = h.solve_pairs_currents(src, dst, want_currents=False, cum=cum, mx=mx)
                        assert st["not_converged"] == 0
                        r = rec[m]
                        r["ms_per_batch"].append(st["device_ms"] / args.batches)
                        r["resid_ms"].append(st["resid_ms"] / max(st["resid_calls"], 1))
                        r["spmv_ms"].append(st["cg_spmv_ms"] / max(st["cg_spmv_calls"], 1))
                        r["iters"].append(st["total_iters"] / npairs)
                        r["resid_fused"], r["resid_bytes"] = st["resid_fused"], st["resid_bytes"]
                    info = h.info
                    rec[m]["device_bytes"] = info["device_bytes"]
                    rec[m]["fused_restrict_solves"] = info["fused_restrict_solves"]
        assert rec[1]["resid_fused"] == 1 and rec[-1]["resid_fused"] == 0, "the variants did not take their paths"
        two, fused = spread(rec[-1]["ms_per_batch"]), spread(rec[1]["ms_per_batch"])
        out = {"batch": width, "npairs_per_call": npairs,
               "maps_bit_identical": bool(np.array_equal(maps[1][0], maps[-1][0]) and np.array_equal(maps[1][1], maps[-1][1])),
               "gain_percent_of_median": 100.0 * (two["median"] - fused["median"]) / two["median"]}
        for m, name in ((-1, "two_pass"), (1, "fused")):
            r = rec[m]
            out[name] = {"ms_per_batch": spread(r["ms_per_batch"]), "resid_ms_per_launch": spread(r["resid_ms"]),
                         "cg_spmv_ms_per_launch": spread(r["spmv_ms"]), "iterations_per_pair": spread(r["iters"]),
                         "device_bytes": r["device_bytes"], "resid_fused": r["resid_fused"], "resid_bytes": r["resid_bytes"],
                         "fused_restrict_solves": r["fused_restrict_solves"]}
        doc["results"].append(out)
        print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
