#!/usr/bin/env python3
"""A/B of csgpu_opts.lattice_maps for csgpu_components and csgpu_solve_rhs: connected components from the lattice form
(csrc/lattice_components.h, lattice_maps = 1) against the CSR path (lattice_maps = -1: ensure_csr + cc_hook_kernel of
csrc/raster.h, which is what every earlier build runs), and general right-hand sides with the lattice post-check against the
CSR one. Not a test: it measures and writes JSON.

  (default)  a `size`^2 fp64 raster with the bench's 15 % NODATA mask and an all-valid one; per setting a fresh handle, in the
             order 1, -1, -1, 1: the FIRST csgpu_components call (on the CSR path it includes the CSR build, which is what a
             user pays), then -- on the first handle of each setting -- one csgpu_solve_rhs of 16 columns
  --kernels  one handle per setting and raster, the components call only: the run to put under
             `rocprofv3 --kernel-trace --stats`; --merge-kernel-stats CSV then adds that run's per-kernel calls and times to the
             JSON: hook rounds = calls of the hook kernel, time per round against its algorithmic bytes
  --big N    an N x N raster (default 21000) with NODATA stripes that leave stripes + 1 components, DEFAULT options: asserts
             status 0, the count, no CSR form, and that a one-column csgpu_solve_rhs converges

Times: wall around the blocking call; the HIP-event time of the PCG loops for the solves (device_ms). csgpu_components returns
no statistics: its device time is the sum of its kernels in the --kernels run.
usage: ab_lattice_components.py [--size N] [--big [N]] [--kernels] [--merge-kernel-stats CSV] [--out FILE]
(env CSGPU_LIB: library to load)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import circuitscape_jl_amd  # noqa: E402,F401
from circuitscape_jl_amd import lib as L  # noqa: E402

LATTICE_KERNELS = ("dia_cc_hook_kernel",)
CSR_KERNELS = ("cc_hook_kernel", "dia_to_csr_kernel")
SHARED_KERNELS = ("cc_jump_kernel", "cc_root_flag_kernel", "cc_relabel_kernel")


def make_raster(size, seed=12345):  # bench.py's generator
    return 1.0 / np.exp(np.random.default_rng(seed).standard_normal((size, size)))


def nodata_raster(g, frac=0.15):  # bench.py's mask
    return np.where(np.random.default_rng(2468).random(g.shape) < frac, 0.0, g)


def rhs_columns(lab, ncols, seed=23):
    """zero-sum random columns supported inside the largest component"""
    rng = np.random.default_rng(seed)
    nodes = np.flatnonzero(lab == np.bincount(lab).argmax())
    B = np.zeros((len(lab), ncols), order="F")
    for c in range(ncols):
        v = rng.standard_normal(len(nodes))
        B[nodes, c] = v - v.mean()
    return B


def one_handle(g, setting, ncols, solve, rhs):
    """rhs: a list that keeps the right-hand sides drawn for the first solve for the later ones (the labels are equal)"""
    rec = {"lattice_maps": setting}
    t0 = time.perf_counter()
    with L.raster_setup(g, L.default_opts(batch=16, lattice_maps=setting)) as h:
        rec["setup_wall_s"] = time.perf_counter() - t0
        info = h.info
        rec.update(n=info["n"], rows=info["level_n"][0], nnz=info["level_nnz"][0], cellspace=info["cellspace"],
                   device_bytes_after_setup=info["device_bytes"])
        t0 = time.perf_counter()
        lab, cnt = h.components()
        rec["components_wall_ms"] = (time.perf_counter() - t0) * 1e3
        info = h.info
        rec.update(ncomponents=int(cnt), csr_built_after_components=info["csr_built"],
                   device_bytes_after_components=info["device_bytes"])
        x = None
        if solve:
            if not rhs:
                rhs.append(rhs_columns(lab, ncols))
            t0 = time.perf_counter()
            x, st = h.solve_rhs(rhs[0])
            rec["solve_rhs"] = {"columns": ncols, "wall_ms": (time.perf_counter() - t0) * 1e3, "solve_ms": st["solve_ms"],
                                "pcg_event_ms": st["device_ms"], "total_iters": st["total_iters"],
                                "not_converged": st["not_converged"], "max_relres": st["max_relres"],
                                "stats_lattice_maps": st["lattice_maps"], "csr_built": h.info["csr_built"],
                                "device_bytes": h.info["device_bytes"]}
    L.trim_memory()
    print(json.dumps(rec), flush=True)
    return rec, lab, x


def ab(g, ncols=16, orders=(1, -1, -1, 1), solve=True):
    runs, labs, xs, rhs = [], {}, {}, []
    for setting in orders:
        try:
            # (the solve once each way: its 16 columns of a 10000^2 raster are 12.8 GB up and as many down)
            rec, lab, x = one_handle(g, setting, ncols, solve and setting not in xs, rhs)
            labs.setdefault(setting, lab)
            if x is not None:
                xs[setting] = x
        except Exception as e:  # (out of device memory is a result here, not a crash)
            rec = {"lattice_maps": setting, "failed": repr(e)}
            print(json.dumps(rec), flush=True)
        runs.append(rec)
    out = {"runs": runs}
    if 1 in labs and -1 in labs:
        out["labels_equal_between_paths"] = bool(np.array_equal(labs[1], labs[-1]))
        if 1 in xs and -1 in xs:
            out["solutions_bit_equal_between_paths"] = bool(np.array_equal(xs[1], xs[-1]))
    wall = {s: [r["components_wall_ms"] for r in runs if r["lattice_maps"] == s and "components_wall_ms" in r] for s in (1, -1)}
    if wall[1] and wall[-1]:
        out["first_components_wall_ms"] = {"lattice": wall[1], "csr": wall[-1]}
        out["lattice_over_csr"] = float(np.mean(wall[1]) / np.mean(wall[-1]))
    return out


def striped_raster(size, stripes=2):
    """all ones but `stripes` full NODATA columns, evenly spaced: stripes + 1 components"""
    g = np.ones((size, size))
    for k in range(1, stripes + 1):
        g[:, k * size // (stripes + 1)] = 0.0
    return g


def case_big(size, stripes=2):
    g = striped_raster(size, stripes)
    t0 = time.perf_counter()
    with L.raster_setup(g, L.default_opts(batch=4)) as h:
        rec = {"size": size, "stripes": stripes, "setup_wall_s": time.perf_counter() - t0, "nnz": h.info["level_nnz"][0]}
        t0 = time.perf_counter()
        lab, cnt = h.components()
        rec.update(components_wall_ms=(time.perf_counter() - t0) * 1e3, ncomponents=int(cnt), csr_built=h.info["csr_built"],
                   component_sizes=[int(v) for v in np.bincount(lab)])
        print(json.dumps(rec), flush=True)
        lattice = rec["nnz"] >= 2 ** 31   # (default options: the lattice path exactly where no CSR form can exist)
        assert cnt == stripes + 1 and rec["csr_built"] == (0 if lattice else 1), rec
        x, st = h.solve_rhs(rhs_columns(lab, 1))
        rec["solve_rhs"] = {"columns": 1, "solve_ms": st["solve_ms"], "total_iters": st["total_iters"],
                            "not_converged": st["not_converged"], "max_relres": st["max_relres"],
                            "stats_lattice_maps": st["lattice_maps"], "csr_built": h.info["csr_built"]}
        print(json.dumps(rec), flush=True)
        assert st["not_converged"] == 0 and st["lattice_maps"] == (1 if lattice else 0), rec
    return rec


def merge_kernel_stats(doc, csv_path):
    import csv
    rows = {}
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for k in LATTICE_KERNELS + CSR_KERNELS + SHARED_KERNELS:
                if name.startswith("void csgpu::" + k + "<") or name.startswith("csgpu::" + k + "<") or name.startswith(k + "<") \
                        or name.startswith("csgpu::" + k + "(") or name.startswith(k + "("):
                    e = rows.setdefault(k, {"calls": 0, "total_ms": 0.0})
                    e["calls"] += int(r.get("Calls", 0))
                    e["total_ms"] += float(r.get("TotalDurationNs", 0)) / 1e6
    for e in rows.values():
        e["ms_per_call"] = e["total_ms"] / max(e["calls"], 1)
    doc["kernel_stats"] = {"source": "rocprofv3 --kernel-trace --stats over `--kernels` (one components call per setting and raster; "
                                     "hook rounds = calls of the hook kernel)", "kernels": rows}
    run = doc.get("kernels_run", {})
    n = run.get("rows")
    if n:
        # algorithmic bytes of one hooking round, fp64: the matrix once + f[i] and four neighbours' labels per row
        nnz = run.get("nnz", 9 * n)
        per_round = {"dia_cc_hook_kernel": n * 5 * 8 + n * 5 * 4, "cc_hook_kernel": nnz * (8 + 4) + (n + 1) * 4 + (nnz + n) * 4}
        for k, b in per_round.items():
            if k in rows:
                rows[k]["bytes_per_round"] = b
                rows[k]["gb_per_s"] = b / (rows[k]["ms_per_call"] * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--big", type=int, nargs="?", const=21000, default=0)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--merge-kernel-stats", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_components_ab.json"))
    args = ap.parse_args()
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    if args.merge_kernel_stats:
        merge_kernel_stats(doc, args.merge_kernel_stats)
    else:
        L.load(os.environ.get("CSGPU_LIB"))
        if args.big:
            doc["big_default_options"] = case_big(args.big)
        elif args.kernels:
            g = nodata_raster(make_raster(args.size))
            res = ab(g, orders=(1, -1), solve=False)
            doc["kernels_run"] = {"size": args.size, "nodata_fraction": 0.15, "rows": res["runs"][0].get("rows"),
                                  "nnz": res["runs"][0].get("nnz"), **res}
        else:
            g = make_raster(args.size)
            doc["nodata15_fp64"] = {"size": args.size, "nodata_fraction": 0.15, **ab(nodata_raster(g))}
            doc["allvalid_fp64"] = {"size": args.size, "nodata_fraction": 0.0, **ab(g)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
