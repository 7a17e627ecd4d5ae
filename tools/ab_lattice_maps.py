#!/usr/bin/env python3
"""A/B of csgpu_opts.lattice_maps: cumulative / maximum current maps of pair solves from the lattice form
(csrc/lattice_currents.h, lattice_maps = 1) against the CSR path (lattice_maps = -1: ensure_csr + the three kernels of
csrc/currents.h, which is what every earlier build runs). Not a test: it measures and writes JSON.

  --case a   10000^2 fp64 bench raster, batch 32, 32 pairs: cumulative + maximum map only, then again with curr_out
  --case b   the same on the bench's 15 % NODATA mask
  --case c   21000^2, batch 4, 4 pairs, cumulative map at DEFAULT options (asserts: converged, lattice path, no CSR form, node
             current 1 at the terminals to 1e-4 sqrt(n) -- read from the maximum map, which the call fills as well -- and
             currents >= 0)
  --kernels  one handle per setting, two maps-only calls each and nothing else: the run to put under
             `rocprofv3 --kernel-trace --stats`; --merge-kernel-stats CSV then adds that run's per-kernel times to the JSON

Per setting a handle of its own, two rounds in the order 1, -1, -1, 1; per handle the first call (which builds the CSR form on
the CSR path) and a warm repeat. Times: wall around the blocking call, the library's own wall (solve_ms) and the HIP-event
time of the PCG loops (device_ms). Device memory: csgpu_info.device_bytes after the call and the largest used-memory
figure hipMemGetInfo gave while the call ran (sampled every 5 ms; the library's pool keeps what it freed, so the figure
after the call is the high-water mark as well).
usage: ab_lattice_maps.py [--case a,b,c] [--size N] [--big N] [--out FILE]   (env CSGPU_LIB: library to load)"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import circuitscape_jl_amd  # noqa: E402,F401
from circuitscape_jl_amd import lib as L  # noqa: E402

NEW_KERNELS = ("dia_branch_max_kernel", "dia_node_current_kernel")
CSR_KERNELS = ("branch_max_kernel", "node_current_kernel", "current_accumulate_kernel", "dia_to_csr_kernel")


def make_raster(size, seed=12345):  # bench.py's generator
    return 1.0 / np.exp(np.random.default_rng(seed).standard_normal((size, size)))


def nodata_raster(g, frac=0.15):  # bench.py's mask
    return np.where(np.random.default_rng(2468).random(g.shape) < frac, 0.0, g)


def giant_component_nodes(g):
    """node ids (column-major over the valid cells, src/raster/pairwise.jl:271-301) of the largest 8-connected component"""
    from scipy import ndimage
    lab, _ = ndimage.label(g > 0, structure=np.ones((3, 3), dtype=int))
    big = lab == np.bincount(lab[lab > 0]).argmax()
    valid_cm = (g > 0).T.ravel()
    node_of_cell = np.cumsum(valid_cm) - 1
    return node_of_cell[np.flatnonzero(big.T.ravel())]


class MemSampler:
    def __init__(self):
        self.hip = None
        for name in ("libamdhip64.so", "libamdhip64.so.6", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
            try:
                self.hip = ctypes.CDLL(name)
                break
            except OSError:
                pass

    def used(self):
        if self.hip is None:
            return -1
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if self.hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
            return -1
        return total.value - free.value

    def during(self, fn):
        peak, stop = [self.used()], threading.Event()

        def poll():
            while not stop.is_set():
                peak[0] = max(peak[0], self.used())
                time.sleep(0.005)
        t = threading.Thread(target=poll, daemon=True)
        t.start()
        try:
            out = fn()
        finally:
            stop.set()
            t.join()
        peak[0] = max(peak[0], self.used())
        return out, peak[0]


MEM = MemSampler()


def timed_call(h, src, dst, n, curr_out, label):
    cum, mx = np.zeros(n), np.zeros(n)
    t0 = time.perf_counter()
    (R, _, C, st), peak = MEM.during(lambda: h.solve_pairs_currents(src, dst, want_currents=curr_out, cum=cum, mx=mx))
    wall = (time.perf_counter() - t0) * 1e3
    info = h.info
    rec = {"call": label, "wall_ms": wall, "solve_ms": st["solve_ms"], "pcg_event_ms": st["device_ms"],
           "outside_pcg_ms": st["solve_ms"] - st["device_ms"],  # right-hand sides, post-processing (the kernels compared), copies
           "total_iters": st["total_iters"], "not_converged": st["not_converged"], "max_relres": st["max_relres"],
           "stats_lattice_maps": st["lattice_maps"], "csr_built": info["csr_built"], "device_bytes": info["device_bytes"],
           "peak_used_bytes": peak, "cum_sum": float(cum.sum()), "mx_max": float(mx.max())}
    del C
    return rec, cum, mx


def ab(g, batch, npairs, pool, curr_out, orders=(1, -1, -1, 1), calls=("first", "warm")):
    ids = np.random.default_rng(5).choice(pool, size=2 * npairs, replace=False)
    src, dst = [int(v) for v in ids[:npairs]], [int(v) for v in ids[npairs:]]
    runs, maps = [], {}
    for setting in orders:
        rec = {"lattice_maps": setting, "curr_out": bool(curr_out)}
        try:
            t0 = time.perf_counter()
            with L.raster_setup(g, L.default_opts(batch=batch, lattice_maps=setting)) as h:
                rec["setup_wall_s"] = time.perf_counter() - t0
                n = h.info["n"]
                rec["device_bytes_after_setup"] = h.info["device_bytes"]
                rec["calls"] = []
                for label in calls:
                    c, cum, mx = timed_call(h, src, dst, n, curr_out, label)
                    rec["calls"].append(c)
                if setting in maps:
                    rec["equal_to_first_round"] = bool(np.array_equal(maps[setting][0], cum) and np.array_equal(maps[setting][1], mx))
                maps.setdefault(setting, (cum, mx))
        except Exception as e:  # (out of device memory is a result here, not a crash)
            rec["failed"] = repr(e)
        L.trim_memory() if hasattr(L, "trim_memory") else None
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    out = {"runs": runs}
    if 1 in maps and -1 in maps:
        out["maps_bit_equal_between_paths"] = bool(np.array_equal(maps[1][0], maps[-1][0]) and np.array_equal(maps[1][1], maps[-1][1]))
    rest = {s: [c["outside_pcg_ms"] for r in runs if r["lattice_maps"] == s and "calls" in r for c in r["calls"] if c["call"] == "warm"]
            for s in (1, -1)}
    if rest[1] and rest[-1]:
        out["warm_outside_pcg_ms"] = {"lattice": rest[1], "csr": rest[-1]}
    warm = {s: [c["wall_ms"] for r in runs if r["lattice_maps"] == s and "calls" in r for c in r["calls"] if c["call"] == "warm"]
            for s in (1, -1)}
    if warm[1] and warm[-1]:
        out["warm_wall_ms"] = {"lattice": warm[1], "csr": warm[-1]}
        out["warm_lattice_over_csr"] = float(np.mean(warm[1]) / np.mean(warm[-1]))
        out["verdict"] = "lattice path faster warm" if out["warm_lattice_over_csr"] < 1.0 else "lattice path SLOWER warm"
    return out


def case_ab(size, nodata):
    g = make_raster(size)
    if nodata:
        g = nodata_raster(g)
        pool = giant_component_nodes(g)
    else:
        pool = np.arange(size * size)
    return {"size": size, "nodata_fraction": 0.15 if nodata else 0.0, "batch": 32, "pairs": 32,
            "maps_only": ab(g, 32, 32, pool, False), "with_curr_out": ab(g, 32, 32, pool, True, orders=(1, -1))}


def case_c(size):
    """the first cumulative current map at this size: default options, no CSR form can exist (nnz >= 2^31)"""
    g = make_raster(size)
    n = size * size
    ids = np.random.default_rng(5).choice(n, size=8, replace=False)
    src, dst = [int(v) for v in ids[:4]], [int(v) for v in ids[4:]]
    t0 = time.perf_counter()
    with L.raster_setup(g, L.default_opts(batch=4)) as h:
        setup_s = time.perf_counter() - t0
        nnz = h.info["nnz"]
        rec, cum, mx = timed_call(h, src, dst, n, False, "first")
        # per-pair terminals: one more call per pair would double the time; the maximum map holds max_p curr_p, and a terminal's
        # own pair gives 1 there while no other pair's current through that node exceeds the unit current it injects
        bound = 1e-4 * np.sqrt(n)
        term = [float(mx[q]) for q in src + dst]
        rec.update(size=size, nnz=nnz, setup_wall_s=setup_s, terminal_currents=term, terminal_bound=bound,
                   cum_min=float(cum.min()), mx_min=float(mx.min()))
        print(json.dumps(rec), flush=True)
        assert rec["not_converged"] == 0, rec
        assert rec["stats_lattice_maps"] == 1 and rec["csr_built"] == 0, rec
        assert all(abs(t - 1.0) <= bound for t in term), (term, bound)
        assert rec["cum_min"] >= 0.0 and rec["mx_min"] >= 0.0
    return rec


def kernels_run(size, nodata):
    g = make_raster(size)
    pool = giant_component_nodes(nodata_raster(g)) if nodata else np.arange(size * size)
    if nodata:
        g = nodata_raster(g)
    return ab(g, 32, 32, pool, False, orders=(1, -1), calls=("first", "warm"))


def merge_kernel_stats(doc, csv_path):
    import csv
    rows = {}
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for k in NEW_KERNELS + CSR_KERNELS:
                if name.startswith("void csgpu::" + k + "<") or name.startswith("csgpu::" + k + "<") or name.startswith(k + "<"):
                    e = rows.setdefault(k, {"calls": 0, "total_ms": 0.0})
                    e["calls"] += int(r.get("Calls", 0))
                    e["total_ms"] += float(r.get("TotalDurationNs", 0)) / 1e6
    for e in rows.values():
        e["ms_per_call"] = e["total_ms"] / max(e["calls"], 1)
    doc["kernel_stats"] = {"source": "rocprofv3 --kernel-trace --stats over `--kernels` (2 maps-only calls per setting)", "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="a,b,c")
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--big", type=int, default=21000)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--merge-kernel-stats", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_maps_ab.json"))
    args = ap.parse_args()
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    if args.merge_kernel_stats:
        merge_kernel_stats(doc, args.merge_kernel_stats)
    else:
        L.load(os.environ.get("CSGPU_LIB"))
        if args.kernels:
            doc["kernels_run"] = kernels_run(args.size, False)
        else:
            for c in args.case.split(","):
                if c == "a":
                    doc["a_10000_fp64_batch32"] = case_ab(args.size, False)
                elif c == "b":
                    doc["b_10000_fp64_batch32_nodata15"] = case_ab(args.size, True)
                elif c == "c":
                    doc["c_21000_batch4_default_options"] = case_c(args.big)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
