"""How the multi-device calls merge their csgpu_stats (csrc/csgpu.hip, DESIGN.md section 6, "Multi-GPU"): the
checks shared by test_multi_stats_emu.py and test_multi_stats_gpu.py. `L` is circuitscape_jl_amd.lib with a library loaded.

The shapes are the smallest at which a merge rule can go wrong: 21 pairs at batch 4 are five full chunks and a ragged chunk of
one pair that runs at K = 1, whose cg_spmv_bytes differ from the full chunks' ("last value wins" is then visible next to "max")."""
import numpy as np

BATCH = 4
SUMS = ("total_iters", "not_converged", "cg_spmv_calls", "graph_launches", "polished_batches", "resid_calls", "stream_slots")
MAXES = ("max_iters", "max_relres", "batch", "lattice_maps")
LAST = ("cg_spmv_bytes", "resid_bytes", "resid_fused")   # within a device; the maximum across devices
TIMES = ("solve_ms", "device_ms", "cg_spmv_ms", "resid_ms")


def problem():
    """The raster and the 21 pairs of 7 cells of test_multi_device_handle_matches_single_device."""
    N = 40
    g = np.exp(np.random.default_rng(5).standard_normal((N, N + 3)))
    cells = np.random.default_rng(6).choice(N * (N + 3), size=7, replace=False)
    src = [int(cells[i]) for i in range(7) for j in range(i + 1, 7)]
    dst = [int(cells[j]) for i in range(7) for j in range(i + 1, 7)]
    return g, cells, src, dst


def merge_chunks(stats):
    """Sequential calls on one device merged by the rules of the library."""
    out = {k: sum(s[k] for s in stats) for k in SUMS}
    out.update({k: max(s[k] for s in stats) for k in MAXES})
    out.update({k: stats[-1][k] for k in LAST})
    return out


def check_chunk_merge(L):
    """csgpu_multi_solve_pairs on one device == one csgpu_solve_pairs call per chunk, the stats merged by the rules."""
    g, _, src, dst = problem()
    with L.raster_setup(g, L.default_opts(batch=BATCH)) as h:
        chunks = [h.solve_pairs(src[o:o + BATCH], dst[o:o + BATCH]) for o in range(0, len(src), BATCH)]
    per_chunk = [c[3] for c in chunks]
    assert [s["batch"] for s in per_chunk] == [4, 4, 4, 4, 4, 1]
    assert per_chunk[-1]["cg_spmv_bytes"] != per_chunk[0]["cg_spmv_bytes"]   # (or "last wins" could not be told from "max")
    want = merge_chunks(per_chunk)
    with L.multi_raster_setup(g, L.default_opts(batch=BATCH), devices=[0]) as m:
        R, _, got = m.solve_pairs(src, dst)
    assert got["nrhs"] == 21 and got["stream_slots"] == 0 and got["device_pairs"] == [21]
    for k in SUMS + MAXES + LAST:
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(R, np.concatenate([c[0] for c in chunks]))


def _same_stats(a, b):
    for k in a:
        if k not in TIMES:
            assert a[k] == b[k], (k, a[k], b[k])


def check_pass_through(L):
    """The map calls on one device are ONE call on one handle: every stats field but the times, the resistances / check
    voltages and the cumulative / maximum maps (in/out: both start from cum = 0.5, mx = 0.01) equal the plain handle's."""
    g, cells, src, dst = problem()
    n = g.size
    w = (1 + np.arange(len(src)) % 3).astype(np.int32)
    pts = [int(c) for c in cells[:5]]
    sources = [[p] for p in pts]
    grounds = [[q for q in pts if q != p] for p in pts]
    with L.raster_setup(g, L.default_opts(batch=BATCH)) as h:
        cum1, mx1 = np.full(n, 0.5), np.full(n, 0.01)
        R1, _, _, st1 = h.solve_pairs_currents(src, dst, weights=w, want_currents=False, cum=cum1, mx=mx1)
        scum1, smx1 = np.full(n, 0.5), np.full(n, 0.01)
        v1, _, _, sst1 = h.solve_sources(sources, grounds, check=pts, cum=scum1, mx=smx1)
    with L.multi_raster_setup(g, L.default_opts(batch=BATCH), devices=[0]) as m:
        cumm, mxm = np.full(n, 0.5), np.full(n, 0.01)
        Rm, stm = m.solve_pairs_currents(src, dst, weights=w, cum=cumm, mx=mxm)
        scumm, smxm = np.full(n, 0.5), np.full(n, 0.01)
        vm, _, _, sstm = m.solve_sources(sources, grounds, check=pts, cum=scumm, mx=smxm)
    assert st1["nrhs"] == 21 and stm["device_pairs"] == [21] and sst1["nrhs"] == 5 and sstm["device_pairs"] == [5]
    _same_stats(st1, stm)
    _same_stats(sst1, sstm)
    assert np.array_equal(R1, Rm) and np.array_equal(cum1, cumm) and np.array_equal(mx1, mxm)
    assert np.array_equal(v1, vm) and np.array_equal(scum1, scumm) and np.array_equal(smx1, smxm)
    assert np.max(cum1) > 0.5 and np.max(scum1) > 0.5   # (the maps were written at all)


def check_stream_slots_are_carried(L):
    """A csgpu_multi_solve_pairs_currents call without either map is a plain resistance call per device and may stream (here:
    csgpu_opts.stream = 1 and stream_min = 1, 21 pairs at batch 8): the slots of the stream are reported, as the plain handle
    reports them. (Before merge_stats the multi call dropped them and reported 0.)"""
    g, _, src, dst = problem()
    with L.raster_setup(g, L.default_opts(batch=8, stream=1, stream_min=1)) as h:
        R1, _, _, st1 = h.solve_pairs_currents(src, dst, want_currents=False)
    with L.multi_raster_setup(g, L.default_opts(batch=8, stream=1, stream_min=1), devices=[0]) as m:
        Rm, stm = m.solve_pairs_currents(src, dst)
    assert st1["stream_slots"] > 0 and stm["stream_slots"] == st1["stream_slots"], (st1["stream_slots"], stm["stream_slots"])
    _same_stats(st1, stm)
    assert np.array_equal(R1, Rm)


def check_error_precedence(L):
    """A pair with src == n in one chunk of a three-device call: the call returns CSGPU_BAD_ARGS with the failing device named,
    every chunk was dealt, and the chunks of the other devices came back solved."""
    import ctypes
    assert L.device_count() == 3
    g, _, src, dst = problem()
    bad = list(src)
    bad[9] = g.size                                    # chunk 2 = pairs 8..11
    with L.raster_setup(g, L.default_opts(batch=BATCH)) as h:
        want = np.concatenate([h.solve_pairs(src[o:o + BATCH], dst[o:o + BATCH])[0] for o in range(0, len(src), BATCH)])
    with L.multi_raster_setup(g, L.default_opts(batch=BATCH)) as m:
        s = np.ascontiguousarray(bad, dtype=np.int64)
        d = np.ascontiguousarray(dst, dtype=np.int64)
        res = np.zeros(len(bad))
        st = L.Stats()
        rc = L.lib().csgpu_multi_solve_pairs(m._p, s.ctypes.data, d.ctypes.data, len(bad), None, 0, None, res.ctypes.data,
                                             ctypes.byref(st))
        msg = L.lib().csgpu_last_error().decode()
        done = L._multi_busy(m, st)["device_pairs"]
    assert rc == 4, rc                                 # CSGPU_BAD_ARGS
    assert msg.startswith("device ") and "pair node id out of range" in msg, msg
    # the failing device stops after its chunk; the two others drain the queue
    assert sum(done) == 21 and st.nrhs == 21, done
    ok = np.ones(21, dtype=bool)
    ok[8:12] = False
    assert np.array_equal(res[ok], want[ok])
    assert np.all(res[~ok] == 0.0)
