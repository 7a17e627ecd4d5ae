"""Checks of csgpu_opts.lattice_maps: voltage maps, node currents, cumulative / maximum maps and the explicit residual check
of pair solves computed from the lattice form (csrc/lattice_currents.h: dia_branch_max_kernel, dia_node_current_kernel; the
post-check of csrc/pcg.h through dia_apply) without a CSR form of the fine-level matrix. Shared by the emulator tests
(test_lattice_maps_emu.py) and their device twins (test_lattice_maps_gpu.py).

The lattice kernels give every entry the arithmetic of the CSR kernels of csrc/currents.h on the CSR form the handle would
build from the same lattice form, so everything a call returns must be EQUAL, bit for bit, whichever path runs -- except
max_relres, whose residual b - A x is summed in another order."""
import numpy as np

# (raster shape, dia_seg or 0 for the default). A workgroup of the kernels owns TI rows of `dia_seg` raster columns:
# TI = 256 at batch 1; 16 (fp64) / 32 (fp32) at batch 32.
SHAPES = {
    "tall": ((261, 70), 16),   # more than one strip at every width, rows no multiple of any TI; segments 16,16,16,16,6
    "small": ((40, 45), 0),    # smaller than one tile both ways
    "wide": ((70, 261), 16),   # wide: 17 segments, the last one partial
}


def raster(shape, dtype=np.float64, nodata=False, seed=3):
    rng = np.random.default_rng(seed)
    g = np.exp(rng.standard_normal(shape))
    if nodata:
        g[rng.random(shape) < 0.15] = 0.0
    return g.astype(dtype)


def pair_list(pts, npairs, seed):
    rng = np.random.default_rng(seed)
    src = [pts[int(i)] for i in rng.integers(0, len(pts), npairs)]
    dst = [pts[(pts.index(s) + 1 + int(k)) % len(pts)] for s, k in zip(src, rng.integers(0, len(pts) - 1, npairs))]
    return src, dst


def opts(L, batch, maps, seg=0, **kw):
    kw.update(batch=batch, lattice_maps=maps)
    if seg:
        kw["dia_seg"] = seg
    return L.default_opts(**kw)


def focal_nodes(L, g, batch, seg, raster_kw, nodata, npts=10, seed=11):
    """Node ids (the caller's compact numbering) to take pairs from; on a NODATA raster all inside the largest component, read
    from a lattice_maps = -1 handle (components() walks the CSR form and would build it on the handle under test)."""
    rng = np.random.default_rng(seed)
    if not nodata:
        return [int(q) for q in rng.choice(g.size, size=npts, replace=False)]
    with L.raster_setup(g, opts(L, batch, -1, seg), **raster_kw) as h:
        assert h.info["cellspace"] == 1
        lab, _ = h.components()
    big = np.flatnonzero(lab == np.bincount(lab).argmax())
    return [int(q) for q in rng.choice(big, size=npts, replace=False)]


def maps_call(L, g, o, src, dst, weights, raster_kw, want_currents=True, want_voltages=True):
    """One handle, one csgpu_solve_pairs_currents with cum / mx preloaded with non-zero values."""
    with L.raster_setup(g, o, **raster_kw) as h:
        n = h.info["n"]
        pre = np.random.default_rng(29)
        cum = (0.25 + pre.random(n)).astype(g.dtype)
        mx = (0.05 * pre.random(n)).astype(g.dtype)
        before = h.info
        R, V, C, st = h.solve_pairs_currents(src, dst, weights=weights, want_voltages=want_voltages,
                                             want_currents=want_currents, cum=cum, mx=mx)
        after = h.info
    assert st["not_converged"] == 0
    return dict(R=R, V=V, C=C, cum=cum, mx=mx, st=st, before=before, after=after)


def check_equals_csr_path(L, name, batch, dtype=np.float64, precond_bytes=0, nodata=False, maps_only_too=False, **raster_kw):
    """Check 1: batch + 3 pairs (a full batch, then a short one at a narrower width) with lattice_maps = 1 and -1."""
    shape, seg = SHAPES[name]
    g = raster(shape, dtype, nodata)
    pts = focal_nodes(L, g, batch, seg, raster_kw, nodata)
    src, dst = pair_list(pts, batch + 3, seed=5)
    weights = [int(w) for w in np.random.default_rng(7).integers(0, 3, batch + 3)]
    got = maps_call(L, g, opts(L, batch, 1, seg, precond_bytes=precond_bytes), src, dst, weights, raster_kw)
    ref = maps_call(L, g, opts(L, batch, -1, seg, precond_bytes=precond_bytes), src, dst, weights, raster_kw)
    tag = (name, batch, np.dtype(dtype).name, precond_bytes, nodata, raster_kw)
    if nodata:
        assert got["after"]["cellspace"] == 1 and ref["after"]["cellspace"] == 1
    for key in ("R", "V", "C", "cum", "mx"):
        assert np.array_equal(got[key], ref[key]), (tag, key, float(np.max(np.abs(got[key] - ref[key]))))
    assert got["st"]["total_iters"] == ref["st"]["total_iters"], tag
    assert got["st"]["lattice_maps"] == 1 and ref["st"]["lattice_maps"] == 0, tag
    assert got["st"]["max_relres"] < 1e-4 and ref["st"]["max_relres"] < 1e-4, tag
    if dtype == np.float64:
        # two evaluations of one residual (test_recurrence_residual_post_check_at_size uses the same figure)
        a, b = got["st"]["max_relres"], ref["st"]["max_relres"]
        assert abs(a - b) <= 1e-3 * max(a, b), (tag, a, b)
    assert np.any(got["cum"] != got["cum"][0]) and np.all(got["C"] >= 0)
    if maps_only_too:
        # cumulative / maximum map only: the currents are accumulated inside the kernel and never stored
        only = maps_call(L, g, opts(L, batch, 1, seg, precond_bytes=precond_bytes), src, dst, weights, raster_kw,
                         want_currents=False, want_voltages=False)
        assert only["C"] is None and only["st"]["lattice_maps"] == 1
        assert np.array_equal(only["cum"], got["cum"]), (tag, float(np.max(np.abs(only["cum"] - got["cum"]))))
        assert np.array_equal(only["mx"], got["mx"]), tag
        assert np.array_equal(only["R"], got["R"]), tag


def csr_bytes(info, val_bytes):
    """rowptr + colidx + vals of the device matrix of level 0"""
    n, nnz = info["level_n"][0], info["level_nnz"][0]
    return (n + 1) * 4 + nnz * (4 + val_bytes)


def check_no_csr_form(L, batch=4, name="tall"):
    """Check 2. csgpu_info.device_bytes counts the work vectors a handle allocates at its first solve, so "unchanged" is
    asserted (i) between the first and a second maps call of the lattice handle and (ii) against the lattice_maps = -1
    handle after the same call, which must hold exactly the three CSR arrays more."""
    shape, seg = SHAPES[name]
    g = raster(shape)
    pts = focal_nodes(L, g, batch, seg, {}, False)
    src, dst = pair_list(pts, batch + 3, seed=5)
    got = maps_call(L, g, opts(L, batch, 1, seg), src, dst, None, {})
    ref = maps_call(L, g, opts(L, batch, -1, seg), src, dst, None, {})
    assert got["before"]["csr_built"] == 0 and ref["before"]["csr_built"] == 0
    assert got["after"]["csr_built"] == 0 and got["st"]["lattice_maps"] == 1
    assert ref["after"]["csr_built"] == 1 and ref["st"]["lattice_maps"] == 0
    assert got["before"]["device_bytes"] == ref["before"]["device_bytes"]
    assert ref["after"]["device_bytes"] - got["after"]["device_bytes"] == csr_bytes(ref["after"], 8), \
        (ref["after"]["device_bytes"], got["after"]["device_bytes"], csr_bytes(ref["after"], 8))
    with L.raster_setup(g, opts(L, batch, 1, seg)) as h:
        n = h.info["n"]
        cum = np.zeros(n)
        h.solve_pairs_currents(src, dst, want_currents=False, cum=cum)
        first = h.info
        h.solve_pairs_currents(src, dst, want_voltages=True, cum=cum)
        second = h.info
    assert first["csr_built"] == 0 and second["csr_built"] == 0
    assert first["device_bytes"] == second["device_bytes"] == got["after"]["device_bytes"]
    # explicit_check = 1 on a resistance-only call: the whole solution is carried and checked, still no CSR form
    res = {}
    for maps in (1, -1):
        with L.raster_setup(g, opts(L, batch, maps, seg, explicit_check=1)) as h:
            R, _, _, st = h.solve_pairs(src, dst)
            res[maps] = (R, st, h.info["csr_built"])
        assert st["not_converged"] == 0
    assert res[1][2] == 0 and res[-1][2] == 1
    assert res[1][1]["lattice_maps"] == 1 and res[-1][1]["lattice_maps"] == 0
    assert np.array_equal(res[1][0], res[-1][0]) and np.array_equal(res[1][0], got["R"])
    # branch currents are indexed by the stored entries of the CSR matrix: that call takes the CSR path whatever the option
    out = {}
    for maps in (1, -1):
        with L.raster_setup(g, opts(L, batch, maps, seg)) as h:
            R, V, C, st, B = h.solve_pairs_currents(src, dst, want_voltages=True, want_branch=True)
            out[maps] = (R, V, C, B, st, h.info["csr_built"])
    assert out[1][5] == 1 and out[1][4]["lattice_maps"] == 0
    for k in range(4):
        assert np.array_equal(out[1][k], out[-1][k]), k
    assert np.array_equal(out[1][2], got["C"])


def reference_node_currents(G, v):
    """Node currents of one pair from its voltages and the host Laplacian G (scipy CSR), by the rule of src/out.jl:178-290 as
    csrc/currents.h states it. Returns (currents, largest |branch current|)."""
    import scipy.sparse as sp
    U = sp.triu(G, k=1).tocoo()
    i, j, gabs = U.row, U.col, np.abs(U.data)
    b = gabs * (v[i] - v[j])
    mpos, mneg = b.max(), (-b).max()
    with np.errstate(divide="ignore", invalid="ignore"):
        bp = np.where(np.abs(b / mpos) < 1e-8, 0.0, b)    # entries of B  (pos orientation)
        bn = np.where(np.abs(-b / mneg) < 1e-8, 0.0, -b)  # entries of B' (neg orientation)
    n = G.shape[0]
    cin, cout = np.zeros(n), np.zeros(n)
    np.add.at(cin, j, np.maximum(bp, 0.0))    # g (v_i - v_j) > 0 flows from i into j
    np.add.at(cin, i, np.maximum(-bp, 0.0))
    np.add.at(cout, i, np.maximum(-bn, 0.0))  # thresholded with the other orientation's maximum
    np.add.at(cout, j, np.maximum(bn, 0.0))
    return np.maximum(cin, cout), float(np.max(np.abs(b)))


def check_against_numpy(L, batch=4):
    """Check 3: independent of the CSR kernels. Node currents recomputed in numpy from the RETURNED voltages and the host graph
    of oracle.refgraph, to 1e-7 max_e |b_e| per column (at most eight incident entries may fall on the other side of the
    1e-8 max drop threshold when a conductance differs in its last bit between the two builds of the graph, plus
    rounding); Kirchhoff at the terminals: the solve stops at ||b - A x|| <= 1e-10 sqrt(2), a node's share of that
    residual is what its current can be off by -- 1 +- 1e-10 sqrt(n) at both terminals of every pair, and currents >= 0."""
    from oracle import refgraph as rg
    shape, seg = SHAPES["tall"]
    g = raster(shape)
    n = g.size
    pts = focal_nodes(L, g, batch, seg, {}, False)
    src, dst = pair_list(pts, batch + 3, seed=5)
    o = opts(L, batch, 1, seg, rtol=1e-10, criterion=1, atol=0.0)
    got = maps_call(L, g, o, src, dst, None, {})
    assert got["st"]["lattice_maps"] == 1 and got["after"]["csr_built"] == 0
    G = rg.raster_laplacian_from_conductance(g)
    bound = 1e-10 * np.sqrt(n)
    for p in range(len(src)):
        ref, bmax = reference_node_currents(G, got["V"][:, p])
        err = float(np.max(np.abs(got["C"][:, p] - ref)))
        print("pair %d: max |curr - numpy| = %.3e (bound %.3e), terminals %.3e %.3e (bound %.3e)" %
              (p, err, 1e-7 * bmax, abs(got["C"][src[p], p] - 1), abs(got["C"][dst[p], p] - 1), bound))
        assert err <= 1e-7 * bmax, (p, err, bmax)
        assert abs(got["C"][src[p], p] - 1.0) <= bound and abs(got["C"][dst[p], p] - 1.0) <= bound, p
        assert got["C"][:, p].min() >= 0.0


def check_multi(L, batch=4):
    """Check 4b: two replicas on device 0. The maximum map is order-independent and must be equal; the cumulative map adds the
    same non-negative currents per node in another order (per replica, then combined): (pairs + 1) roundings of the sum."""
    shape, seg = SHAPES["small"]
    g = raster(shape)
    n = g.size
    pts = focal_nodes(L, g, batch, seg, {}, False)
    src, dst = pair_list(pts, 2 * batch + 3, seed=5)
    weights = [int(w) for w in np.random.default_rng(7).integers(0, 3, len(src))]
    cum1, mx1 = np.full(n, 0.5), np.full(n, 0.01)
    with L.raster_setup(g, opts(L, batch, 1, seg)) as h:
        R1, _, _, st1 = h.solve_pairs_currents(src, dst, weights=weights, want_currents=False, cum=cum1, mx=mx1)
    assert st1["lattice_maps"] == 1 and st1["not_converged"] == 0
    cumm, mxm = np.full(n, 0.5), np.full(n, 0.01)
    with L.multi_raster_setup(g, opts(L, batch, 1, seg), devices=[0, 0]) as m:
        Rm, stm = m.solve_pairs_currents(src, dst, weights=weights, cum=cumm, mx=mxm)
        assert m.info(0)["csr_built"] == 0 and m.info(1)["csr_built"] == 0
    assert stm["lattice_maps"] == 1 and stm["not_converged"] == 0
    assert np.array_equal(mxm, mx1)
    assert np.all(np.abs(cumm - cum1) <= (len(src) + 1) * 2.0 ** -52 * cum1), float(np.max(np.abs(cumm - cum1)))
    assert np.max(np.abs(Rm - R1) / R1) < 1e-10


def check_default_unchanged(L, batch=4, name="tall"):
    """Check 5: with default options a maps call takes the CSR path, as before."""
    shape, seg = SHAPES[name]
    g = raster(shape)
    pts = focal_nodes(L, g, batch, seg, {}, False)
    src, dst = pair_list(pts, batch + 3, seed=5)
    got = maps_call(L, g, L.default_opts(batch=batch, dia_seg=seg), src, dst, None, {})
    assert got["st"]["lattice_maps"] == 0
    assert got["before"]["csr_built"] == 0 and got["after"]["csr_built"] == 1
