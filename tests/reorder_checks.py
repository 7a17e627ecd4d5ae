"""Shared checks of the device-side locality reordering (csgpu_opts.reorder, csrc/reorder.h), run on the emulator build by
test_reorder_emu.py and on the device by test_reorder_gpu.py. `L` is the loaded binding (circuitscape_jl_amd.lib).

Every check sets reorder=1. References: scipy (permuted matrix, reverse Cuthill-McKee, sparse direct solves of the CALLER's
matrix), the host restatement of the reference's current post-processing (oracle/refmaps.py) and the reorder=0 handle."""
import functools
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csg
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TIGHT = dict(rtol=1e-10, atol=0.0, criterion=1)
PARITY = 1e-6  # the project's parity bound


@functools.lru_cache(maxsize=2)
def geometric(n, seed=777):
    """bench.geometric_network: node ids without locality by construction"""
    from bench import geometric_network
    G, _ = geometric_network(n, seed)
    G = G.tocsr()
    G.sort_indices()
    return G


@functools.lru_cache(maxsize=1)
def multi_component_graph(hub_degree=2100, seed=5):
    """Two geometric networks of different size, three isolated nodes (a diagonal entry only) and a star whose hub (degree
    hub_degree + 1) hangs on the first network; the ids of everything interleaved by one random permutation."""
    rng = np.random.default_rng(seed)
    A1, A2 = geometric(1200, 3), geometric(500, 4)
    n1, n2 = A1.shape[0], A2.shape[0]
    hub = n1 + n2 + 3
    n = hub + 1 + hub_degree
    W = sp.block_diag([-sp.triu(A1, k=1), -sp.triu(A2, k=1), sp.csr_matrix((3 + 1 + hub_degree, 3 + 1 + hub_degree))]).tolil()
    leaves = np.arange(hub + 1, n)
    w = rng.uniform(0.5, 2.0, size=hub_degree + 1)
    W[hub, leaves] = w[:-1]
    W[17, hub] = w[-1]  # the star joins the first network
    W = sp.csr_matrix(W)
    W = W + W.T
    d = np.asarray(W.sum(axis=1)).ravel()
    d[n1 + n2:n1 + n2 + 3] = 1.0  # isolated nodes: an unknown of their own
    G = (sp.diags(d) - W).tocsr()
    p = rng.permutation(n)
    G = G[p][:, p].tocsr()
    G.sort_indices()
    return G


def permutation_of(h):
    perm = h.permutation()
    assert perm.dtype == np.int32
    return perm


def inverse(perm):
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    return inv


def mean_span(G, perm):
    C = G.tocoo()
    p = np.asarray(perm, dtype=np.int64)
    return float(np.mean(np.abs(p[C.row] - p[C.col])))


# ---- 1: the permutation is one ------------------------------------------------------------------------------------------
def check_permutation(L, G):
    n = G.shape[0]
    with L.setup(G, L.default_opts(reorder=1)) as h:
        perm = permutation_of(h)
        assert h.info["reordered"] == 1 and h.info["reorder_ms"] > 0 and h.info["n"] == n
        assert np.array_equal(np.sort(perm), np.arange(n))
        _, lab = csg.connected_components(G, directed=False)
        for c in np.unique(lab):  # the rows of one component are contiguous
            rows = np.sort(perm[lab == c])
            assert rows[-1] - rows[0] + 1 == len(rows), c
    with L.setup(G, L.default_opts(reorder=1)) as h2:  # the same matrix gives the same order
        assert np.array_equal(permutation_of(h2), perm)
    with L.setup(G, L.default_opts(reorder=0)) as h0:
        assert h0.info["reordered"] == 0 and np.array_equal(permutation_of(h0), np.arange(n))
        assert h0.info["reorder_ms"] == 0 and h0.info["span_after"] == 0
    return perm


def check_not_applied(L, oracle):
    """reorder=1 is ignored where the handle has locality already: raster handles (all-valid and with NODATA), a host CSR
    that takes cell space, a host CSR with the lattice structure of a raster"""
    from oracle import refgraph as rg
    rng = np.random.default_rng(2)
    g = np.exp(rng.standard_normal((40, 37)))
    gh = g.copy()
    gh[rng.random(g.shape) < 0.1] = 0.0
    for cond in (g, gh):
        with L.raster_setup(cond, L.default_opts(reorder=1)) as h:
            assert h.info["reordered"] == 0
            assert np.array_equal(permutation_of(h), np.arange(h.info["n"]))
    from circuitscape_jl_amd import solver as ps
    nm = rg.construct_node_map(gh, None)
    graph = rg.construct_graph(gh, nm, False, False)
    comp = np.asarray(max(rg.connected_components(graph), key=len), dtype=np.int64)  # 1-based ids of the largest component
    A = oracle.regularize(sp.csr_matrix(rg.laplacian(graph))[comp - 1][:, comp - 1])
    row, col = ps._node_coords(nm, comp)
    with L.setup(A, L.default_opts(reorder=1), node_row=row, node_col=col) as h:
        assert h.info["cellspace"] == 1 and h.info["reordered"] == 0
        assert np.array_equal(permutation_of(h), np.arange(A.shape[0]))
    A = oracle.regularize(rg.raster_laplacian_from_conductance(g))
    with L.setup(A, L.default_opts(reorder=1)) as h:  # lattice detected from the matrix
        assert h.info["lattice_period"] > 0 and h.info["reordered"] == 0
        assert np.array_equal(permutation_of(h), np.arange(A.shape[0]))


def check_multi_same_permutation(L, G, devices):
    with L.setup(G, L.default_opts(reorder=1)) as h:
        perm = permutation_of(h)
    with L.multi_setup(G, L.default_opts(reorder=1), devices=devices) as m:
        assert m.ndevices == len(devices)
        for slot in range(m.ndevices):
            assert m.info(slot)["reordered"] == 1
            assert np.array_equal(m.permutation(slot), perm), slot


# ---- 2: the device matrix is P A P', exactly ----------------------------------------------------------------------------
def check_permuted_matrix(L, G):
    with L.setup(G, L.default_opts(reorder=1, precond_bytes=0)) as h:
        assert h.info["reordered"] == 1
        inv = inverse(permutation_of(h))
        B = h.level_matrix(0, "A")
        span_after = h.info["span_after"]
    ref = G[inv][:, inv].tocsr()
    ref.sort_indices()
    assert np.array_equal(B.indptr, ref.indptr)
    assert np.array_equal(B.indices, ref.indices)
    assert np.array_equal(B.data.view(np.int64), ref.data.astype(np.float64).view(np.int64))  # bit-equal: moved, not recomputed
    return B, span_after


# ---- 3: quality against reverse Cuthill-McKee ---------------------------------------------------------------------------
def check_quality(L, G, downloaded=True):
    n = G.shape[0]
    with L.setup(G, L.default_opts(reorder=1, precond_bytes=0)) as h:
        info = h.info
        perm = permutation_of(h)
        B = h.level_matrix(0, "A") if downloaded else None
    assert info["reordered"] == 1
    dev = info["span_after"] * n
    given = mean_span(G, np.arange(n))
    assert abs(info["span_before"] * n - given) <= 1e-9 * given
    assert abs(dev - mean_span(G, perm)) <= 1e-9 * dev
    if B is not None:  # cross-check against the downloaded matrix
        C = B.tocoo()
        assert abs(dev - float(np.mean(np.abs(C.row.astype(np.int64) - C.col)))) <= 1e-9 * dev
    rcm = csg.reverse_cuthill_mckee(G.tocsr(), symmetric_mode=True)
    prcm = np.empty(n, dtype=np.int64)
    prcm[rcm] = np.arange(n)
    ref = mean_span(G, prcm)
    print("mean |col - row|: as given %.1f, device %.1f, reverse Cuthill-McKee %.1f (device / RCM %.2f, given / device %.1f); "
          "reorder %.2f ms of %.2f ms set-up" % (given, dev, ref, dev / ref, given / dev, info["reorder_ms"], info["setup_ms"]))
    assert dev <= 2.0 * ref, (dev, ref)
    assert dev <= given / 10.0, (dev, given)


# ---- 4: same answers through every entry point --------------------------------------------------------------------------
class Direct:
    """Sparse direct solves of the caller's matrix, component by component (one node of every component grounded)."""

    def __init__(self, G):
        self.G = G.tocsr()
        self.n = G.shape[0]
        _, self.lab = csg.connected_components(G, directed=False)
        self.lu = {}

    def comp(self, node):
        return np.flatnonzero(self.lab == self.lab[node])

    def solve_comp(self, node, b):
        """x with A x = b on the component of `node` (b sums to zero there), x = 0 at the component's first node"""
        c = int(self.lab[node])
        nodes = self.comp(node)
        if c not in self.lu:
            keep = nodes[1:]
            self.lu[c] = (keep, spla.splu(self.G[keep][:, keep].tocsc()) if len(keep) else None)
        keep, lu = self.lu[c]
        x = np.zeros(self.n)
        if lu is not None:
            x[keep] = lu.solve(b[keep])
        return x

    def pair(self, s, d):
        b = np.zeros(self.n)
        b[d] += 1.0
        b[s] -= 1.0
        return self.solve_comp(s, b)

    def reduced(self, b, ground):
        """x of the reduced system (rows / columns of `ground` removed) on the components that hold a ground; 0 elsewhere"""
        x = np.zeros(self.n)
        for c in np.unique(self.lab[ground]):
            nodes = np.flatnonzero(self.lab == c)
            keep = np.setdiff1d(nodes, ground)
            x[keep] = spla.spsolve(self.G[keep][:, keep].tocsc(), b[keep])
        return x


def branch_reference(G, v):
    """branch_out of one pair at the caller's CSR positions: |g (v_row - v_col)| at the entries row < col, the reference's
    1e-8 drop threshold (out.jl:250-290), 0 elsewhere"""
    G = G.tocsr()
    rows = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    upper = rows < G.indices
    b = np.abs(G.data) * (v[rows] - v[G.indices])
    mx = b[upper].max()
    b = np.where(np.abs(b / mx) < 1e-8, 0.0, b)
    return np.where(upper, np.abs(b), 0.0), upper


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def check_entry_points(L, G, precond_bytes, batch, seed=0):
    from oracle import refmaps
    n = G.shape[0]
    D = Direct(G)
    rng = np.random.default_rng(seed)
    big = np.flatnonzero(D.lab == np.bincount(D.lab).argmax())
    pts = [int(q) for q in rng.choice(big, size=max(batch + 2, 5), replace=False)]
    npairs = batch + 1  # a ragged last batch
    src = [pts[0]] * npairs
    dst = pts[1:npairs + 1]
    if len(np.unique(D.lab)) > 1:  # a pair inside the second component too
        other = np.flatnonzero(D.lab == np.argsort(np.bincount(D.lab))[-2])
        src[-1], dst[-1] = int(other[0]), int(other[-1])
    o = dict(TIGHT, batch=batch, precond_bytes=precond_bytes)
    h = L.setup(G, L.default_opts(reorder=1, **o))
    h0 = L.setup(G, L.default_opts(reorder=0, **o))
    try:
        assert h.info["reordered"] == 1 and h0.info["reordered"] == 0
        # components: array-equal to the unordered handle's
        lab1, nc1 = h.components()
        lab0, nc0 = h0.components()
        assert nc1 == nc0 == len(np.unique(D.lab)) and np.array_equal(lab1, lab0)
        # products in the caller's numbering
        for k in (1, 4):
            x = rng.standard_normal((n, k))
            ref = G @ x
            y = h.spmv(x if k > 1 else x[:, 0])
            assert np.max(np.abs(y - (ref if k > 1 else ref[:, 0]))) <= 1e-12 * max(1.0, np.abs(ref).max())
        # pair solves: resistances, gathered voltages, voltage columns
        Vd = np.column_stack([D.pair(s, d) for s, d in zip(src, dst)])
        Rd = np.array([Vd[d, p] - Vd[s, p] for p, (s, d) in enumerate(zip(src, dst))])
        gather = pts[:3]
        R, gath, V, st = h.solve_pairs(src, dst, gather=gather, want_voltages=True)
        assert st["not_converged"] == 0
        assert np.max(np.abs(R - Rd) / Rd) < PARITY, np.max(np.abs(R - Rd) / Rd)
        for p, (s, d) in enumerate(zip(src, dst)):
            nodes = D.comp(s)
            assert rel(V[nodes, p], Vd[nodes, p] - Vd[s, p]) < PARITY, p
            if D.lab[s] == D.lab[gather[0]]:
                assert rel(gath[p], Vd[gather, p] - Vd[s, p]) < PARITY, p
        R2, _, _, _ = h.solve_pairs(src, dst)  # the resistance-only path (focal accumulation)
        assert np.max(np.abs(R2 - Rd) / Rd) < PARITY
        # currents: per pair, cumulative with a NON-ZERO incoming vector, maximum, branch currents at the caller's entries
        w = (1 + np.arange(npairs) % 3).astype(np.int32)
        cum = np.full(n, 0.25)
        mx = np.full(n, 1e-3)
        Rc, Vc, C, stc, Br = h.solve_pairs_currents(src, dst, weights=w, want_voltages=True, want_currents=True, cum=cum, mx=mx,
                                                    want_branch=True)
        assert stc["not_converged"] == 0 and np.max(np.abs(Rc - Rd) / Rd) < PARITY
        assert Br.shape == (G.nnz, npairs)
        for p, (s, d) in enumerate(zip(src, dst)):
            vd = np.zeros(n)
            nodes = D.comp(s)
            vd[nodes] = Vd[nodes, p] - Vd[s, p]
            cref = refmaps.get_node_currents(G, vd)
            assert np.max(np.abs(C[:, p] - cref)) < PARITY * cref.max(), p
            bref, upper = branch_reference(G, vd)
            assert np.all(Br[~upper, p] == 0.0), p                     # non-zero at the caller's row < col positions only ...
            sure = bref > 1e-6 * bref.max()
            assert np.all(Br[sure, p] != 0.0), p                       # ... and at all of them that carry current
            assert np.max(np.abs(Br[:, p] - bref)) < PARITY * bref.max(), p
        assert np.allclose(cum, 0.25 + C @ w.astype(np.float64), rtol=1e-12, atol=1e-14)
        assert np.array_equal(mx, np.maximum(1e-3, C.max(axis=1)))
        # general right-hand sides: consistent on every component (the isolated nodes take any value: their rows are x = b)
        nr = min(batch, 2) + 1
        Bm = rng.standard_normal((n, nr))
        for c in np.unique(D.lab):
            nodes = np.flatnonzero(D.lab == c)
            if len(nodes) > 1:
                Bm[nodes] -= Bm[nodes].mean(axis=0)
        X, sr = h.solve_rhs(Bm)
        assert sr["not_converged"] == 0
        for c in np.unique(D.lab):
            nodes = np.flatnonzero(D.lab == c)
            for q in range(nr):
                if len(nodes) == 1:
                    assert abs(X[nodes[0], q] - Bm[nodes[0], q] / G[nodes[0], nodes[0]]) < PARITY * abs(Bm[nodes[0], q])
                    continue
                xd = D.solve_comp(nodes[0], Bm[:, q])[nodes]
                xg = X[nodes, q] - X[nodes[0], q]
                assert rel(xg, xd) < PARITY, (c, q)
        # grounded solves (dense right-hand sides) and sparse sources: one-to-all columns on the largest component
        cols = pts[:min(batch + 1, len(pts))]
        srcs = [[p] for p in cols]
        gnds = [[q for q in cols if q != p] for p in cols]
        Bd = np.zeros((n, len(cols)))
        for c, p in enumerate(cols):
            Bd[p, c] = 1.0
        Xd = np.column_stack([D.reduced(Bd[:, c], gnds[c]) for c in range(len(cols))])
        Xg, Cg, sg = h.solve_grounded(Bd, gnds, want_currents=True)
        assert sg["not_converged"] == 0 and rel(Xg, Xd) < PARITY
        for c in range(len(cols)):
            assert np.all(Xg[gnds[c], c] == 0)
        cum = np.full(n, 0.5)
        mx = np.full(n, 1e-3)
        v, Xs, Cs, ss = h.solve_sources(srcs, gnds, check=cols, want_voltages=True, want_currents=True, cum=cum, mx=mx)
        assert ss["not_converged"] == 0 and rel(Xs, Xd) < PARITY
        assert np.max(np.abs(v - Xd[cols, np.arange(len(cols))]) / Xd[cols, np.arange(len(cols))]) < PARITY
        assert np.array_equal(v, Xs[cols, np.arange(len(cols))])
        for c in range(len(cols)):
            cref = refmaps.get_node_currents(G, Xd[:, c])
            assert np.max(np.abs(Cs[:, c] - cref)) < PARITY * cref.max(), c
            assert np.max(np.abs(Cg[:, c] - cref)) < PARITY * cref.max(), c
        assert np.allclose(cum, 0.5 + Cs.sum(axis=1), rtol=1e-12, atol=1e-14)
        assert np.array_equal(mx, np.maximum(1e-3, Cs.max(axis=1)))
        # short-circuited node sets
        sets = [[pts[0]] + [int(q) for q in G[pts[0]].indices if q != pts[0]][:3], [pts[1], pts[2]], [pts[3]]]
        sets = [sorted(set(q)) for q in sets]
        if not (set(sets[0]) & set(sets[1])) and not (set(sets[0]) & set(sets[2])):
            a, b = [0, 0, 1], [1, 2, 2]
            Rr, srp = h.solve_region_pairs(sets, a, b)
            assert srp["not_converged"] == 0
            for p in range(3):
                I, J = sets[a[p]], sets[b[p]]
                vv = np.zeros(n)
                vv[I] = 1.0
                nodes = D.comp(I[0])
                free = np.setdiff1d(nodes, I + J)
                rhs = -(G[free][:, I] @ np.ones(len(I)))
                vv[free] = spla.spsolve(G[free][:, free].tocsc(), rhs)
                Rref = 1.0 / float(vv @ (G @ vv))
                assert abs(Rr[p] - Rref) / Rref < PARITY, (p, Rr[p], Rref)
    finally:
        h.close()
        h0.close()


# ---- 5: the reference's network goldens with reorder = 1 ----------------------------------------------------------------
class SetupSpy:
    """records csgpu_get_info().reordered of every handle the solver layer sets up"""

    def __init__(self, L):
        self.L = L
        self.seen = []

    def __enter__(self):
        self.orig = self.L.setup

        def setup(*a, **kw):
            h = self.orig(*a, **kw)
            self.seen.append(h.info["reordered"])
            return h

        self.L.setup = setup
        return self

    def __exit__(self, *a):
        self.L.setup = self.orig


def check_network_golden(L, name):
    from circuitscape_jl_amd import solver as ps
    from conftest import compare_resistances, load_case
    from helpers import expected_ids, run_fixture
    from test_emu_solver import _check_network_tables
    case = load_case(name)
    with SetupSpy(L) as spy:
        got = run_fixture(case, ps.HIPAMGSolver(bs=8, opts={"reorder": 1}))
        exp = np.array(case["expected"])
        assert np.array_equal(expected_ids(case), got[1:, 0])
        compare_resistances(exp[1:, 1:], got[1:, 1:], rtol=1e-6, atol=1e-9)
        st = {"want_tables": True}
        run_fixture(case, ps.HIPAMGSolver(bs=4, opts={"rtol": 1e-10, "atol": 0.0, "criterion": 1, "reorder": 1}), stats=st)
        assert _check_network_tables(case, st) > 0
    assert spy.seen and all(r == 1 for r in spy.seen), spy.seen


def check_network_advanced_golden(L, name):
    from circuitscape_jl_amd import solver as ps
    from conftest import load_case
    from helpers import run_network_advanced_fixture
    case = load_case(name)
    with SetupSpy(L) as spy:
        got = run_network_advanced_fixture(case, ps.HIPAMGSolver(bs=1, opts={"reorder": 1}))
    exp = np.array(case["expected_voltages"])
    assert np.array_equal(exp[:, 0] + 1, got[:, 0])
    assert np.max(np.abs(exp[:, 1] - got[:, 1])) <= 1e-5 * max(1.0, np.abs(exp[:, 1]).max())
    assert spy.seen and all(r == 1 for r in spy.seen), spy.seen


# ---- 6: several replicas ------------------------------------------------------------------------------------------------
def check_multi(L, G, devices, npts=21, seed=11):
    """multi_setup(reorder=1): solve_sources / solve_grounded / solve_pairs_currents equal to the single reordered handle
    (bounds of test_multi_sources_two_replicas_on_one_device)"""
    n = G.shape[0]
    rng = np.random.default_rng(seed)
    pts = [int(q) for q in rng.choice(n, size=npts, replace=False)]
    src = [[p] for p in pts]
    gnd = [[q for q in pts if q != p] for p in pts]
    ps_, pd_ = [pts[0]] * (npts - 1), pts[1:]
    o = lambda: L.default_opts(batch=8, itmax=3000, reorder=1)
    with L.setup(G, o(), index_dtype=np.int32, index_base=0) as h:
        assert h.info["reordered"] == 1
        cum1, mx1 = np.zeros(n), np.zeros(n)
        v1, X1, C1, st1 = h.solve_sources(src, gnd, check=pts, want_voltages=True, want_currents=True, cum=cum1, mx=mx1)
        assert st1["not_converged"] == 0
        pc1, pm1 = np.full(n, 0.5), np.full(n, 0.01)
        R1, _, _, sp1 = h.solve_pairs_currents(ps_, pd_, want_currents=False, cum=pc1, mx=pm1)
    with L.multi_setup(G, o(), devices=devices, index_dtype=np.int32, index_base=0) as m:
        assert m.ndevices == len(devices) and all(m.info(s)["reordered"] == 1 for s in range(m.ndevices))
        cumm, mxm = np.zeros(n), np.zeros(n)
        vm, Xm, Cm, stm = m.solve_sources(src, gnd, check=pts, want_voltages=True, want_currents=True, cum=cumm, mx=mxm)
        assert sum(stm["device_pairs"]) == npts and stm["not_converged"] == 0
        B = np.zeros((n, npts))
        for c, p in enumerate(pts):
            B[p, c] = 1.0
        Xg, _, stg = m.solve_grounded(B, gnd)
        assert stg["not_converged"] == 0
        pcm, pmm = np.full(n, 0.5), np.full(n, 0.01)
        Rm, spm = m.solve_pairs_currents(ps_, pd_, cum=pcm, mx=pmm)
    assert np.max(np.abs(vm - v1) / v1) < 1e-6
    assert np.max(np.abs(Xm - X1)) < 1e-6 * np.max(np.abs(X1)) and np.max(np.abs(Xg - X1)) < 1e-6 * np.max(np.abs(X1))
    assert np.max(np.abs(Cm - C1)) < 1e-6 * np.max(C1)
    assert np.max(np.abs(cumm - cum1)) < 1e-6 * np.max(cum1) and np.max(np.abs(mxm - mx1)) < 1e-6 * np.max(mx1)
    assert np.max(np.abs(Rm - R1) / R1) < 1e-6
    assert np.max(np.abs(pcm - pc1)) < 1e-6 * np.max(pc1) and np.max(np.abs(pmm - pm1)) < 1e-6 * np.max(pm1)


# ---- expanders are left alone -------------------------------------------------------------------------------------------
def check_expander_not_reordered(L, n=120000):
    """A graph the expansion probe calls an expander (Erdos-Renyi, BASELINE configs[4]'s kind) has no locality to restore:
    with reorder=1 the probe runs once, before the ordering, the handle is not reordered and is the reorder=0 handle -- one
    level, the same iterations and the same answers bit for bit."""
    import bench
    G, rng = bench.random_network(n)
    focal = rng.choice(G.shape[0], size=8, replace=False)
    src, gnd, chk = bench.one_to_all_columns(focal)
    out = {}
    for ro in (0, 1):
        with L.setup(G, L.default_opts(batch=8, precond_bytes=4, itmax=3000, reorder=ro), index_dtype=np.int32,
                     index_base=0) as h:
            info = h.info
            v, _, _, st = h.solve_sources(src, gnd, check=chk)
            assert info["levels"] == 1 and info["expander_probe_hit"] == 1 and info["reordered"] == 0 and st["not_converged"] == 0
            assert np.array_equal(permutation_of(h), np.arange(G.shape[0]))
            out[ro] = (v, st["total_iters"])
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
