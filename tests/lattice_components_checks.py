"""Checks of csgpu_components and csgpu_solve_rhs served from the lattice form (csrc/lattice_components.h: dia_cc_hook_kernel;
the explicit post-check of csrc/pcg.h through dia_apply) on a handle with csgpu_opts.lattice_maps = 1, without a CSR form of
the fine-level matrix. Shared by the emulator tests (test_lattice_components_emu.py) and their device twins
(test_lattice_components_gpu.py).

The components are a function of the graph alone, so the labels and the count must be EQUAL to those of the CSR path
(lattice_maps = -1) and to scipy.ndimage.label on the mask; the solutions of csgpu_solve_rhs must be equal bit for bit (the
iteration never read the CSR form), only max_relres is summed in another order."""
import functools

import numpy as np

from lattice_maps_checks import csr_bytes

# name -> (shape, components with eight neighbours, with four). All masks keep more than half of the cells (the bound of
# cell space); the counts are those of scipy.ndimage.label.
CASES = {
    "serpentine": ((61, 64), 1, 1),      # long winding path: many hooking / jumping rounds
    "diagonals": ((70, 70), 1, 4),       # the +R-1 / +R+1 slots
    "hwall": ((261, 70), 2, 2),          # no edge across the numbering wrap; two 256-row strips, rows no multiple of 64
    "rand45": ((261, 70), 48, 925),      # components of all sizes, isolated cells, relabel scan, cell-space compaction
    "rand45_small": ((40, 45), 9, 99),
    "allvalid": ((261, 70), 1, 1),       # no NODATA: not cell space
    "allvalid_small": ((40, 45), 1, 1),
}
# csgpu_solve_rhs: (raster, dia_seg or 0 for the default)
RHS_CASES = {"tall": ("allvalid", 16), "small": ("allvalid_small", 0), "rand45": ("rand45", 0)}
PRECISIONS = {"fp64": (np.float64, 0), "fp32": (np.float32, 0), "mixed": (np.float64, 4)}


@functools.lru_cache(maxsize=None)
def _rand45_masks():
    rng = np.random.default_rng(17)
    return rng.random((261, 70)) < 0.45, rng.random((40, 45)) < 0.45


@functools.lru_cache(maxsize=None)
def nodata_mask(name):
    shape = CASES[name][0]
    m = np.zeros(shape, dtype=bool)
    if name == "serpentine":
        for k, j in enumerate(range(2, shape[1], 3)):
            m[:, j] = True
            m[0 if k % 2 == 0 else shape[0] - 1, j] = False
    elif name == "diagonals":
        i = np.arange(shape[0])
        m[i, i] = True
        m[i, shape[1] - 1 - i] = True
    elif name == "hwall":
        m[130, :] = True
    elif name == "rand45":
        m = _rand45_masks()[0]
    elif name == "rand45_small":
        m = _rand45_masks()[1]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def raster(name, dtype=np.float64):
    """conductances exp(N(0, 1)) on the valid cells, 0 on the NODATA cells"""
    m = nodata_mask(name)
    g = np.exp(np.random.default_rng(3).standard_normal(m.shape))
    g = np.where(m, 0.0, g).astype(dtype)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def scipy_labels(name, four):
    """Components of the mask by scipy.ndimage.label, in the compact column-major node numbering, numbered by smallest node id."""
    from scipy import ndimage
    valid = ~nodata_mask(name)
    structure = ndimage.generate_binary_structure(2, 1) if four else np.ones((3, 3), dtype=int)
    lab, cnt = ndimage.label(valid, structure=structure)
    per_node = lab.T.ravel()[valid.T.ravel()]
    uniq, first = np.unique(per_node, return_index=True)
    dense = np.zeros(cnt + 1, dtype=np.int32)
    dense[uniq[np.argsort(first)]] = np.arange(len(uniq), dtype=np.int32)
    out = dense[per_node]
    out.setflags(write=False)
    return out, cnt


_COMPONENTS = {}


def device_components(L, name, four, dtype, avg, maps):
    """components() of a fresh handle, once per library and case: (labels, count, info before, info after)"""
    key = (L.loaded_path(), name, four, np.dtype(dtype).name, avg, maps)
    if key not in _COMPONENTS:
        g = raster(name, dtype)
        kw = {} if maps is None else {"lattice_maps": maps}
        with L.raster_setup(g, L.default_opts(**kw), four_neighbors=four, avg_resistances=avg) as h:
            before = h.info
            lab, cnt = h.components()
            after = h.info
        assert after["lattice_period"] > 0, (name, after)
        assert after["cellspace"] == (1 if nodata_mask(name).any() else 0), (name, after["cellspace"])
        assert after["n"] == int((g > 0).sum()) == len(lab)
        lab.setflags(write=False)
        _COMPONENTS[key] = (lab, cnt, before, after)
    return _COMPONENTS[key]


def check_equals_csr_path(L, name, four, dtype=np.float64, avg=False):
    """Check 1: labels and count of a lattice_maps = 1 handle equal those of a lattice_maps = -1 handle; only the latter builds a
    CSR form, and it is exactly the three CSR arrays larger."""
    lab, cnt, before, after = device_components(L, name, four, dtype, avg, 1)
    rlab, rcnt, rbefore, rafter = device_components(L, name, four, dtype, avg, -1)
    tag = (name, four, np.dtype(dtype).name, avg)
    assert np.array_equal(lab, rlab), (tag, int(np.count_nonzero(lab != rlab)))
    assert cnt == rcnt, (tag, cnt, rcnt)
    assert before["csr_built"] == 0 and rbefore["csr_built"] == 0, tag
    assert after["csr_built"] == 0, tag
    assert rafter["csr_built"] == 1, tag
    assert before["device_bytes"] == rbefore["device_bytes"] == after["device_bytes"], tag
    assert rafter["device_bytes"] - after["device_bytes"] == csr_bytes(rafter, np.dtype(dtype).itemsize), \
        (tag, rafter["device_bytes"], after["device_bytes"], csr_bytes(rafter, np.dtype(dtype).itemsize))


def check_against_scipy(L, name, four):
    """Check 2: independent of the CSR kernels."""
    lab, cnt, _, after = device_components(L, name, four, np.float64, False, 1)
    want, wcnt = scipy_labels(name, four)
    assert wcnt == CASES[name][2 if four else 1], (name, four, wcnt)
    assert cnt == wcnt, (name, four, cnt, wcnt)
    assert np.array_equal(lab, want), (name, four, int(np.count_nonzero(lab != want)))
    assert after["csr_built"] == 0


def host_laplacian(g):
    """Host Laplacian of a raster in the reference's compact numbering (eight neighbours), every node with a stored diagonal
    entry (laplacian!, core.jl:608-634, stores one for an isolated node as well), regularised; and the nodes' cells."""
    import scipy.sparse as sp
    from circuitscape_jl_amd import solver as ps
    from oracle import refgraph as rg, refsolve as rs
    nm = rg.construct_node_map(g, None)
    G = rg.laplacian(rg.construct_graph(g, nm, False, False)).tocoo()
    n = G.shape[0]
    lone = np.setdiff1d(np.arange(n), G.row)
    A = sp.csr_matrix((np.concatenate([G.data, np.zeros(len(lone))]),
                       (np.concatenate([G.row, lone]), np.concatenate([G.col, lone]))), shape=(n, n))
    A.sort_indices()
    row, col = ps._node_coords(nm, np.arange(1, n + 1))
    return rs.regularize(A), row, col


def component_rhs(lab, ncols, dtype, seed=23):
    """ncols zero-sum random columns, each supported inside one component (one with at least two nodes)."""
    rng = np.random.default_rng(seed)
    sizes = np.bincount(lab)
    comps = np.flatnonzero(sizes >= 2)
    B = np.zeros((len(lab), ncols))
    for c in range(ncols):
        nodes = np.flatnonzero(lab == comps[int(rng.integers(0, len(comps)))])
        v = rng.standard_normal(len(nodes))
        B[nodes, c] = v - v.mean()
    return np.asfortranarray(B.astype(dtype))


def check_streamed_host_matrix(L):
    """Check 3: a host matrix streamed into the lattice form in several blocks of rows -- the stand-in, at test size, for a
    handle that cannot hold a CSR form -- answers components() and solve_rhs() without one."""
    name = "rand45_small"
    A, row, col = host_laplacian(np.asarray(raster(name)))
    want, wcnt = scipy_labels(name, False)
    with L.setup(A, L.default_opts(batch=4, host_stream_block=997, lattice_maps=1), node_row=row, node_col=col) as h:
        info = h.info
        assert info["host_blocks"] > 1 and info["cellspace"] == 1 and info["lattice_period"] > 0, info
        assert info["csr_built"] == 0
        lab, cnt = h.components()
        assert h.info["csr_built"] == 0
        assert cnt == wcnt == CASES[name][1]
        assert np.array_equal(lab, want), int(np.count_nonzero(lab != want))
        B = component_rhs(lab, 5, np.float64)
        X, st = h.solve_rhs(B)
        assert st["not_converged"] == 0 and st["lattice_maps"] == 1 and st["max_relres"] < 1e-4, st
        assert h.info["csr_built"] == 0
    # (the residual of the returned solution on the host matrix, column by column)
    for c in range(B.shape[1]):
        assert np.linalg.norm(A @ X[:, c] - B[:, c]) <= 1e-4 * np.linalg.norm(B[:, c]), c


def rhs_call(L, g, o, ncols, four=False):
    """One handle: its components, then one csgpu_solve_rhs of columns drawn from them."""
    with L.raster_setup(g, o, four_neighbors=four) as h:
        lab, _ = h.components()
        B = component_rhs(lab, ncols, g.dtype)
        X, st = h.solve_rhs(B)
        info = h.info
    return X, st, info, B


def check_solve_rhs(L, case, prec, batch):
    """Check 4: batch + 3 columns (a full batch, then a short one) with lattice_maps = 1 and -1."""
    name, seg = RHS_CASES[case]
    dtype, pb = PRECISIONS[prec]
    g = raster(name, dtype)
    kw = dict(batch=batch, precond_bytes=pb)
    if seg:
        kw["dia_seg"] = seg
    X, st, info, B = rhs_call(L, g, L.default_opts(lattice_maps=1, **kw), batch + 3)
    Xr, str_, infor, Br = rhs_call(L, g, L.default_opts(lattice_maps=-1, **kw), batch + 3)
    tag = (case, prec, batch)
    assert info["lattice_period"] > 0 and info["cellspace"] == (1 if nodata_mask(name).any() else 0), tag
    assert np.array_equal(B, Br), tag   # (the components of the two handles are equal, so are the columns drawn from them)
    assert np.array_equal(X, Xr), (tag, float(np.max(np.abs(X - Xr))))
    assert np.any(X != 0)
    assert st["total_iters"] == str_["total_iters"], (tag, st["total_iters"], str_["total_iters"])
    assert st["lattice_maps"] == 1 and str_["lattice_maps"] == 0, tag
    assert st["not_converged"] == 0 and str_["not_converged"] == 0, tag
    assert st["nrhs"] == batch + 3
    a, b = st["max_relres"], str_["max_relres"]
    print("%s: max_relres lattice %.6e csr %.6e" % (tag, a, b))
    if dtype == np.float64:
        assert abs(a - b) <= 1e-3 * max(a, b), (tag, a, b)   # two evaluations of one residual
    assert info["csr_built"] == 0 and infor["csr_built"] == 1, tag


def product_raster():
    """the 261 x 70 hwall raster with an island: a 5 x 5 room inside a one-cell NODATA ring"""
    g = np.array(raster("hwall"))
    g[19:26, 19:26] = 0.0
    g[20:25, 20:25] = np.exp(np.random.default_rng(41).standard_normal((5, 5)))
    return g


def check_product_path(L):
    """Check 5: raster_pairwise_on_device with lattice_maps = 1 against lattice_maps = -1: the same -1 pattern, equal
    resistances, equal cumulative and maximum maps."""
    from circuitscape_jl_amd import solver as ps
    g = product_raster()
    # two focal points per part (above the wall, below it, the room) and one on a NODATA cell (the wall); 1-based
    pts = ([11, 101, 151, 251, 21, 25, 131], [6, 61, 11, 66, 21, 25, 31], [1, 2, 3, 4, 5, 6, 7])
    tight = {"rtol": 1e-10, "atol": 0.0, "criterion": 1}
    out = {}
    for maps in (1, -1):
        solver = ps.HIPAMGSolver(bs=4, opts=dict(tight, lattice_maps=maps))
        st, stc = {}, {}
        plain = ps.raster_pairwise_on_device(g, pts, solver, stats=st)
        cum = ps.initialize_cum_maps(g, write_max=True)
        with_cum = ps.raster_pairwise_on_device(g, pts, solver, stats=stc, cum=cum)
        assert st["not_converged"] == 0 and stc["not_converged"] == 0
        assert stc["lattice_maps"] == (1 if maps > 0 else 0)
        out[maps] = (plain, with_cum, cum)
    R = out[1][0][1:, 1:]
    part = [0, 0, 1, 1, 2, 2, -1]
    for i in range(7):
        for j in range(7):
            if i != j:
                assert (R[i, j] == -1) == (part[i] != part[j] or part[i] < 0), (i, j, R[i, j])
    assert np.all(R[R != -1] >= 0) and np.count_nonzero(R > 0) == 6
    for k in (0, 1):
        assert np.array_equal(out[1][k], out[-1][k]), k
    assert np.array_equal(out[1][0], out[1][1])
    assert np.array_equal(out[1][2].cum_curr, out[-1][2].cum_curr)
    assert np.array_equal(out[1][2].max_curr, out[-1][2].max_curr)
    assert out[1][2].cum_curr.max() > 0


def check_default_unchanged(L, name="allvalid_small"):
    """Check 6: with default options components() builds the CSR form, as before."""
    _, cnt, before, after = device_components(L, name, False, np.float64, False, None)
    assert cnt == 1 and before["csr_built"] == 0 and after["csr_built"] == 1


def check_multi(L, name="rand45_small"):
    """Check 7: components() of the replicas of a multi handle equal the single handle's; no replica builds a CSR form."""
    lab, cnt, _, _ = device_components(L, name, False, np.float64, False, 1)
    with L.multi_raster_setup(np.asarray(raster(name)), L.default_opts(lattice_maps=1), devices=[0, 0]) as m:
        for slot in (0, 1):
            mlab, mcnt = m.components(slot)
            assert mcnt == cnt and np.array_equal(mlab, lab), slot
        assert m.info(0)["csr_built"] == 0 and m.info(1)["csr_built"] == 0
