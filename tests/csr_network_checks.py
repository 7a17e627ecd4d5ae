"""Checks of the general-CSR kernel family on network-shaped matrices: spmv_kernel in its K and tile variants and
spmm_longrow_kernel (csrc/spmv.h); spgemm_merge_kernel / spgemm_lds_kernel / spgemm_tentative_kernel and transpose with
row_rank_sort_kernel (csrc/amg_setup.h). Run on the emulator build by test_csr_network_emu.py and on the device by
test_csr_network_gpu.py. `L` is the loaded binding (circuitscape_jl_amd.lib).

Reference and tolerance, the same wherever a product is checked: the scipy float64 product of the operands as the kernel
sees them (the matrix read back from the handle and the vector, both rounded to the precision the kernel accumulates in),
and per entry the forward bound of an inner product summed in any order,

    |y - ref|[i, c] <= (len_i + 2) * u * (|M| |x|)[i, c],     len_i = stored length of row i, u = np.finfo(dtype).eps.

The bound is per row: an error in a row of small magnitude cannot hide behind a large one. Every check returns the largest
observed error / bound, which the tests print; it is information, never a tolerance.

The matrices (every check prints their row lengths, levels and merge brackets; what a test relies on is asserted):
  ragged     n = 3001, hubs of more than 2560 entries at rows 0, 127, 128, 255, 256, 3000; rows 7, 300, 2990 diagonal only
  clique     700 nodes, nnz / n >= 40: the 32-row long-row kernel
  dense      uniform random, nnz / n in [16, 40): the 64-row long-row kernel; hubs of more than 2560 entries at rows 63, 64
  geo<d>     random geometric, n = 3000, mean degree about d = 2, 4, 10, 20, 40, 90
  geo<d>_hub the same with about 2700 more entries in the row of node 2; R, Q^T and [S Q] then have rows that long too
  pa         preferential attachment, n = 4000, m = 2;  tree: random tree, n = 5000
  tree_hub   the tree with 2700 nodes hung on node 2: the only graph whose general products have a mean row <= 3 (merge
             width 2; the plain tree stays on the LDS fast path), which is why it is here

On the emulator, check A does not see a broken tile clamp in spmv_kernel's accumulation (max(s_rp[r], ts) dropped): the
out-of-range LDS reads land on zeroed memory there. That mutation is caught by check B on the [S Q] rows of the hub graphs
and by D; do not rely on A alone for rows that span tiles unless it runs on the device."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.spatial import cKDTree

PARITY = 1e-6       # the project's parity bound (reorder_checks.PARITY)
TILE = 2560         # kSpmvTile: nonzeros staged in LDS per tile; K >= 16 works on half blocks (128 rows, 1280 nonzeros)
FINE_KS = (1, 2, 4, 8, 16, 32)
LEVEL_KS = (1, 4, 16, 32)
BRACKETS = ("<=3", "<=6", "<=12", "<=24", "<=48", ">48")  # the merge widths 2, 4, 8, 16, 32, 64 of spgemm()

HUB = 2             # id of the hub of the hierarchy graphs: its diagonal is among the first entries of its row block
HUB_DEGREE = 2700
GEO_DEGREES = (2, 4, 10, 20, 40, 90)
HIERARCHY_GRAPHS = tuple("geo%d%s" % (d, s) for d in GEO_DEGREES for s in ("", "_hub")) + ("pa", "tree", "tree_hub")


# ---- matrices -----------------------------------------------------------------------------------------------------------
def laplacian(n, I, J, w, shift=0.0):
    """Graph Laplacian (+ shift on the diagonal) of the edges (I, J) with conductances w; parallel edges add up, self
    loops are dropped, every row stores its diagonal entry."""
    I, J, w = np.asarray(I), np.asarray(J), np.asarray(w, dtype=np.float64)
    keep = I != J
    W = sp.coo_matrix((w[keep], (I[keep], J[keep])), shape=(n, n)).tocsr()
    W = W + W.T
    d = np.asarray(W.sum(axis=1)).ravel() + shift
    A = (sp.diags(d) - W).tocsr()
    A.sort_indices()
    assert np.all(A.diagonal() == d) and (shift == 0.0 or d.min() > 0)
    return A


def _star(rng, hub, degree, eligible):
    to = rng.choice(eligible[eligible != hub], size=degree, replace=False)
    return np.full(degree, hub), to, rng.uniform(0.5, 2.0, degree)


RAGGED_HUBS = {0: 2561, 127: 2570, 128: 2600, 255: 2650, 256: 2700, 3000: 2997}  # row -> edges drawn for it
RAGGED_ALONE = (7, 300, 2990)


def ragged_matrix(seed=11):
    """n = 3001, background degree about 3, hubs longer than one 2560-entry tile on both sides of the 128- and 256-row
    block seams and in the last, partial block, three rows that hold a diagonal entry only; + 1 on the diagonal."""
    n = 3001
    rng = np.random.default_rng(seed)
    eligible = np.setdiff1d(np.arange(n), RAGGED_ALONE)
    back = np.setdiff1d(eligible, list(RAGGED_HUBS))
    m = (3 * len(back)) // 2
    I, J, w = [rng.choice(back, m)], [rng.choice(back, m)], [rng.uniform(0.5, 2.0, m)]
    for hub, degree in RAGGED_HUBS.items():
        a, b, c = _star(rng, hub, degree, eligible)
        I.append(a), J.append(b), w.append(c)
    return laplacian(n, np.concatenate(I), np.concatenate(J), np.concatenate(w), shift=1.0)


def clique_matrix(n=700, seed=12):
    rng = np.random.default_rng(seed)
    I, J = np.triu_indices(n, k=1)
    return laplacian(n, I, J, rng.uniform(0.5, 2.0, len(I)), shift=1.0)


DENSE_HUBS = (63, 64)  # the two sides of a seam of the long-row kernel's 64-row blocks


def dense_random_matrix(n=3000, seed=13):
    """Uniform random edges (no locality: one level by design), nnz / n about 25, and two hub rows longer than the long-row
    kernel's 2560-entry tile. (n = 3000, not 2000: a row of a 2000-node graph cannot hold more than 2000 entries.)"""
    rng = np.random.default_rng(seed)
    m = 10 * n
    I, J, w = [rng.integers(0, n, m)], [rng.integers(0, n, m)], [rng.uniform(0.5, 2.0, m)]
    for hub in DENSE_HUBS:
        a, b, c = _star(rng, hub, HUB_DEGREE, np.arange(n))
        I.append(a), J.append(b), w.append(c)
    return laplacian(n, np.concatenate(I), np.concatenate(J), np.concatenate(w), shift=1.0)


# name -> (builder, nnz / n bracket [lo, hi), max row above the tile, min row == 1)
FINE_MATRICES = {
    "ragged": (ragged_matrix, (0, 16), True, True),          # the 256-row kernel
    "clique": (clique_matrix, (40, np.inf), False, False),   # the 32-row long-row kernel
    "dense": (dense_random_matrix, (16, 40), True, False),   # the 64-row long-row kernel
}


def geometric_graph(d, hub, n=3000, seed=21):
    """Random geometric graph of mean degree about d in the unit square, a path along x for connectivity, node ids
    permuted at random; hub: node HUB gets HUB_DEGREE more edges to nodes drawn at random."""
    rng = np.random.default_rng(seed + d)
    pts = rng.random((n, 2))
    pairs = cKDTree(pts).query_pairs(np.sqrt(d / (np.pi * n)), output_type="ndarray")
    order = np.argsort(pts[:, 0])
    I = np.concatenate([pairs[:, 0], order[:-1]])
    J = np.concatenate([pairs[:, 1], order[1:]])
    perm = rng.permutation(n)
    I, J = perm[I], perm[J]
    w = rng.uniform(0.5, 2.0, len(I))
    if hub:
        a, b, c = _star(rng, HUB, HUB_DEGREE, np.arange(n))
        I, J, w = np.concatenate([I, a]), np.concatenate([J, b]), np.concatenate([w, c])
    return laplacian(n, I, J, w)


def preferential_attachment_graph(n=4000, m=2, seed=31):
    rng = np.random.default_rng(seed)
    targ, I, J = [0], [], []
    for v in range(1, n):
        for t in set(int(targ[q]) for q in rng.integers(0, len(targ), m)):
            I.append(v), J.append(t)
            targ += [t, v]
    return laplacian(n, I, J, rng.uniform(0.5, 2.0, len(I)))


def random_tree(hub, n=5000, seed=32):
    """every node hangs on an earlier node drawn at random; hub: HUB_DEGREE of the nodes hang on node HUB instead. With
    the hub the mean row stays below 3 entries while one row is far longer than a lane group of the SpGEMM fast path
    (64), so its products take the narrowest general merge (width 2)."""
    rng = np.random.default_rng(seed)
    I = np.arange(1, n)
    J = np.array([rng.integers(0, v) for v in I])
    if hub:
        J[rng.choice(np.arange(HUB, n - 1), size=HUB_DEGREE, replace=False)] = HUB  # (J[v - 1] is the parent of v > HUB)
    return laplacian(n, I, J, rng.uniform(0.5, 2.0, n - 1))


_GRAPHS = {}


def hierarchy_graph(name):
    if name not in _GRAPHS:
        if name == "pa":
            G = preferential_attachment_graph()
        elif name.startswith("tree"):
            G = random_tree(name.endswith("_hub"))
        else:
            G = geometric_graph(int(name[3:].split("_")[0]), name.endswith("_hub"))
        if name.endswith("_hub"):
            assert G.indptr[HUB + 1] - G.indptr[HUB] > HUB_DEGREE
        if name.startswith("tree"):
            assert G.nnz <= 3 * G.shape[0]
        _GRAPHS[name] = G
    return _GRAPHS[name]


def row_stats(M):
    lens = np.diff(M.indptr)
    return int(lens.min()), float(lens.mean()), int(lens.max())


# ---- the bound ----------------------------------------------------------------------------------------------------------
def row_bound(M, xs, u):
    """(len_i + 2) * u * (|M| |x|)[i, c] for a float64 CSR matrix M and a float64 block xs"""
    lens = np.diff(M.indptr).astype(np.float64)
    return (lens[:, None] + 2.0) * u * (abs(M) @ np.abs(xs))


def worst_ratio(err, bound, what):
    """max err / bound over the entries; an entry whose bound is 0 must be exact. Asserts err <= bound everywhere."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert err.shape == bound.shape and np.all(np.isfinite(err)), what
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s: error %.3e above the bound %.3e (ratio %.3g) at %s" % (what, err[at], bound[at], worst, at))
    return worst


def check_product(M, x, y, dt, what):
    """y (computed in dt from M and x as given to the kernel) against scipy within the per-row bound; returns (ratio,
    ref, bound, xs) with x as a block"""
    M64 = M.astype(dt).astype(np.float64)
    xs = np.asarray(x, dtype=dt).astype(np.float64).reshape(M.shape[1], -1)
    y = np.asarray(y, dtype=np.float64).reshape(M.shape[0], -1)
    ref = M64 @ xs
    bound = row_bound(M64, xs, float(np.finfo(dt).eps))
    return worst_ratio(np.abs(y - ref), bound, what), ref, bound, xs


# ---- A: the fine product on the ragged and dense matrices ---------------------------------------------------------------
def check_fine_products(L, name, dtype, ks=FINE_KS):
    build, (lo, hi), above_tile, has_single = FINE_MATRICES[name]
    A = build()
    n = A.shape[0]
    lens = np.diff(A.indptr)
    assert lo <= A.nnz / n < hi, (name, A.nnz / n)
    assert (lens.max() > TILE) == above_tile and (lens.min() == 1) == has_single, (name, row_stats(A))
    if name == "ragged":
        assert all(TILE < lens[r] <= n for r in RAGGED_HUBS) and all(lens[r] == 1 for r in RAGGED_ALONE)
        assert all(lens[r] > 2 * (TILE // 2) for r in RAGGED_HUBS)  # three 1280-entry tiles at K >= 16
    if name == "dense":
        assert all(lens[r] > TILE for r in DENSE_HUBS)
    Ain = A.astype(dtype)
    worst = 0.0
    with L.setup(Ain, L.default_opts(max_levels=1)) as h:
        info = h.info
        assert info["levels"] == 1 and info["val_bytes"] == np.dtype(dtype).itemsize and info["reordered"] == 0
        B = h.level_matrix(0, "A")
        assert B.dtype == np.dtype(dtype) and np.array_equal(B.indptr, Ain.indptr) and np.array_equal(B.indices, Ain.indices)
        assert np.array_equal(B.data, Ain.data)  # the kernel's matrix is the input rounded to the handle's precision
        for k in ks:
            x = np.random.default_rng(100 + k).standard_normal((n, k)).astype(dtype)
            y = h.spmv(x if k > 1 else x[:, 0])
            assert y.dtype == np.dtype(dtype)
            worst = max(worst, check_product(B, x, y, dtype, "%s %s K=%d" % (name, np.dtype(dtype).name, k))[0])
    print("fine product %s %s: rows min/mean/max %d/%.2f/%d, worst error / bound %.3f"
          % (name, np.dtype(dtype).name, *row_stats(A), worst))
    return worst


# ---- B, C: the hierarchy of a graph, set up once per (library, graph, precision) ------------------------------------------
class Hier:
    def __init__(self, L, name, precond_bytes, dtype=np.float64):
        self.name, self.G = name, hierarchy_graph(name).astype(dtype)
        self.h = L.setup(self.G, L.default_opts(precond_bytes=precond_bytes))
        try:
            info = self.h.info
            self.levels = info["levels"]
            self.level_n = info["level_n"]
            self.dt = np.float32 if (info["precond_bytes"] or info["val_bytes"]) == 4 else np.float64
            assert info["reordered"] == 0 and info["val_bytes"] == np.dtype(dtype).itemsize
            assert self.dt == (np.float32 if precond_bytes == 4 or np.dtype(dtype).itemsize == 4 else np.float64)
        except BaseException:
            self.h.close()  # (not yet in _HIER: release() would never see it)
            raise
        self.mats = {}

    def matrix(self, lvl, which):
        """the operator as read back (None where the size query reports it absent)"""
        if (lvl, which) not in self.mats:
            M = self.h.level_matrix(lvl, which)
            self.mats[lvl, which] = M if M.nnz > 0 else None
        return self.mats[lvl, which]

    def seen(self, lvl, which):
        """float64 copy of the operator as the kernels of the hierarchy see it"""
        return self.matrix(lvl, which).astype(self.dt).astype(np.float64)


_HIER = {}


def hierarchy(L, name, precond_bytes, dtype=np.float64):
    key = (L.loaded_path(), name, precond_bytes, np.dtype(dtype).name)
    if key not in _HIER:
        _HIER[key] = Hier(L, name, precond_bytes, dtype)
    return _HIER[key]


def release():
    for H in _HIER.values():
        H.h.close()
    _HIER.clear()


def check_level_operators(L, name, precond_bytes, ks=LEVEL_KS, dtype=np.float64):
    """B: every operator of every level times a block of vectors through level_spmv, and the dots fused into [S Q]"""
    H = hierarchy(L, name, precond_bytes, dtype)
    assert H.levels >= 2, (name, H.level_n)
    u = float(np.finfo(H.dt).eps)
    worst, worst_dot, done = 0.0, 0.0, []
    for lvl in range(H.levels):
        last = lvl == H.levels - 1
        for which in ("A", "P", "R") + (("Q", "QT", "M") if lvl == 0 else ()):
            M = H.matrix(lvl, which)
            if M is None:
                assert last and which != "A", (name, lvl, which)  # only P and R of the coarsest level may be absent
                continue
            done.append((lvl, which))
            for k in ks:
                x = np.random.default_rng(1000 * lvl + k).standard_normal((M.shape[1], k)).astype(H.dt)
                y, dots = H.h.level_spmv(lvl, which, x if k > 1 else x[:, 0])
                what = "%s pb=%d level %d %s K=%d" % (name, precond_bytes, lvl, which, k)
                r, ref, bound, xs = check_product(M, x, y, H.dt, what)
                worst = max(worst, r)
                if which == "M":
                    nr = M.shape[0]
                    refd = np.einsum("ik,ik->k", xs[:nr], ref)
                    absd = np.einsum("ik,ik->k", np.abs(xs[:nr]), np.abs(ref))
                    bd = np.einsum("ik,ik->k", np.abs(xs[:nr]), bound) + (nr + 2) * np.finfo(np.float64).eps * absd
                    worst_dot = max(worst_dot, worst_ratio(np.abs(dots - refd), bd, what + " fused dots"))
                else:
                    assert dots is None
    assert all((0, w) in done for w in ("A", "P", "R", "Q", "QT", "M")), (name, done)
    print("level products %s pb=%d u=%.1e: levels %s, worst error / bound %.3f (fused dots %.3f)"
          % (name, precond_bytes, u, H.level_n, worst, worst_dot))
    return worst, worst_dot


def sorted_within_rows(M):
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    return bool(np.all(np.diff(M.indices.astype(np.int64))[np.diff(rows) == 0] > 0))  # strictly increasing inside a row


def same_matrix(X, Y):
    return X.shape == Y.shape and abs(X - Y).nnz == 0


def values_on(pattern, M):
    """values of M at the stored positions of `pattern` (CSR, sorted within rows); M's pattern is a subset of it"""
    nc = pattern.shape[1]
    rows = np.repeat(np.arange(pattern.shape[0], dtype=np.int64), np.diff(pattern.indptr))
    keys = rows * nc + pattern.indices
    C = M.tocoo()
    C.sum_duplicates()
    pos = np.searchsorted(keys, C.row.astype(np.int64) * nc + C.col)
    assert np.all(pos < len(keys)) and np.array_equal(keys[np.minimum(pos, len(keys) - 1)], C.row.astype(np.int64) * nc + C.col)
    out = np.zeros(pattern.nnz)
    out[pos] = C.data
    return out


def merge_bracket(mean):
    for name, top in zip(BRACKETS, (3.0, 6.0, 12.0, 24.0, 48.0, np.inf)):
        if mean <= top:
            return name


def general_products(H):
    """The two SpGEMM products of every level that coarsens, A P and R (A P), from the read-back operands: (level, product,
    mean row of the left operand, its maximum row, maximum row of the right operand, general); general = outside the LDS
    fast path of spgemm() (right maximum > 12 or left maximum > 64), where the mean selects the merge width."""
    out = []
    for lvl in range(H.levels - 1):
        A, P, R = H.seen(lvl, "A"), H.seen(lvl, "P"), H.seen(lvl, "R")
        AP = (abs(A) @ abs(P)).tocsr()
        for what, X, Y in (("A*P", A, P), ("R*(AP)", R, AP)):
            ma, mb = int(np.diff(X.indptr).max()), int(np.diff(Y.indptr).max())
            out.append((lvl, what, X.nnz / X.shape[0], ma, mb, mb > 12 or ma > 64))
    return out


def check_setup_kernels(L, name, precond_bytes, dtype=np.float64):
    """C: transposes, sorted rows, the Galerkin products and level 0's matrix, on every level"""
    H = hierarchy(L, name, precond_bytes, dtype)
    assert H.levels >= 2, (name, H.level_n)
    u = float(np.finfo(H.dt).eps)
    A0 = H.matrix(0, "A")
    assert A0.dtype == H.G.dtype and np.array_equal(A0.indptr, H.G.indptr) and np.array_equal(A0.indices, H.G.indices)
    assert np.array_equal(A0.data, H.G.data)  # the input (rounded to fp32 by the caller of an fp32 handle), bit for bit
    worst = 0.0
    for lvl in range(H.levels):
        for which in ("A", "P", "R", "Q", "QT", "M"):
            M = H.matrix(lvl, which)
            if M is not None:
                assert sorted_within_rows(M), (name, lvl, which)
                assert M.indptr[0] == 0 and M.indptr[-1] == M.nnz and np.all(np.diff(M.indptr) >= 0)
                assert M.nnz == 0 or (M.indices.min() >= 0 and M.indices.max() < M.shape[1])
        if lvl == H.levels - 1:
            assert H.matrix(lvl, "A") is not None
            continue
        A, P, R = H.seen(lvl, "A"), H.seen(lvl, "P"), H.seen(lvl, "R")
        assert A.shape == (H.level_n[lvl],) * 2 and P.shape == (H.level_n[lvl], H.level_n[lvl + 1])
        assert same_matrix(R, P.T.tocsr()), (name, lvl, "R != P'")
        if lvl == 0:
            assert same_matrix(H.seen(0, "QT"), H.seen(0, "Q").T.tocsr()), (name, "QT != Q'")
        Ac = H.matrix(lvl + 1, "A")
        S = (abs(R) @ (abs(A) @ abs(P))).tocsr()  # no cancellation: its stored pattern is the structural pattern
        S.sort_indices()
        assert S.data.min() > 0
        assert np.array_equal(Ac.indptr, S.indptr) and np.array_equal(Ac.indices, S.indices), (name, lvl, "Galerkin pattern")
        ref = values_on(S, P.T.tocsr() @ (A @ P))
        c = int(np.diff(R.indptr).max()) + int(np.diff(A.indptr).max()) + 4
        worst = max(worst, worst_ratio(np.abs(Ac.data.astype(np.float64) - ref), c * u * S.data,
                                       "%s pb=%d Galerkin product of level %d" % (name, precond_bytes, lvl)))
    prods = general_products(H)
    for lvl, what, mean, ma, mb, general in prods:
        print("  %s pb=%d level %d %-7s left rows mean %.2f max %d, right rows max %d: %s"
              % (name, precond_bytes, lvl, what, mean, ma, mb, "merge " + merge_bracket(mean) if general else "LDS fast path"))
    stats = ", ".join("%s %d/%.2f/%d" % (w, *row_stats(H.matrix(0, w))) for w in ("A", "R", "QT", "M"))
    print("set-up %s pb=%d: levels %s, level 0 rows min/mean/max %s, worst Galerkin error / bound %.3f"
          % (name, precond_bytes, H.level_n, stats, worst))
    return worst


def covered_brackets(L, cases):
    """the merge-width brackets the general SpGEMM products of `cases` = [(graph, precond_bytes), ...] fall into"""
    seen = {}
    for name, pb in cases:
        for lvl, what, mean, ma, mb, general in general_products(hierarchy(L, name, pb)):
            if general:
                seen.setdefault(merge_bracket(mean), []).append((name, pb, lvl, what))
    return seen


def check_coverage(L, cases):
    seen = covered_brackets(L, cases)
    for b in BRACKETS:
        print("merge bracket %-4s: %d products, e.g. %s" % (b, len(seen.get(b, [])), seen.get(b, [None])[0]))
    assert all(b in seen for b in BRACKETS), sorted(seen)
    return seen


# ---- D: solves that run the epilogues on long rows ----------------------------------------------------------------------
def diagonal_tile_is_not_the_last(A, row, block_rows, tile):
    """In the row block of `row` (block_rows rows, staged `tile` nonzeros at a time from the block's first nonzero), the
    row's diagonal entry lies in an earlier tile than the row's last entry."""
    k0 = A.indptr[(row // block_rows) * block_rows]
    cols = A.indices[A.indptr[row]:A.indptr[row + 1]]
    kd = A.indptr[row] + int(np.flatnonzero(cols == row)[0])
    return (kd - k0) // tile < (A.indptr[row + 1] - 1 - k0) // tile


def check_epilogue_solves(L, d, precond_bytes, batch):
    G = hierarchy_graph("geo%d_hub" % d)
    n = G.shape[0]
    assert G.indptr[HUB + 1] - G.indptr[HUB] > TILE
    assert diagonal_tile_is_not_the_last(G, HUB, 256, TILE) and diagonal_tile_is_not_the_last(G, HUB, 128, TILE // 2)
    A = G.copy()
    A.data = A.data + np.finfo(np.float64).eps * np.linalg.norm(A.data)  # the reference's shift, on every stored entry
    rng = np.random.default_rng(7 * d + batch)
    npairs = batch + 3  # a ragged last batch
    pts = [int(q) for q in rng.choice(np.setdiff1d(np.arange(n), [HUB]), size=2 * npairs, replace=False)]
    src, dst = pts[:npairs], pts[npairs:]
    src[1] = HUB  # one pair leaves from the hub
    lu = spla.splu(A.tocsc())
    Vd = np.zeros((n, npairs))
    for p, (s, t) in enumerate(zip(src, dst)):
        b = np.zeros(n)
        b[t] += 1.0
        b[s] -= 1.0
        v = lu.solve(b)
        Vd[:, p] = v - v[s]
    Rd = Vd[dst, np.arange(npairs)]
    with L.setup(A, L.default_opts(precond_bytes=precond_bytes, batch=batch, rtol=1e-10, atol=0.0)) as h:
        info = h.info
        R, _, V, st = h.solve_pairs(src, dst, want_voltages=True)
    assert info["levels"] >= 2 and info["reordered"] == 0
    assert st["not_converged"] == 0, st
    eR = float(np.max(np.abs(R - Rd) / Rd))
    eV = max(float(np.max(np.abs(V[:, p] - Vd[:, p])) / np.max(np.abs(Vd[:, p]))) for p in range(npairs))
    print("solve geo%d_hub pb=%d batch=%d: levels %s, %d iterations, resistances %.2e, voltages %.2e (bound %.0e)"
          % (d, precond_bytes, batch, info["level_n"], st["total_iters"], eR, eV, PARITY))
    assert eR < PARITY, eR
    assert eV < PARITY, eV
    return eR, eV
