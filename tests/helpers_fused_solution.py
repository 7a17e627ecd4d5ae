"""Checks of the fused residual update + restriction for solves that CARRY the solution (csgpu_opts.fused_restrict = 1,
the XUP form of lattice_rupd_restrict_kernel, csrc/lattice.h): shared by the emulator tests (test_emu_fused_solution.py)
and the device tests (test_gpu_fused_solution.py). Every block compares a handle with fused_restrict = 1 against one
with fused_restrict = -1, otherwise identical (precond_bytes = 0, fixed_k = 1, stream = -1), in the style of
helpers.check_fused_residual_restriction."""
import contextlib

import numpy as np

from helpers import sources_problem

NPTS = 21


@contextlib.contextmanager
def handle_pair(L, g, modes=(-1, 1), ground=None, **kw):
    """{fused_restrict: handle} on the same raster with the same options"""
    o = dict(precond_bytes=0, fixed_k=1, stream=-1)
    o.update(kw)
    hs = {}
    try:
        for m in modes:
            oo = dict(o)
            if m is not None:   # (None: the option is left at its default)
                oo["fused_restrict"] = m
            hs[m] = L.raster_setup(g, L.default_opts(**oo), ground=ground)
        yield hs
    finally:
        for h in hs.values():
            h.close()


class PathCounter:
    """fused_restrict_solves of a pair of handles from one x-carrying solve to the next"""

    def __init__(self, hs):
        self.hs = hs
        self.seen = {m: h.info["fused_restrict_solves"] for m, h in hs.items()}

    def taken(self, sts, what=""):
        """the solves just run took the fused pass on the `1` handle and two passes on the `-1` handle"""
        now = self.hs[1].info["fused_restrict_solves"]
        assert now > self.seen[1], ("fused pass not taken by a solve that carries the solution", what, now)
        self.seen[1] = now
        assert self.hs[-1].info["fused_restrict_solves"] == 0, what
        assert sts[1]["resid_fused"] == 1 and sts[-1]["resid_fused"] == 0, (what, sts[1]["resid_fused"], sts[-1]["resid_fused"])

    def not_taken(self, sts, what=""):
        for m, h in self.hs.items():
            assert h.info["fused_restrict_solves"] == self.seen[m], (what, m, h.info["fused_restrict_solves"])
            assert sts[m]["resid_fused"] == 0, (what, m)


def pair_list(pts, npairs, seed=11):
    """npairs pairs among the focal nodes, one of them with src == dst inside the first batch"""
    rng = np.random.default_rng(seed)
    k = len(pts)
    src = [int(pts[i]) for i in rng.integers(0, k, npairs)]
    dst = [int(pts[(pts.index(s_) + 1 + int(d)) % k]) for s_, d in zip(src, rng.integers(0, k - 2, npairs))]
    dst[3] = src[3]
    return src, dst


def _same_stats(a, b):
    assert a["total_iters"] == b["total_iters"], (a["total_iters"], b["total_iters"])
    assert a["max_relres"] == b["max_relres"], (a["max_relres"], b["max_relres"])
    assert a["not_converged"] == 0 and b["not_converged"] == 0


def check_pairs_voltages(L, shape, batch, check_every=1, dtype=np.float64):
    """block 1: csgpu_solve_pairs with volt_out -- resistances, the n x npairs voltages, iteration counts and the explicit
    ||Ax-b||/||b|| are the two-pass path's bit for bit (x += alpha p is the same fma on the same stored values)"""
    g, G, pts, cases = sources_problem(shape, NPTS, seed=7)
    src, dst = pair_list(pts, batch + 5)
    with handle_pair(L, g.astype(dtype), batch=batch, check_every=check_every) as hs:
        pc = PathCounter(hs)
        out, sts = {}, {}
        for m, h in hs.items():
            R, _, V, st = h.solve_pairs(src, dst, want_voltages=True)
            assert R.dtype == dtype and V.shape == (h.info["n"], batch + 5) and R[3] == 0 and np.all(V[:, 3] == 0)
            out[m], sts[m] = (R, V), st
        pc.taken(sts, ("pairs", shape, batch, check_every))
        assert np.array_equal(out[1][0], out[-1][0]), (shape, batch, check_every, np.max(np.abs(out[1][0] - out[-1][0])))
        assert np.array_equal(out[1][1], out[-1][1]), (shape, batch, check_every, np.max(np.abs(out[1][1] - out[-1][1])))
        _same_stats(sts[1], sts[-1])


def check_pairs_currents(L, shape, batch, check_every=1, dtype=np.float64, branch=False):
    """block 2: csgpu_solve_pairs_currents -- voltages, node currents, the cumulative and maximum current maps (two calls
    accumulating into the same maps), optionally the branch currents"""
    g, G, pts, cases = sources_problem(shape, NPTS, seed=7)
    npairs = batch + 5
    src, dst = pair_list(pts, npairs)
    w = (1 + np.arange(npairs) % 3).astype(np.int32)
    with handle_pair(L, g.astype(dtype), batch=batch, check_every=check_every) as hs:
        pc = PathCounter(hs)
        n = hs[1].info["n"]
        out = {}
        for call in range(2):
            sts = {}
            for m, h in hs.items():
                if call == 0:
                    out[m] = {"cum": np.full(n, 0.25, dtype=dtype), "mx": np.full(n, 1e-3, dtype=dtype)}
                r = h.solve_pairs_currents(src, dst, weights=w, want_voltages=True, want_currents=True, cum=out[m]["cum"],
                                           mx=out[m]["mx"], want_branch=branch and call == 0)
                out[m]["R"], out[m]["V"], out[m]["C"], sts[m] = r[:4]
                if branch and call == 0:
                    out[m]["B"] = r[4]
            pc.taken(sts, ("currents", shape, batch, call))
            for key in out[1]:
                assert np.array_equal(out[1][key], out[-1][key]), (shape, batch, call, key)
            _same_stats(sts[1], sts[-1])
        assert np.all(out[1]["cum"] > 0.25 - 1e-12) and np.max(out[1]["mx"]) > 1e-3


def check_rhs(L, shape, batch, ncols=21):
    """block 3: csgpu_solve_rhs with zero-mean random columns"""
    g, G, pts, cases = sources_problem(shape, NPTS, seed=7)
    rng = np.random.default_rng(17)
    B = rng.standard_normal((g.size, ncols))
    B -= B.mean(axis=0)
    with handle_pair(L, g, batch=batch, check_every=1) as hs:
        pc = PathCounter(hs)
        X, sts = {}, {}
        for m, h in hs.items():
            X[m], sts[m] = h.solve_rhs(B)
        pc.taken(sts, ("rhs", shape, batch))
        assert np.array_equal(X[1], X[-1]), (shape, batch, np.max(np.abs(X[1] - X[-1])))
        _same_stats(sts[1], sts[-1])


def check_finite_grounds(L, shape, batch):
    """block 4: a handle with finite grounds on the diagonal (csgpu_raster_setup_grounded). Without Dirichlet sets
    csgpu_solve_grounded / csgpu_solve_sources take the fused pass; WITH them (masks touch r between the update and the
    cycle) they do not, and both give the two-pass handle's bits."""
    g, G, pts, cases = sources_problem(shape, NPTS, seed=7)
    rng = np.random.default_rng(19)
    ground = 0.01 * np.exp(rng.standard_normal(shape))
    n = g.size
    with handle_pair(L, g, ground=ground, batch=batch, check_every=1) as hs:
        pc = PathCounter(hs)
        none = [[] for _ in pts]
        # one-to-all columns through csgpu_solve_grounded, all-to-one columns through csgpu_solve_sources
        src, val, gnd, chk, B = cases[0]
        out, sts = {}, {}
        for m, h in hs.items():
            X, C, st = h.solve_grounded(B, none, want_currents=True)
            out[m], sts[m] = (X, C), st
        pc.taken(sts, ("solve_grounded, no Dirichlet sets", shape, batch))
        assert np.array_equal(out[1][0], out[-1][0]) and np.array_equal(out[1][1], out[-1][1]), (shape, batch)
        _same_stats(sts[1], sts[-1])
        src, val, gnd, chk, B = cases[1]
        out, sts = {}, {}
        for m, h in hs.items():
            cum, mx = np.full(n, 0.25), np.full(n, 1e-3)
            v, X, C, st = h.solve_sources(src, none, values=val, check=pts, want_voltages=True, want_currents=True,
                                          cum=cum, mx=mx)
            out[m], sts[m] = (v, X, C, cum, mx), st
        pc.taken(sts, ("solve_sources, no Dirichlet sets", shape, batch))
        for a, b in zip(out[1], out[-1]):
            assert np.array_equal(a, b), (shape, batch)
        _same_stats(sts[1], sts[-1])
        # the same handles with Dirichlet sets: two passes on both
        out, sts = {}, {}
        for m, h in hs.items():
            X, C, st = h.solve_grounded(B, gnd, want_currents=True)
            src0, val0, gnd0, chk0, _ = cases[0]
            v, X2, _, st2 = h.solve_sources(src0, gnd0, values=val0, check=chk0, want_voltages=True)
            out[m], sts[m] = (X, C, v, X2), st
            assert st2["resid_fused"] == 0
        pc.not_taken(sts, ("Dirichlet sets", shape, batch))
        for a, b in zip(out[1], out[-1]):
            assert np.array_equal(a, b), (shape, batch)
        _same_stats(sts[1], sts[-1])


def check_mixed_precision_stays_two_pass(L, shape, batch):
    """block 6: an fp32 hierarchy under the fp64 iteration has no fused pass, whatever the option says"""
    g, G, pts, cases = sources_problem(shape, NPTS, seed=7)
    src, dst = pair_list(pts, batch + 5)
    with handle_pair(L, g, batch=batch, check_every=1, precond_bytes=4) as hs:
        pc = PathCounter(hs)
        out, sts = {}, {}
        for m, h in hs.items():
            R, _, V, st = h.solve_pairs(src, dst, want_voltages=True)
            R2, _, C, st2 = h.solve_pairs_currents(src, dst, want_currents=True)
            assert st2["resid_fused"] == 0
            out[m], sts[m] = (R, V, R2, C), st
        pc.not_taken(sts, ("mixed", shape, batch))
        assert hs[1].info["fused_restrict_solves"] == 0
        for a, b in zip(out[1], out[-1]):
            assert np.array_equal(a, b)
        _same_stats(sts[1], sts[-1])


def check_polishing(L, shape=(90, 77), batch=16, check_every=(1, 4, 3)):
    """block 7: with rtol = 1e-2 columns stop above ||r||/||b|| = 1e-4 and are re-opened on the true residual; the fused path
    then continues with the in-place two-pass update, x included, from whichever buffer the last real launch wrote"""
    g, G, pts, cases = sources_problem(shape, 12, seed=8)
    src, dst = [int(p_) for p_ in pts[:6]] * 3, [int(p_) for p_ in pts[6:]] * 3
    for ce in check_every:
        with handle_pair(L, g, batch=batch, check_every=ce, rtol=1e-2) as hs:
            pc = PathCounter(hs)
            out, sts = {}, {}
            for m, h in hs.items():
                R, _, V, st = h.solve_pairs(src, dst, want_voltages=True)
                assert st["not_converged"] == 0 and st["polished_batches"] > 0, st
                out[m], sts[m] = (R, V), st
            pc.taken(sts, ("polishing", ce))
            assert np.array_equal(out[1][0], out[-1][0]), (ce, np.max(np.abs(out[1][0] - out[-1][0])))
            assert np.array_equal(out[1][1], out[-1][1]), (ce, np.max(np.abs(out[1][1] - out[-1][1])))
            assert sts[1]["total_iters"] == sts[-1]["total_iters"]


def check_true_residual_criterion(L, shape=(80, 75), batch=16):
    """block 8: criterion = 1 reads the fused kernel's partials of r'r, which are summed in another order than the two-pass
    kernel's: same iteration counts, results to 1e-12 (the bound of helpers.check_fused_residual_restriction)"""
    g, G, pts, cases = sources_problem(shape, 12, seed=3)
    src, dst = [int(p_) for p_ in pts[:6]] * 3, [int(p_) for p_ in pts[6:]] * 3
    with handle_pair(L, g, batch=batch, check_every=1, criterion=1, rtol=1e-9) as hs:
        pc = PathCounter(hs)
        out, sts = {}, {}
        for m, h in hs.items():
            R, _, V, st = h.solve_pairs(src, dst, want_voltages=True)
            assert st["not_converged"] == 0
            out[m], sts[m] = (R, V), st
        pc.taken(sts, "true residual")
        assert sts[1]["total_iters"] == sts[-1]["total_iters"]
        assert np.max(np.abs(out[1][0] - out[-1][0]) / out[-1][0]) < 1e-12
        assert np.max(np.abs(out[1][1] - out[-1][1])) < 1e-12 * np.max(np.abs(out[-1][1]))


def check_enriched_level(L, shape=(96, 85), batch=16, frac=0.15):
    """block 9: a NODATA raster whose level 0 is enriched (set up as in helpers.check_enrichment_fused). The fused form sums
    the coarse right-hand side in another order there (enrich_coarse_fix): that helper's bounds, and the same bits from two
    set-ups of the fused handle."""
    rng = np.random.default_rng(23)
    base = np.exp(0.5 * rng.standard_normal(shape))
    g = np.where(rng.random(shape) < frac, 0.0, base)
    out, sts = {}, {}
    src = dst = None
    for fused in (-1, 1, 1):
        with L.raster_setup(g, L.default_opts(batch=batch, precond_bytes=0, enrich=0, enrich_tau=0.1, fused_restrict=fused,
                                              stream=-1, check_every=1, fixed_k=1)) as h:
            assert h.info["enrich_vectors"] > 0
            if src is None:
                labels, _ = h.components()
                big = np.flatnonzero(labels == np.bincount(labels).argmax())
                ids = np.random.default_rng(6).choice(big, size=2 * (batch + 5), replace=False)
                src, dst = [int(v) for v in ids[:batch + 5]], [int(v) for v in ids[batch + 5:]]
            R, _, V, st = h.solve_pairs(src, dst, want_voltages=True)
            assert st["not_converged"] == 0
            assert (h.info["fused_restrict_solves"] > 0) == (fused == 1), (fused, h.info["fused_restrict_solves"])
            assert st["resid_fused"] == (1 if fused == 1 else 0)
            out.setdefault(fused, []).append((R, V, st["total_iters"]))
    two, fa, fb = out[-1][0], out[1][0], out[1][1]
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2], "not reproducible across set-ups"
    assert np.max(np.abs(fa[0] - two[0]) / np.abs(two[0])) < 1e-7
    assert np.max(np.abs(fa[1] - two[1])) < 1e-7 * np.max(np.abs(two[1]))
    assert abs(fa[2] - two[2]) <= max(1, two[2] // 50), (fa[2], two[2])


def check_default_unchanged(L, shape=(64, 57), batch=16):
    """block 10: with the option unset a solve that carries the solution runs two passes, as before"""
    g, G, pts, cases = sources_problem(shape, NPTS, seed=7)
    src, dst = pair_list(pts, batch + 5)
    with handle_pair(L, g, modes=(None,), batch=batch, check_every=1) as hs:
        h = hs[None]
        _, _, V, st = h.solve_pairs(src, dst, want_voltages=True)
        assert V is not None and st["resid_fused"] == 0 and h.info["fused_restrict_solves"] == 0
        _, _, _, st = h.solve_pairs_currents(src, dst, want_currents=True)
        assert st["resid_fused"] == 0 and h.info["fused_restrict_solves"] == 0
        # (the resistance-only solve of the same handle keeps the fused pass)
        _, _, _, st = h.solve_pairs(src, dst)
        assert st["resid_fused"] == 1 and h.info["fused_restrict_solves"] > 0


def check_fused_solution_update(L, shapes=((31, 200), (64, 57), (101, 130)), batches=(16, 32), blocks=(1, 2, 3, 4),
                                check_every=(1, 4)):
    """Blocks 1 - 4 over shapes and batch widths: every check_every on the first shape (1: direct launches, where odd
    iteration counts leave r in the second buffer, 4: captured chunks), the first elsewhere; branch currents once, on the
    smallest shape."""
    smallest = min(shapes, key=lambda s: s[0] * s[1])
    for shape in shapes:
        for batch in batches:
            for ce in (check_every if shape == shapes[0] else check_every[:1]):
                if 1 in blocks:
                    check_pairs_voltages(L, shape, batch, ce)
                if 2 in blocks:
                    check_pairs_currents(L, shape, batch, ce, branch=(shape == smallest and batch == batches[0]))
            if 3 in blocks:
                check_rhs(L, shape, batch)
            if 4 in blocks:
                check_finite_grounds(L, shape, batch)
