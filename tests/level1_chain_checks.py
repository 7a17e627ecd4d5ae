"""Checks of the chained level-1 pass (csgpu_opts.fused_level1 = 2: out = x + S (b - A x) + Q2 x_c of a lattice V(2,2) level
in ONE marching pass, dia_chain_kernel in csrc/stencil.h) and of the first CG product of a batch, which is not handed the
old search direction (dia_cg_kernel with pin = nullptr). Shared by the emulator tests (test_level1_chain_emu.py) and their
device twins (test_level1_chain_gpu.py).

The chained pass gives every entry the arithmetic of the two launches it replaces, so everything a solve returns must be
EQUAL, bit for bit, whichever runs. The level-1 lattice of an R x C raster is (R+1)//3 x (C+1)//3; a workgroup of the pass
owns 14 (batch 32) or 30 (batch 16) rows of `dia_seg` raster columns in double precision."""
import numpy as np

LATTICE9 = 1  # CSGPU_FORM_LATTICE9

# (raster shape, dia_seg / restrict_seg or 0 for the defaults): what the level-1 lattice looks like to the pass
SHAPES = {
    "one_tile": ((37, 34), 0),        # 12 x 11: smaller than one tile both ways; R, C = 1 mod 3
    "many_tiles": ((301, 200), 16),   # 100 x 67: strips of 14 / 30 rows and segments of 16 columns, neither divides
    "residue0": ((63, 60), 8),        # 21 x 20; R, C = 0 mod 3
    "thin_wide": ((98, 293), 8),      # 33 x 98; R, C = 2 mod 3
    "thin_tall": ((293, 98), 8),      # 98 x 33
}


def problem(shape, seed=3, npts=10):
    rng = np.random.default_rng(seed)
    g = np.exp(rng.standard_normal(shape))
    pts = [int(q) for q in rng.choice(shape[0] * shape[1], size=npts, replace=False)]
    return g, pts


def pair_list(pts, npairs, seed):
    rng = np.random.default_rng(seed)
    src = [pts[int(i)] for i in rng.integers(0, len(pts), npairs)]
    dst = [pts[(pts.index(s) + 1 + int(k)) % len(pts)] for s, k in zip(src, rng.integers(0, len(pts) - 1, npairs))]
    return src, dst


def opts(L, batch, f1, seg=0, precond_bytes=0):
    kw = dict(batch=batch, precond_bytes=precond_bytes, check_every=1, fixed_k=1, stream=-1, lattice_level1_min_rows=100,
              tail_rows=64, fused_level1=f1)
    if seg:
        kw.update(dia_seg=seg, restrict_seg=seg)
    return L.default_opts(**kw)


def solve(L, g, o, src, dst, gather):
    with L.raster_setup(g, o) as h:
        R, ga, _, st = h.solve_pairs(src, dst, gather=gather)
        info = h.info
    assert st["not_converged"] == 0
    assert info["level_form"][1] == LATTICE9, info["level_form"][:info["levels"]]
    return R, ga, st["total_iters"], info["chained_level1_cycles"]


def check_chain_equals_two_launches(L, name, batch, modes=(1,), precond_bytes=0, dtype=np.float64):
    """fused_level1 = 2 against every value of `modes` (1: front half fused, back half in two launches; -1: four passes):
    level 1 in nine-point lattice form, the counter of chained cycles > 0 exactly for the value 2, equal resistances,
    gathered voltages and iteration counts. The pair list is longer than a batch (a short last batch follows a full one)."""
    shape, seg = SHAPES[name]
    g, pts = problem(shape)
    g = g.astype(dtype)
    src, dst = pair_list(pts, batch + 3, seed=5)
    got = solve(L, g, opts(L, batch, 2, seg, precond_bytes), src, dst, pts[:3])
    assert got[3] > 0, "the chained pass did not run"
    for m in modes:
        ref = solve(L, g, opts(L, batch, m, seg, precond_bytes), src, dst, pts[:3])
        assert ref[3] == 0, (m, ref[3])
        assert np.array_equal(got[0], ref[0]), (name, batch, m, float(np.max(np.abs(got[0] - ref[0]))))
        assert np.array_equal(got[1], ref[1]), (name, batch, m)
        assert got[2] == ref[2], (name, batch, m, got[2], ref[2])


def check_default(L, batch=32):
    """fused_level1 = 0: the chained pass is the default of a double-precision hierarchy and of no other."""
    shape, seg = SHAPES["residue0"]
    g, pts = problem(shape)
    src, dst = pair_list(pts, batch + 3, seed=2)
    for dtype, pb, chained in ((np.float64, 0, True), (np.float64, 4, False), (np.float32, 0, False)):
        got = solve(L, g.astype(dtype), opts(L, batch, 0, seg, pb), src, dst, None)
        assert (got[3] > 0) == chained, (dtype, pb, got[3])


def check_second_solve_on_a_handle(L, batch, name="residue0"):
    """A handle that has solved before holds the first solve's search direction in both p buffers; the first product of the
    next batch must not see it: results equal to those of a fresh handle given only the second pair list."""
    shape, seg = SHAPES[name]
    g, pts = problem(shape, seed=8)
    first = pair_list(pts, batch + 2, seed=1)
    second = pair_list(pts[::-1], batch + 2, seed=9)
    with L.raster_setup(g, opts(L, batch, 0, seg)) as h:
        h.solve_pairs(first[0], first[1], gather=pts[:3])
        R, ga, _, st = h.solve_pairs(second[0], second[1], gather=pts[:3])
    with L.raster_setup(g, opts(L, batch, 0, seg)) as h:
        R2, ga2, _, st2 = h.solve_pairs(second[0], second[1], gather=pts[:3])
    assert st["not_converged"] == 0 and st2["not_converged"] == 0
    assert np.array_equal(R, R2), float(np.max(np.abs(R - R2)))
    assert np.array_equal(ga, ga2) and st["total_iters"] == st2["total_iters"]
