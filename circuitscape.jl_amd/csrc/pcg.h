// pcg.h -- K6/K7/K8: AMG V-cycle application and the preconditioned-CG driver.
//
// GPU counterpart of
//   aspreconditioner(ml) / ldiv!(z, P, r): one V(nu_pre, nu_post) cycle from a zero initial guess
//       (AlgebraicMultigrid.jl __solve!, restated in SURVEY.md 2.3; reference call site src/core.jl:164,178)
//   Krylov.cg(G, curr; M, ldiv=true, rtol, itmax): src/core.jl:639, and the residual check src/core.jl:640-641.
// The smoother is damped Jacobi fused into the SpMV epilogue (symmetric, so CG theory holds); the first
// pre-smoothing sweep from the zero guess needs no matrix product at all.
#pragma once
#include <algorithm>
#include <deque>
#include <limits>
#include <type_traits>

#include "amg_setup.h"
#include "blas1.h"
#include "spmv.h"
#include "stencil.h"
#include "lattice.h"
#include "tail.h"
#include "raster.h"
#include "poly.h"
#include "enrich.h"

namespace csgpu {

template <class T>
inline void ensure_level_work(Hierarchy<T>& H, int K) {
  if (H.work_k == K) return;
  if (K <= H.work_kcap) {  // a narrower batch (the ragged tail of a pair list) runs in the buffers of the widest one: every
    H.work_k = K;          // offset inside them is computed from the K of the launch
    return;
  }
  for (size_t l = 0; l < H.levels.size(); ++l) {
    Level<T>& L = H.levels[l];
    const size_t elems = (size_t)std::max(L.A.nrows, 1) * K;
    if (l == 0 && L.lattice_two_product()) {
      // the two marching products of an index-free level read b and write out directly (n x K x 2 vectors saved: 25.6 GB
      // at 10000^2, K = 16, fp64); the generic branch of vcycle() allocates them should it ever run on this level
      L.xa.release();
      L.rb.release();
    } else {
      L.xa.alloc(elems * sizeof(T));
      L.rb.alloc(elems * sizeof(T));
    }
    L.qs.release();  // third buffer, allocated on demand by levels that run more than one post-smoothing sweep
    if (l > 0)
      L.b.alloc(2 * elems * sizeof(T));  // [0, elems): restricted rhs, [elems, 2*elems): this level's solution
    else
      L.b.release();
  }
  H.work_k = K;
  H.work_kcap = K;
}

// Jacobi sweeps per preconditioner application of a hierarchy of ONE level (see vcycle; csgpu_opts.last_level_sweeps).
// Measured on BASELINE configs[4]'s network (n = 5e6, 1.05e8 stored entries, one MI355X, profiles/r6_network_sweeps.jsonl):
// every sweep is one more pass over the matrix per iteration, and on an expander -- D^-1 A is well conditioned -- the
// iterations it saves do not pay for it: 8 sweeps 6 iterations / 113 sources/s (K = 16) and 157 (K = 32), 4: 7 / 168 / 222,
// 2: 10 / 189 / 239, 1: 12 / 216 / 256, none (plain Jacobi scaling): 20 / 202 / 219.
constexpr int kSingleLevelSweeps = 1;

// Knobs::fused_restrict resolved for a CG iteration in precision T
template <class T>
inline bool fused_restrict_wanted() {
  const int f = knobs().fused_restrict;
  return f > 0 || (f == 0 && sizeof(T) == 8);
}

// Knobs::fused_level1 = 0 resolved for the back half of a lattice V(2,2) level in precision T: the chained pass (stencil.h)
// is the default where an A/B on the device showed it winning: a double-precision hierarchy (10000^2, K = 32: 582.8 -> 569.9 ms
// of device time per batch, profiles/level1_chain_ab.json). An fp32 hierarchy and single precision have not been timed with
// it and keep the two launches (build-time A/B knob: -DCSGPU_CHAIN_L1_FP64=0)
#ifndef CSGPU_CHAIN_L1_FP64
#define CSGPU_CHAIN_L1_FP64 1
#endif
// Knobs::fused_level1 resolved for the front half (x = S b and b_c = Q2' b in one pass): 0 = on in double precision
template <class T>
inline bool fused_level1_wanted() {
  const int f = knobs().fused_level1;
  return f > 0 || (f == 0 && sizeof(T) == 8);
}
template <class T>
inline bool chained_level1_default() {
  return sizeof(T) == 8 && CSGPU_CHAIN_L1_FP64 != 0;
}

// Optional fusions at level 0 of the V-cycle.
template <class T>
struct VcycleFuse {
  bool xa_ready = false;       // level-0 first pre-smoothing sweep already written to L.xa by the caller
  const T* dotw = nullptr;     // fuse partials of dotw . out into the final post-smoothing product
  const int* skip = nullptr;   // device flag: non-zero turns every launch of the cycle into a no-op
  double* partials = nullptr;  // [spmv_grid][K]
  bool b_has_tail = false;     // level 0: the input vector b is followed by room for the level-1 solution, so the
                               // two-product form out = [S Q][b; x_c] can be used (needs L.M and V(1,1))
  bool bc_ready = false;       // lattice two-product level 0: the caller already wrote b_c = Q^T b into the level-1 right-hand
                               // side (lattice_rupd_restrict, lattice.h), the cycle skips its restriction
  const int* pair_src = nullptr;  // lattice two-product level 0, with bc_ready: b is the right-hand sides of a batch of pair
  const int* pair_dst = nullptr;  // solves and was never stored -- the second product synthesises it (DIA_SQP, stencil.h)
  int pair_cols = 0;
};

// Levels from `first` down run in one launch (tail.h) when they are small: the first level l >= 1 with at most
// 4096 rows (measured: above that one workgroup per column is slower than the launches it replaces), provided at least two
// levels are left. CSGPU_TAIL_ROWS=0 switches the tail off (A/B knob).
// what tail_first_level would decide, without deciding it (csgpu_get_info on a handle that has not solved yet)
template <class T>
inline int tail_first_level_peek(const Hierarchy<T>& H) {
  if (H.tail_first != -2) return H.tail_first;
  const int rows = knobs().tail_rows;  // (read once per hierarchy)
  const int nl = (int)H.levels.size();
  for (int l = 1; l + 1 < nl; ++l)
    if (H.levels[l].A.nrows <= rows && nl - l <= kTailMaxLevels) return l;
  return -1;
}

template <class T>
inline int tail_first_level(Hierarchy<T>& H) {
  if (H.tail_first != -2) return H.tail_first;
  const int l = H.tail_first = tail_first_level_peek(H);
  if (l >= 1 && knobs().tail_debug)
    fprintf(stderr, "csgpu: coarse tail from level %d (%d rows) of %d\n", l, H.levels[l].A.nrows, (int)H.levels.size());
  return l;
}

template <class T, int K>
inline void launch_tail(Hierarchy<T>& H, int first, const T* b, T* out, int nu_first, int nu_deep, const int* skip,
                        hipStream_t st) {
  const int nl = (int)H.levels.size();
  TailArgs<T> a;
  a.nlev = nl - first;
  a.dense = H.coarse_dense ? 1 : 0;
  const bool dirichlet = H.dir_mode != 0 && H.coarse_dense;  // DirichletCoarse (below)
  a.inv = dirichlet ? dptr<T>(H.coarse_inv_defl) : dptr<T>(H.coarse_inv);
  a.dir_cand = dirichlet ? (const T*)dptr<T>(H.coarse_cand) : nullptr;
  a.dir_comp = dirichlet ? (const int*)dptr<int>(H.coarse_comp) : nullptr;
  a.dir_coef = dirichlet ? H.dir_coef : nullptr;
  a.dir_ncomp = dirichlet ? H.dir_ncomp : 0;
  a.dir_mode = dirichlet ? H.dir_mode : 0;
  int64_t off = 0;
  for (int t = 0; t < a.nlev; ++t) {
    Level<T>& L = H.levels[first + t];
    TailLevel<T>& tl = a.lev[t];
    tl.n = L.A.nrows;
    tl.nu = (first + t == 1) ? nu_first : nu_deep;
    if (!L.weights.empty()) tl.nu = (int)L.weights.size();
    CS_REQUIRE(tl.nu <= kTailMaxSweeps, CSGPU_BAD_ARGS, "more sweeps per coarse level than the tail kernel holds weights for");
    for (int s = 0; s < kTailMaxSweeps; ++s) tl.w[s] = L.weights.empty() ? (T)L.omega : (T)L.weights[std::min<size_t>(s, L.weights.size() - 1)];
    tl.omega = (T)L.omega;
    tl.arp = L.A.rp();
    tl.aci = L.A.ci();
    tl.ava = L.A.va();
    tl.dinv = dptr<T>(L.dinv);
    tl.rrp = L.R.rp();
    tl.rci = L.R.ci();
    tl.rva = L.R.va();
    tl.has_q = L.Q.nnz > 0 ? 1 : 0;
    const Csr<T>& PQ = tl.has_q ? L.Q : L.P;
    tl.qrp = PQ.rp();
    tl.qci = PQ.ci();
    tl.qva = PQ.va();
    tl.cand = L.cand.p ? (const T*)dptr<T>(L.cand) : nullptr;
    tl.off = off;
    off += 4 * (int64_t)tl.n;
  }
  if (H.tail_k != K || H.tail_stride != off) {
    H.tail_ws.alloc((size_t)off * K * sizeof(T));
    H.tail_stride = off;
    H.tail_k = K;
  }
  // projection of the candidate out of the tail's right-hand sides: near-singular fp32 hierarchies only (A/B knob:
  // CSGPU_NO_TAIL_PROJECTION)
  // (not for Dirichlet-masked solves: their right-hand sides DO have a component along the candidate)
  a.cand_inv_norm2 = (H.near_singular && H.cand_norm2 > 0 && !dirichlet && knobs().tail_projection) ? (T)(1.0 / H.cand_norm2) : T(0);
  a.scratch = dptr<T>(H.tail_ws);
  a.stride = off;
  a.bin = b;
  a.xout = out;
  a.skip = skip;
  hipLaunchKernelGGL((coarse_tail_kernel<T, K>), dim3(K), dim3(kTailThreads), 0, st, a);
}

template <class T>
inline SpmvArgs<T> level_args(const Level<T>& L, const T* x, T* y, const int* skip = nullptr) {
  SpmvArgs<T> a = spmv_args(L.A, x, y);
  a.order = L.orderA.p ? dptr<int>(L.orderA) : nullptr;
  a.skip = skip;
  return a;
}

// out = V-cycle(b) on level l, zero initial guess. `out` must not alias b or the level's work vectors.
// Smoothing: nu_pre / nu_post damped-Jacobi sweeps on level 0, nu_coarse on every coarser level (they hold ~1/9 of
// the work each, so extra sweeps there are nearly free and cut the iteration count).
template <class T, int K>
inline void vcycle(Hierarchy<T>& H, int l, const T* b, T* out, int nu_pre0, int nu_post0, int nu_coarse,
                   hipStream_t st, const VcycleFuse<T>* fuse = nullptr) {
  Level<T>& L = H.levels[l];
  const int n = L.A.nrows;
  const bool last = (l + 1 == (int)H.levels.size());
  const int gv = grid_for((int64_t)n * K);
  // Level 1 gets nu_coarse sweeps, the levels below it one more: they hold 1/81 of the fine level's work and the extra
  // sweep saves an iteration of the slowest column (measured at 10000^2, profiles/r2_sweeps_per_level.json: level 1 with
  // one sweep costs 2 iterations whatever the deeper levels do). Experiment knobs: CSGPU_NU_L1, CSGPU_NU_DEEP.
  const int nu_l1 = knobs().nu_l1, nu_deep = knobs().nu_deep;
  const int nu_lvl = l == 1 ? (nu_l1 > 0 ? nu_l1 : nu_coarse) : (nu_deep > 0 ? nu_deep : nu_coarse + 1);
  // Chebyshev levels (amg_setup.h): one weight per sweep, fixed at setup; the sweep count is the polynomial's degree
  const bool cheb = l >= 1 && !L.weights.empty();
  const int nu_pre = l == 0 ? nu_pre0 : (cheb ? (int)L.weights.size() : nu_lvl);
  const int nu_post = l == 0 ? nu_post0 : (cheb ? (int)L.weights.size() : nu_lvl);
  auto weight = [&](int sweep) { return cheb ? (T)L.weights[sweep] : (T)L.omega; };
  const bool want_dot = fuse && fuse->dotw && l == 0;
  const int* skip = fuse ? fuse->skip : nullptr;
  auto dot_with_out = [&]() {  // partials of dotw . out by a launch of its own: a last product that cannot carry them
    hipLaunchKernelGGL((dot_kernel<T, K, false>), dim3(spmv_grid<T, K>(n)), dim3(256), 0, st, (int64_t)n, fuse->dotw,
                       (const T*)out, fuse->partials, (const T*)nullptr, (const T*)nullptr, (double*)nullptr);
  };
  if (l >= 1 && l == tail_first_level(H)) {
    const int nu1 = nu_l1 > 0 ? nu_l1 : nu_coarse, nud = nu_deep > 0 ? nu_deep : nu_coarse + 1;
    launch_tail<T, K>(H, l, b, out, nu1, nud, skip, st);
    return;
  }
  if (last && H.coarse_dense) {
    const bool dirichlet = H.dir_mode != 0;
    hipLaunchKernelGGL((dense_apply_kernel<T, K>), dim3(gv), dim3(256), 0, st, n,
                       dirichlet ? dptr<T>(H.coarse_inv_defl) : dptr<T>(H.coarse_inv), b, out, skip);
    if (dirichlet)
      hipLaunchKernelGGL((dense_dirichlet_kernel<T, K>), dim3(K), dim3(256), 0, st, n, (const T*)dptr<T>(H.coarse_cand),
                         (const int*)dptr<int>(H.coarse_comp), H.dir_ncomp, H.dir_coef, H.dir_mode, b, out, skip);
    if (want_dot) dot_with_out();
    return;
  }
  if (!(l == 0 && fuse && fuse->b_has_tail && nu_pre == 1 && nu_post == 1 && L.two_product()) &&
      (L.xa.bytes < (size_t)n * K * sizeof(T) || L.rb.bytes < (size_t)n * K * sizeof(T))) {
    CS_REQUIRE(L.A.nnz > 0 || last, CSGPU_INTERNAL, "generic V-cycle branch on a level without a CSR matrix");
    L.xa.alloc((size_t)n * K * sizeof(T));  // (level 0 of an index-free hierarchy running the generic branch)
    L.rb.alloc((size_t)n * K * sizeof(T));
  }
  T* cur = dptr<T>(L.xa);
  T* oth = dptr<T>(L.rb);
  const T omega = (T)L.omega;
  const bool use25 = K >= 8 && L.A25.n == n && n > 0;  // refined-tile lattice level: index-free products with A (dia25.h)
  constexpr int K25 = K >= 8 ? K : 8;                  // (the 25-point kernels exist from that batch width up)
  auto jacobi_sweep = [&](const T* xin, T* xout, bool dot, int sweep = 0) {
    if (use25 && !dot) {
      dia25_launch<T, K25>(L.A25, D25_JACOBI, xin, xout, b, (const T*)dptr<T>(L.dinv), weight(sweep), skip, st);
      return;
    }
    SpmvArgs<T> a = level_args(L, xin, xout, skip);
    a.b = b;
    a.dinv = dptr<T>(L.dinv);
    a.omega = weight(sweep);
    if (dot) {
      a.dotw = fuse->dotw;
      a.partials = fuse->partials;
    }
    spmv_launch<T, K>(a, EPI_JACOBI, dot, st);
  };
  if (last) {
    // coarsest level too large for a dense inverse: a fixed number of damped-Jacobi sweeps
    hipLaunchKernelGGL((scale_dinv_kernel<T, K>), dim3(gv), dim3(256), 0, st, (int64_t)n, cur, b, dptr<T>(L.dinv), omega, skip);
    // (a hierarchy of ONE level -- a graph the set-up declines to coarsen, BASELINE configs[4] -- is polynomial-preconditioned
    // CG: every sweep is one more pass over the matrix per iteration; Knobs::last_level_sweeps, 0 = the Jacobi scaling alone)
    const int want = knobs().last_level_sweeps;
    const int sweeps = want == 0 ? (H.levels.size() == 1 ? kSingleLevelSweeps : 8) : std::max(want, 0);
    if (sweeps <= 0) {
      hipLaunchKernelGGL((scale_dinv_kernel<T, K>), dim3(gv), dim3(256), 0, st, (int64_t)n, out, b, dptr<T>(L.dinv), omega, skip);
      if (want_dot) dot_with_out();
      return;
    }
    for (int s = 0; s < sweeps; ++s) {
      const bool fin = (s + 1 == sweeps);
      jacobi_sweep(cur, fin ? out : oth, fin && want_dot);
      std::swap(cur, oth);
    }
    return;
  }
  // the next level: its right-hand side, its solution behind it, its cycle
  Level<T>& Lc = H.levels[l + 1];
  T* bc = dptr<T>(Lc.b);
  T* xc = bc + (size_t)std::max(Lc.A.nrows, 1) * K;
  auto coarse_cycle = [&](const T* bcoarse, T* xcoarse) {
    VcycleFuse<T> cf;
    cf.skip = skip;
    vcycle<T, K>(H, l + 1, bcoarse, xcoarse, nu_pre0, nu_post0, nu_coarse, st, &cf);
  };
  if (l == 0 && fuse && fuse->b_has_tail && nu_pre == 1 && nu_post == 1 && L.two_product()) {
    // two-product form of the level (build_sq_kernel): b_c = Q^T b ; x_c = coarse(b_c) ; out = [S Q][b; x_c]
    xc = const_cast<T*>(b) + (size_t)n * K;
    if (L.lattice_two_product()) {
      if (!fuse->bc_ready) lattice_restrict<T, K>(L.Ql, b, bc, skip, st);  // index-free Q^T b (lattice.h)
    } else {
      SpmvArgs<T> a = spmv_args(L.QT, b, bc);
      a.skip = skip;
      a.order_lr = L.orderQT.p ? dptr<int>(L.orderQT) : nullptr;
      spmv_launch<T, K>(a, EPI_PLAIN, false, st);
    }
    coarse_cycle(bc, xc);
    if (want_dot) CS_REQUIRE(fuse->dotw == b, CSGPU_INTERNAL, "two-product level: fused dot must be with the input vector");
    if (L.lattice_two_product()) {
      // S in lattice form + index-free Q, one marching kernel (stencil.h); partials of b'out always written
      dia_sq_product<T, K>(L.Sdia, L.Ql, b, (const T*)xc, out, fuse->partials, skip, st, (const T*)nullptr,
                           fuse->bc_ready ? fuse->pair_src : nullptr, fuse->pair_dst, fuse->pair_cols);
      return;
    }
    SpmvArgs<T> a = spmv_args(L.M, b, out);
    a.order = L.orderA.p ? dptr<int>(L.orderA) : nullptr;
    a.skip = skip;
    if (want_dot) {
      a.dotw = nullptr;  // dot with x itself (captured at the diagonal entry of S)
      a.partials = fuse->partials;
    }
    spmv_launch_wide<T, K>(a, want_dot, st);
    return;
  }
  if (l >= 1 && L.lattice_v22() && nu_pre == 2 && nu_post == 2) {
    // lattice form of the level (lattice_level1_setup, lattice_setup.h): four marching products, no column index
    // x = S b (the two pre-sweeps) and b_c = Q2' b (residual + restriction): one pass over b, or two
    const int f1 = knobs().fused_level1;
    if (!(fused_level1_wanted<T>() && lattice_apply_restrict<T, K>(L.Sdia, L.Ql, b, cur, bc, skip, st))) {
      dia_apply<T, K>(L.Sdia, b, cur, (const T*)nullptr, skip, st);
      lattice_restrict<T, K>(L.Ql, b, bc, skip, st);
    }
    coarse_cycle(bc, xc);
    // out = x + S (b - A x) + Q2 x_c (residual, prolongation + post-sweeps): one chained pass that keeps t = b - A x on chip
    // (stencil.h; fused_level1 = 2), or two launches with t stored
    if ((f1 >= 2 || (f1 == 0 && chained_level1_default<T>())) &&
        dia_chain_product<T, K>(L.Adia, L.Sdia, L.Ql, b, (const T*)cur, (const T*)xc, out, skip, st)) {
      ++H.chained_level1_cycles;
      return;
    }
    dia_apply<T, K>(L.Adia, (const T*)cur, oth, b, skip, st);       // t = b - A x
    dia_sq_product<T, K>(L.Sdia, L.Ql, (const T*)oth, (const T*)xc, out, (double*)nullptr, skip, st, (const T*)cur);
    return;                                                         // out = x + S t + Q2 x_c
  }
  // pre-smoothing (first sweep from x = 0 is a scaling)
  if (nu_pre >= 1) {
    int s_first = 1;
    const bool no_j0 = !knobs().dia25_fused_j0;  // A/B knob
    if (use25 && nu_pre >= 2 && !no_j0 && !(fuse && fuse->xa_ready && l == 0)) {
      // 25-point lattice level: the sweep from zero and the first real sweep in one marching pass (dia25.h, JACOBI0)
      dia25_launch<T, K25>(L.A25, D25_JACOBI0, (const T*)nullptr, oth, b, (const T*)dptr<T>(L.dinv), weight(1), skip, st, omega);
      std::swap(cur, oth);
      s_first = 2;
    } else if (!(fuse && fuse->xa_ready && l == 0)) {
      hipLaunchKernelGGL((scale_dinv_kernel<T, K>), dim3(gv), dim3(256), 0, st, (int64_t)n, cur, b, dptr<T>(L.dinv), omega, skip);
    }
    for (int s = s_first; s < nu_pre; ++s) {
      jacobi_sweep(cur, oth, false, s);
      std::swap(cur, oth);
    }
  } else {
    CS_HIP(hipMemsetAsync(cur, 0, (size_t)n * K * sizeof(T), st));
  }
  // residual r = b - A x  -> oth
  if (use25) {
    dia25_launch<T, K25>(L.A25, D25_RESID, (const T*)cur, oth, b, (const T*)nullptr, T(0), skip, st);
  } else {
    SpmvArgs<T> a = level_args(L, (const T*)cur, oth, skip);
    a.b = b;
    spmv_launch<T, K>(a, EPI_RESID, false, st);
  }
  // restrict: b_{l+1} = R r
  {
    SpmvArgs<T> a = spmv_args(L.R, (const T*)oth, bc);
    a.skip = skip;
    spmv_launch<T, K>(a, EPI_PLAIN, false, st);
  }
  coarse_cycle(bc, xc);
  if (nu_post >= 1 && L.Q.nnz > 0) {
    // fused prolongation + first post-smoothing sweep: x' = x + omega D^-1 r + Q xc   (r = b - A x is still in `oth`)
    const bool fin = (nu_post == 1);
    SpmvArgs<T> a = spmv_args(L.Q, (const T*)xc, out);
    a.skip = skip;
    a.xadd = cur;
    a.b = oth;
    a.dinv = dptr<T>(L.dinv);
    a.omega = omega;
    if (fin && want_dot) {
      a.dotw = fuse->dotw;
      a.partials = fuse->partials;
    }
    if (fin) {
      spmv_launch<T, K>(a, EPI_QADD, want_dot, st);
    } else {
      // result must not overwrite `cur` or `oth` while they are read: use the level's third buffer
      if (L.qs.bytes < (size_t)n * K * sizeof(T)) L.qs.alloc((size_t)n * K * sizeof(T));
      a.y = dptr<T>(L.qs);
      spmv_launch<T, K>(a, EPI_QADD, false, st);
      T* x2 = dptr<T>(L.qs);
      // remaining sweeps ping-pong between x2/cur (oth is free now)
      T* src = x2;
      T* spare = cur;
      for (int s2 = 1; s2 < nu_post; ++s2) {
        const bool last_sweep = (s2 + 1 == nu_post);
        T* d2 = last_sweep ? out : spare;
        jacobi_sweep(src, d2, last_sweep && want_dot, s2);
        spare = src;
        src = d2;
      }
    }
    return;
  }
  // prolongate and correct in place: x += P xc
  {
    SpmvArgs<T> a = spmv_args(L.P, (const T*)xc, cur);
    a.skip = skip;
    a.xadd = cur;
    spmv_launch<T, K>(a, EPI_ADD, false, st);
  }
  // post-smoothing; the last sweep writes straight into `out` (with the fused dot partials on level 0)
  if (nu_post >= 1) {
    for (int s = 0; s < nu_post; ++s) {
      const bool fin = (s + 1 == nu_post);
      jacobi_sweep(cur, fin ? out : oth, fin && want_dot, s);
      std::swap(cur, oth);
    }
  } else {
    CS_HIP(hipMemcpyAsync(out, cur, (size_t)n * K * sizeof(T), hipMemcpyDeviceToDevice, st));
    if (want_dot) dot_with_out();
  }
}

struct PcgParams {
  double rtol = 1e-6;
  double atol = -1.0;
  int criterion = CSGPU_CRIT_KRYLOV;
  int itmax = 100000;
  int check_every = 4;
  int nu_pre = 1, nu_post = 1, nu_coarse = 3;
  int use_graph = 0;  // 0 = auto (small problems, where launch latency dominates), 1 = always, -1 = never
  // true: the whole solution vector is carried (x += alpha p over all n rows, fused into the r-update) and the
  // reference's post-check (core.jl:640) is evaluated as ||A x - b|| / ||b|| with one extra product.
  // false: only the focal entries listed in PcgWork::fnode are accumulated (resistance-only pair solves consume
  // nothing else: core.jl:231-232, 685-703) and the post-check uses the fp64 recurrence residual r (= b - A x up to
  // rounding: x and r are updated with the same alpha and the same stored p).
  bool need_x = true;
  // true: the caller wrote the right-hand side straight into PcgWork::r (W.b is not valid); only with need_x == false
  // (nothing after the set-up of r0 = b reads b on that path)
  bool rhs_in_r = false;
  // with rhs_in_r: the caller also wrote the preconditioner-precision copy (PcgWork::rp) and knows ||b||^2 of every
  // column (pair right-hand sides: 2, or 0 when src == dst) -- saves a conversion pass and a reduction pass over n x K
  bool rp_ready = false;
  const double* bb_host = nullptr;  // kMaxK values, valid until pcg_solve returns
  // with rhs_in_r: INSTEAD of writing r the caller may hand over the batch's pairs (device arrays, one node id per column;
  // columns >= pair_cols have a zero right-hand side, and so have pairs whose nodes coincide). pcg_solve then writes
  // r0 = e_dst - e_src itself (and the copy in the preconditioner's precision) -- or, on the fused lattice path, never
  // materialises it: the first restriction is a scatter of <= 18 entries per column, the first second-product and the first
  // residual update synthesise it (Knobs::sparse_init; 3 passes over n x K values saved per batch)
  const int* pair_src = nullptr;
  const int* pair_dst = nullptr;
  int pair_cols = 0;
  // Block-diagonal systems (K = 1, one PCG over many components): component label per node and the number of
  // components. When set, the post-check is the WORST component's ||A x - b|| / ||b|| (the reference checks every
  // component's solve separately, advanced.jl:186-312 -> core.jl:640).
  const int* comp_label = nullptr;
  int ncomp = 0;
  // Per-column Dirichlet sets (device arrays: gptr[K+1] offsets into gidx, total = number of grounded entries of the
  // batch): the solve runs on the system with those rows / columns removed, x = 0 there (mask_grounds_kernel).
  const int* gptr = nullptr;
  const int* gidx = nullptr;
  int gtotal = 0;
  // Rasters with short-circuit polygons on the lattice path (poly.h): PCG in the subspace of the vectors that are
  // constant on every polygon -- r and z are projected (averaged over each polygon's cells) after every update.
  const PolyProj* proj = nullptr;
  // need_x on a handle with a lattice form: the explicit post-check takes b - A x from the lattice form (dia_apply) instead of
  // the CSR product, so the solve touches no CSR array at all (csgpu_opts.lattice_maps). Solves without Dirichlet sets and
  // without a projection only; every other solve ignores it.
  bool lattice_check = false;
};

// One captured chunk of `check_every` PCG iterations. Kernel arguments are baked in at capture time, so a graph is
// only valid for the buffers and parameters it was captured with: the key holds every value that reaches a kernel
// argument and is not a pointer owned by PcgWork / the hierarchy (those invalidate the cache when they are
// reallocated).
struct PcgGraphKey {
  int K = 0, ncols_active = 0, criterion = 0, nu_pre = 0, nu_post = 0, nu_coarse = 0, iters = 0;
  double rtol = 0, atol = 0;
  const void* matrix = nullptr;
  int need_x = 0, nf = 0, parity = 0;
  int fused = 0;  // the chunk's residual update is the fused pass (a polishing phase continues two-pass in the same buffers)
  // Dirichlet sets of the batch: the list pointers and the launch geometry of the mask kernels are baked into a chunk
  const void* gptr = nullptr;
  const void* gidx = nullptr;
  int gtotal = 0;
  const void* proj = nullptr;  // member lists of a polygon handle (poly.h)
  bool operator==(const PcgGraphKey& o) const {
    return K == o.K && ncols_active == o.ncols_active && criterion == o.criterion && nu_pre == o.nu_pre &&
           nu_post == o.nu_post && nu_coarse == o.nu_coarse && iters == o.iters && rtol == o.rtol && atol == o.atol &&
           matrix == o.matrix && need_x == o.need_x && nf == o.nf && parity == o.parity && fused == o.fused && gptr == o.gptr &&
           gidx == o.gidx && gtotal == o.gtotal && proj == o.proj;
  }
};

static const int kEnrichRows = 256;  // = kEnrichParts of enrich.h: extra rows of part_a

struct Event {  // (owned: nothing leaks when a CS_REQUIRE or CS_HIP throws)
  hipEvent_t e = nullptr;
  Event() { CS_HIP(hipEventCreate(&e)); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { hipEventDestroy(e); }
};

// Event pairs around launches: grows on demand. PcgWork keeps one per kind of timed launch; a solve's own (one pair around
// all of it) lives and dies with the call.
struct LaunchTimer {
  std::deque<Event> ev;
  void begin(int slot, hipStream_t st) {
    while ((int)ev.size() < 2 * (slot + 1)) ev.emplace_back();
    CS_HIP(hipEventRecord(ev[2 * slot].e, st));
  }
  void end(int slot, hipStream_t st) { CS_HIP(hipEventRecord(ev[2 * slot + 1].e, st)); }
  double sum_ms(int counted) const {  // of the first `counted` pairs
    double ms = 0;
    for (int t = 0; t < counted; ++t) {
      float m = 0;
      CS_HIP(hipEventElapsedTime(&m, ev[2 * t].e, ev[2 * t + 1].e));
      ms += m;
    }
    return ms;
  }
};

// T = precision of the CG iteration (matrix seen by CG, x, r, p, Ap); TP = precision of the AMG hierarchy and of
// everything inside the V-cycle (TP == T, or TP = float under T = double: "fp32 preconditioner").
template <class T, class TP>
struct PcgWork {
  int K = 0;
  int Kcap = 0;               // batch width the buffers were allocated for (>= K: a narrower batch reuses them, see ensure)
  int64_t n = 0;
  DBuf x, r, Ap, b;           // T
  DBuf p;                     // TP: search direction (x and r are updated with exactly these stored values, so the
                              // invariant r = b - A x holds in T precision whatever p's storage precision)
  DBuf z, rp;                 // TP: preconditioned residual; TP copy of r (aliases r when TP == T)
  DBuf p2;                    // TP: second search-direction buffer (stencil path: p = z + beta p is fused into the
                              // product and must not overwrite values neighbouring workgroups still read)
  DBuf r2;                    // T: second residual buffer (with the tail) of the fused residual update + restriction, which
                              // recomputes halo rows from the old residual and so cannot update in place (lattice.h)
  DBuf fnode, xf;             // focal mode (PcgParams::need_x == false): nf node ids, solution values [nf][K] (T)
  int nf = 0;
  bool have_x = false;        // x holds the solution of the last solve (need_x was set)
  bool r2_oom_said = false;   // (verbose: the two-pass fallback of an x-carrying solve without room for r2 was reported)
  DBuf scalars;               // CgScalars
  DBuf dir_coef;              // [kMaxDirComp][kMaxK] doubles: 1 / G of a Dirichlet-masked solve (DirichletCoarse in pcg_solve)
  DBuf part_a, part_b, part_c;
  DBuf part_ca, part_cc;      // collapsed copies of part_a / part_c (collapse_partials_kernel)
  DBuf part_cb;               // collapsed copy of part_b (streaming solves: ||r||^2 of every iteration)
  LaunchTimer ev;   // around the CG SpMV launches
  LaunchTimer ev2;  // ... and around the residual-update launches of the same iterations
  std::vector<std::pair<PcgGraphKey, hipGraphExec_t>> graphs;  // captured iteration chunks
  bool graph_broken = false;                                   // capture failed once: stay on direct launches
  void drop_graphs() {
    for (auto& g : graphs) hipGraphExecDestroy(g.second);
    graphs.clear();
  }
  int64_t tail = 0;
  // tail_rows: rows of the level-1 solution kept right behind the V-cycle's input vector (rp, or r when TP == T)
  void ensure(int64_t n_, int K_, int64_t tail_rows = 0) {
    if (n == n_ && K == K_ && tail == tail_rows) return;
    drop_graphs();
    if (n == n_ && tail == tail_rows && K_ <= Kcap) {
      // the arena of the widest batch serves a narrower one as it is (sizes are monotone in K, offsets are computed from
      // the K of the launch): the short last batch of a pair list runs at ITS width without an allocation
      K = K_;
      return;
    }
    n = n_;
    K = K_;
    Kcap = K_;
    tail = tail_rows;
    const size_t bytes = (size_t)n * K * sizeof(T);
    constexpr bool SAME = std::is_same<T, TP>::value;
    x.release();  // allocated by the first solve that needs the whole solution vector
    p2.release();
    r2.release();
    r.alloc(bytes + (SAME ? (size_t)tail * K * sizeof(T) : 0));
    p.alloc((size_t)n * K * sizeof(TP));
    Ap.release();  // A p is stored only when the residual update does not recompute it, b only when the caller hands the
    b.release();   // right-hand side over in it: both allocated on first need (need_vec) -- 2 x n x K x sizeof(T) saved on
                   // the resistance-only lattice path
    z.alloc((size_t)n * K * sizeof(TP));
    if (!SAME) rp.alloc((size_t)(n + tail) * K * sizeof(TP));
    scalars.alloc(sizeof(CgScalars));
    // one row of kMaxK partials per workgroup of the largest launch: spmv_grid() and grid_for() (<= kMaxGrid)
    // (+ kEnrichRows: the r'z correction rows of enrich.h sit behind the V-cycle's own in part_a)
    const size_t pb = (std::max<size_t>(16384, spmv_grid_upper(n)) + kEnrichRows) * kMaxK * sizeof(double);
    part_a.alloc(pb);
    part_b.alloc(pb);
    part_c.alloc(pb);
    part_ca.alloc((size_t)kCollapsedParts * kMaxK * sizeof(double));
    part_cc.alloc((size_t)kCollapsedParts * kMaxK * sizeof(double));
  }
  // b / Ap / x on demand (see ensure); p2 with the element size of TP
  T* need_vec(DBuf& v, size_t elem = sizeof(T)) {
    const size_t bytes = (size_t)n * K * elem;
    if (v.bytes < bytes) {
      drop_graphs();
      v.alloc(bytes);
    }
    return (T*)v.p;
  }
  T* rhs() { return need_vec(b); }
  // focal nodes of the next solve (host ids); values land in xf[m*K + c]
  void set_focal(const std::vector<int>& nodes, hipStream_t st) {
    nf = (int)nodes.size();
    const size_t cap = std::max<size_t>(nodes.size(), 64);
    if (fnode.bytes < cap * sizeof(int) || xf.bytes < cap * K * sizeof(T)) {
      drop_graphs();  // captured launches hold the old pointers
      fnode.alloc(2 * cap * sizeof(int));
      xf.alloc(2 * cap * K * sizeof(T));
    }
    if (nf > 0) {
      CS_HIP(hipMemcpyAsync(fnode.p, nodes.data(), nodes.size() * sizeof(int), hipMemcpyHostToDevice, st));
      CS_HIP(hipStreamSynchronize(st));
    }
  }
  ~PcgWork() { drop_graphs(); }
};

struct PcgBatchResult {
  CgScalars s;
  double device_ms = 0;
  double spmv_ms = 0;
  int64_t spmv_calls = 0;
  int64_t graph_launches = 0;
  int polished = 0;
  int64_t spmv_bytes = 0;  // algorithmic bytes of one of the timed CG-product launches
  double resid_ms = 0;     // the residual-update launches (with the restriction, on the fused path) of the same iterations
  int64_t resid_calls = 0, resid_bytes = 0;
  int resid_fused = 0;
  int lattice_check = 0;   // 1 = the explicit post-check took b - A x from the lattice form (PcgParams::lattice_check)
  bool explicit_relres = false;  // s.relres is ||A x - b|| / ||b|| of an explicit product (x carried), not the recurrence residual
};

// The coarse-space enrichment (enrich.h) wraps the V-cycle of the lattice two-product level only; polygon handles
// (`projected`) do not use it. ONE predicate for the batch and the streaming loops.
template <class TP>
inline bool enrich_applicable(const Enrich& EN, int64_t n, bool lattice_two_product_path, bool projected) {
  return lattice_two_product_path && !projected && EN.nvec > 0 && EN.n == n && EN.phi_bytes == (int)sizeof(TP);
}

// Acceptance of one column (the reference's only test is the residual, src/core.jl:639-641). When the figure is the fp64
// RECURRENCE residual (resistance-only solves carry no x) and the column did not stop on the rule -- breakdown of the
// recurrence, itmax: exactly the stagnation cases in which the recurrence may have drifted from b - A x -- it is
// accepted only with two decades of margin.
inline bool column_accepted(double relres, int done, bool explicit_relres) {
  if (!(relres < 1e-4)) return false;
  if (!explicit_relres && done != 1 && !(relres < 1e-6)) return false;
  return true;
}

// ---- pieces the batch loop (pcg_solve) and the streaming loop (pcg_stream_pairs) share ---------------------------------

// The resolved pointers of a PcgWork.
template <class T, class TP>
struct PcgPtrs {
  T* r = nullptr;                    // W.r: buffer 0 of the residual ping-pong
  TP* pbuf[2] = {nullptr, nullptr};  // search direction (stencil path: ping-pong; CSR path: one buffer twice)
  TP *z = nullptr, *rp = nullptr;    // rp: the residual in the V-cycle's precision (aliases r when TP == T)
  CgScalars* S = nullptr;
  double *pa = nullptr, *pb = nullptr, *pc = nullptr;  // partial rows: r'z, r'r, p'Ap
  // partial rows of the big SpMM-shaped launches are collapsed before the single-workgroup scalar kernels read them
  double *pac = nullptr, *pcc = nullptr;
  double atol = 0;
  int collapse_min = 0;  // (Knobs::collapse_min: test knob, so that a test can exercise the path on a small problem)
};

template <class T, class TP>
inline PcgPtrs<T, TP> pcg_ptrs(PcgWork<T, TP>& W, const PcgParams& pp, bool second_p) {
  if (second_p) W.need_vec(W.p2, sizeof(TP));
  PcgPtrs<T, TP> w;
  w.r = dptr<T>(W.r);
  w.pbuf[0] = dptr<TP>(W.p);
  w.pbuf[1] = second_p ? dptr<TP>(W.p2) : dptr<TP>(W.p);
  w.z = dptr<TP>(W.z);
  w.rp = std::is_same<T, TP>::value ? (TP*)w.r : dptr<TP>(W.rp);
  w.S = dptr<CgScalars>(W.scalars);
  w.pa = dptr<double>(W.part_a);
  w.pb = dptr<double>(W.part_b);
  w.pc = dptr<double>(W.part_c);
  w.pac = dptr<double>(W.part_ca);
  w.pcc = dptr<double>(W.part_cc);
  w.atol = pp.atol < 0 ? std::sqrt((double)std::numeric_limits<T>::epsilon()) : pp.atol;
  w.collapse_min = knobs().collapse_min >= 0 ? (int)std::max<int64_t>(1, knobs().collapse_min) : 4 * kCollapsedParts;
  return w;
}

// the rows a scalar kernel reads: `src` itself, or its collapsed copy in `dst`
template <int K>
inline std::pair<const double*, int> collapse_partials(double* src, int nparts, double* dst, int collapse_min, hipStream_t st) {
  if (nparts <= collapse_min) return {src, nparts};
  hipLaunchKernelGGL((collapse_partials_kernel<K>), dim3(ceil_div(kCollapsedParts * K, 256)), dim3(256), 0, st,
                     (const double*)src, nparts, dst);
  return {dst, kCollapsedParts};
}

// Fused residual update + restriction (lattice.h, Knobs::fused_restrict): r_new = r - alpha A p and b_c = Q^T r_new in one
// pass. The residual then ping-pongs between W.r and W.r2: the loops flip() after every fused launch, and which buffer holds
// the current residual is part of the graph key. A two-pass solve stays in buffer 0.
template <class T, class TP>
struct ResidualPingPong {
  T* rbuf[2] = {nullptr, nullptr};
  TP* copy = nullptr;  // TP != T: the residual's copy in the preconditioner's precision (one buffer: such solves never flip)
  int sel = 0;
  T* cur() const { return rbuf[sel]; }
  TP* cur_p() const {  // the V-cycle's input, and the vector its fused dot is taken with (apply_preconditioner)
    if constexpr (std::is_same<T, TP>::value) return rbuf[sel]; else return copy;
  }
  T* next() const { return rbuf[sel ^ 1]; }
  void flip() { sel ^= 1; }
  void select(int i) { sel = i; }
  int snapshot() const { return sel; }  // capturing a chunk executes nothing: the flips it made on the host are undone
  void restore(int s) { sel = s; }
  // Launches enqueued after the last column stopped returned without writing (device flag), yet each flipped on the host:
  // the residual is in the buffer the last REAL update wrote -- update number `real` = max_c iters[c] of this solve (buffer 0
  // holds r_0).
  void rewind_to_update(int real) { select(real & 1); }
};

// Which solves take the fused pass. One precision only (the V-cycle reads r itself), solves without masks or projections
// (which touch r between the update and the cycle). An ENRICHED level takes it when the set-up built W = Q'AE
// (EN.ntouch > 0): enrich_pre changes r on its halo cells after the pass has restricted it, and enrich_coarse_fix applies
// the restriction's share of that change to b_c (enrich.h). A solve that carries the whole solution takes it only when asked
// to (Knobs::fused_restrict = 1): the pass then also runs x += alpha p on the cells it owns (the XUP form of the kernel), and
// W.r2 comes ON TOP of x, b and A p -- the default leaves such a solve's device memory as it was.
// Returns the rows of r'r partials a launch of the pass writes (one per workgroup) once the second residual buffer (with the
// tail) exists, 0 = the solve runs two passes. `release_unused`: give a buffer an earlier solve left back first (a solve that
// carries x, b and A p).
template <class T, class TP, int K>
inline int acquire_fused_residual(Hierarchy<TP>& H, PcgWork<T, TP>& W, const PcgParams& pp, int64_t n, bool enrich, bool recompute,
                                  bool lattice_two_product, bool need_x, bool masked, bool release_unused) {
  int rows = 0;
  if constexpr (std::is_same<T, TP>::value && lattice_rupd_restrict_fits<T, K>()) {
    bool fused = fused_restrict_wanted<T>() && recompute && lattice_two_product && (!need_x || knobs().fused_restrict > 0) &&
                 !masked && (!enrich || H.enr.ntouch > 0) && pp.nu_pre == 1 && pp.nu_post == 1;
    const size_t want = ((size_t)n + (size_t)W.tail) * K * sizeof(T);
    if (fused && W.r2.bytes < want) {
      W.drop_graphs();
      try {
        W.r2.alloc(want);
      } catch (const Error& e) {
        // the extra n x K buffer of a solve that works without it: out of memory here is no failure of the call
        if (!need_x || e.code != CSGPU_OOM) throw;
        (void)hipGetLastError();
        W.r2.release();
        fused = false;
        if (knobs().verbose && !W.r2_oom_said) {
          W.r2_oom_said = true;
          fprintf(stderr, "csgpu: fused residual update + restriction: no memory for the second residual buffer of a "
                          "solve that carries the solution, two passes instead\n");
        }
      }
    }
    if (fused) {
      int a_, b_, c_;
      rows = lattice_rupd_restrict_grid<T, K>(H.levels[0].Ql, a_, b_, c_);
      ++H.fused_restrict_solves;
    }
  }
  if (rows == 0 && release_unused && W.r2.p) {
    W.drop_graphs();
    W.r2.release();
  }
  return rows;
}

// work vectors of the enrichment for this batch width
template <class TP, int K, class Work>
inline void enrich_prepare(Enrich& EN, Work& W) {
  if (EN.work_k == K && EN.work_bytes == (int)sizeof(TP)) return;
  W.drop_graphs();  // (captured chunks hold the old work pointers)
  enrich_ensure_work<TP, K>(EN);
}

// z = M^-1 r (r in its V-cycle precision), partials of r'z in fuse.partials. `enrich`: second coarse function on the badly
// shaped aggregates of a perforated raster lattice (enrich.h): a symmetric multiplicative correction around the V-cycle; its
// r'z terms travel as kEnrichParts extra rows behind the V-cycle's own `spmv_gp`. Every launch looks at fuse.skip.
template <class T, class TP, int K>
inline void apply_preconditioner(Hierarchy<TP>& H, const PcgParams& pp, VcycleFuse<TP>& fuse, const ResidualPingPong<T, TP>& rr,
                                 TP* z, bool enrich, int spmv_gp, hipStream_t st) {
  constexpr bool SAME = std::is_same<T, TP>::value;
  TP* rp = rr.cur_p();
  fuse.dotw = rp;
  if (enrich) enrich_pre<TP, K, SAME>(H.enr, rp, fuse.skip, st);
  // (the fused pass restricted r as the update left it: the pre-pass's change of r follows on the coarse side)
  if (enrich && fuse.bc_ready) enrich_coarse_fix<TP, K>(H.enr, dptr<TP>(H.levels[1].b), fuse.skip, st);
  vcycle<TP, K>(H, 0, rp, z, pp.nu_pre, pp.nu_post, pp.nu_coarse, st, &fuse);
  if (enrich) enrich_post<TP, K, SAME>(H.enr, rp, z, fuse.partials + (size_t)spmv_gp * K, fuse.skip, st);
}

// ---- the batch solve -----------------------------------------------------------------------------------------------------
// Every path decision of one pcg_solve, taken by pcg_plan before the first launch. Nothing writes it afterwards but the switch
// to two passes when polishing begins (PcgRun::polish).
struct PcgPlan {
  bool use_dia = false;              // A p from the lattice form, p = z + beta p fused in
  bool two_product = false;          // level 0 of the V-cycle in its two-product form
  bool lattice_two_product = false;  // ... on the index-free lattice path
  bool recompute = false;            // the residual update recomputes A p
  bool fuse_xa = false;              // the residual update writes the V-cycle's first pre-smoothing sweep
  bool grounded = false, projected = false, dirichlet = false, enrich = false;
  bool fused_rr = false;             // the residual update is the fused pass (ResidualPingPong)
  bool sparse_bc = false, virtual_r0 = false, want_graph = false;
  int crit0 = 0, nf = 0, chunk = 1, gv = 0, gm = 1;  // gv, gm: launch grids of the vector kernels, of the mask kernels
  int spmv_g = 0, spmv_gp = 0;       // rows of dot partials the CG product / the last product of the V-cycle write
  int rz_rows = 0, rr_fused_rows = 0;
};

// DirichletCoarse. Dirichlet-masked solves run on the hierarchy of the UNGROUNDED Laplacian, and the mode that makes its
// preconditioned norm optimistic (pcg_plan, crit0) is what makes that preconditioner weak for these solves: along the
// constant of a connected component the grounded operator has the eigenvalue G / n (G = total conductance between the
// column's Dirichlet set and the free nodes of the component), the ungrounded hierarchy answers with 1 / shift (fp64) or not
// at all (fp32: eigenpair dropped, right-hand sides projected), and CG spends its iterations repairing one direction per
// component (300^2 raster, 8 one-to-all columns: 26 / 51 iterations against 10 for a pair solve). Galerkin along the
// candidate v_k of component k on the coarsest level gives the exact answer for that direction:
// v_k'(R A_g P) v_k = 1_k' A_g 1_k = G_k, so the coarsest solve of these solves is
//     x = pinv_without_the_near_kernel_pairs(b) + sum_k v_k (v_k'b) / G_k.
// G_k per column comes from a PROBE: the penalty vector d (d_j = conductance from the free nodes to node j of the set) goes
// down the V-cycle once; every level hands down R (I - A S) d, and v'(R (I - A S) d) = (P v)'d - (A P v)'S d = (P v)'d
// because A annihilates the candidates -- so the component sums of d arrive at the coarsest level intact and the coarsest
// solve, in probe mode, writes coef = 1 / G_k instead of solving (no component labels on the fine level, no index structure
// of the transfer operators needed: the index-free levels serve as they are).
struct DirichletCoarse {  // (takes the hierarchy out of Dirichlet mode when the solve ends, however it ends)
  int* mode = nullptr;
  double** coef = nullptr;
  ~DirichletCoarse() {
    if (mode) *mode = 0;
    if (coef) *coef = nullptr;
  }
};

template <class T, class TP, int K>
inline PcgPlan pcg_plan(const Csr<T>& A, Hierarchy<TP>& H, PcgWork<T, TP>& W, const PcgParams& pp, const Dia<T>* dia) {
  PcgPlan pl;
  Level<TP>& L0 = H.levels[0];
  const int64_t n = A.nrows;
  pl.nf = pp.need_x ? 0 : W.nf;
  pl.use_dia = dia && dia->n == n;
  pl.two_product = H.levels.size() > 1 && L0.two_product() && pp.nu_pre == 1 && pp.nu_post == 1 &&
                   W.tail >= H.levels[1].A.nrows;
  pl.lattice_two_product = pl.two_product && L0.lattice_two_product();
  pl.gv = grid_for(n * K);
  pl.spmv_g = pl.use_dia ? dia_grid<T, TP, K>(*dia) : spmv_grid<T, K>((int)n);
  pl.spmv_gp = pl.lattice_two_product ? dia_grid<TP, TP, K>(L0.Sdia) : spmv_grid<TP, K>((int)n);
  pl.grounded = pp.gptr && pp.gtotal > 0;
  pl.projected = pp.proj && pp.proj->nchunks > 0;  // polygons: PCG in the subspace of polygon-wise constants
  // Dirichlet-masked solves run on the hierarchy of the UNGROUNDED Laplacian: its coarsest pseudo-inverse answers the
  // constant vector with a gain of 1 / (regularisation shift), a right-hand side with a non-zero mean (a unit source)
  // then has an astronomically large r0' M^-1 r0, and the reference's relative rule on that norm is met at once (fuzz
  // finding: ||Ax-b||/||b|| = 7e-5 at rtol 1e-10 on a 155-node tree). The reference builds a hierarchy of the grounded
  // matrix, whose preconditioned norm has no such mode (advanced.jl:282-312). These solves therefore must ALSO meet
  // ||r||_2 <= atol + rtol ||b||_2.
  pl.crit0 = (pl.grounded && pp.criterion == CSGPU_CRIT_KRYLOV) ? CSGPU_CRIT_BOTH : pp.criterion;
  pl.dirichlet = pl.grounded && H.dir_ncomp > 0 && H.coarse_dense && H.coarse_cand.p && A.nnz > 0 && !pp.rhs_in_r;
  pl.gm = pl.grounded ? ceil_div(pp.gtotal, 256) : 1;
  // (not with a projection either -- ADVICE r4: r is replaced after the update wrote xa = omega D^-1 r, so the fused first
  // sweep would start the V-cycle from the unprojected residual)
  pl.fuse_xa = pp.nu_pre >= 1 && H.levels.size() > 1 && !pl.two_product && !pl.grounded && !pl.projected;
  // lattice path: the residual update recomputes A p from the lattice form (one read of p, 5 matrix values per row)
  // instead of the product kernel writing A p and the update reading it back (2 x sizeof(T) per vector element)
  pl.recompute = pl.use_dia && !pl.fuse_xa && knobs().recompute_ap;  // (A/B knob)
  // A p is stored unless the residual update recomputes it; the explicit post-check of a carried solution uses the
  // buffer too. b is read unless the caller wrote the right-hand side straight into r.
  if (!pl.recompute || pp.need_x) W.need_vec(W.Ap);
  if (!pp.rhs_in_r) W.need_vec(W.b);
  // (Dirichlet-masked solves keep the enrichment: with Pm the mask, the preconditioner in effect is Pm M Pm -- r is zero at
  // the grounded entries and z is masked after the correction, so symmetry and the r'z terms hold; polygon handles --
  // `projected` -- do not use it: their hierarchy's matrix carries the strengthened interiors)
  pl.enrich = enrich_applicable<TP>(H.enr, n, pl.use_dia && pl.lattice_two_product, pl.projected);
  pl.rr_fused_rows = acquire_fused_residual<T, TP, K>(H, W, pp, n, pl.enrich, pl.recompute, pl.lattice_two_product, pp.need_x,
                                                      pl.grounded || pl.projected, true);
  pl.fused_rr = pl.rr_fused_rows > 0;
  // pair solves on the lattice two-product path (see PcgParams::pair_src): the first restriction is a scatter of the pairs'
  // <= 18 entries per column -- any precision, any batch width -- and on the fused path r0 is never stored at all
  // (an enriched level on the fused path takes the scatter too -- the pre-pass's share follows on the coarse side, exactly as
  // after a fused update, so a column's first cycle sees the same b_c here and in the streaming loop -- but r0 itself is
  // stored: the pre-pass reads it)
  pl.sparse_bc = pp.pair_src && pp.rhs_in_r && knobs().sparse_init && pl.use_dia && pl.lattice_two_product && !pl.grounded &&
                 !pl.projected && (!pl.enrich || pl.fused_rr);
  pl.virtual_r0 = pl.sparse_bc && pl.fused_rr && pp.bb_host && !pl.enrich;
  if (pl.enrich) enrich_prepare<TP, K>(H.enr, W);
  pl.rz_rows = pl.spmv_gp + (pl.enrich ? kEnrichParts : 0);
  // Launch-bound regime (small rasters: ~75 launches of a few microseconds each per iteration): replay a captured
  // hipGraph of `check_every` iterations instead of issuing the launches one by one. The first chunk always runs
  // directly (it is the one the SpMV timing events sit in); every device-side early-out (skip flag) works unchanged
  // inside the graph because it lives in device memory.
  pl.chunk = std::max(1, pp.check_every);
  pl.want_graph = !W.graph_broken && !(pl.use_dia && (pl.chunk & 1)) &&
                  (pp.use_graph > 0 || (pp.use_graph == 0 && (int64_t)n * K <= ((int64_t)1 << 25)));
  return pl;
}

// One pcg_solve: what it was called with, its plan and buffers, and the state its phases advance.
template <class T, class TP, int K>
struct PcgRun {
  static constexpr bool MIXED = !std::is_same<T, TP>::value;
  const Csr<T>& A;
  Hierarchy<TP>& H;
  PcgWork<T, TP>& W;
  const PcgParams& pp;
  const Dia<T>* dia;
  int ncols_active;
  hipStream_t st;
  int64_t n;  // A.nrows
  PcgPtrs<T, TP> w;
  PcgPlan plan;
  T* x = pp.need_x ? dptr<T>(W.x) : nullptr;
  T* Ap = (!plan.recompute || pp.need_x) ? dptr<T>(W.Ap) : nullptr;
  const T* b = pp.rhs_in_r ? nullptr : dptr<T>(W.b);
  T* xf = dptr<T>(W.xf);
  const int* fnode = dptr<int>(W.fnode);
  VcycleFuse<TP> fuse;
  DirichletCoarse dirichlet_guard;
  ResidualPingPong<T, TP> resid{{w.r, plan.fused_rr ? dptr<T>(W.r2) : nullptr}, w.rp};
  int it = 0, host_done = 0;
  int parity = 0;              // w.pbuf[parity] holds the current search direction (stencil path: ping-pong; CSR path: one buffer)
  int criterion = plan.crit0;  // switches to the true residual for the polishing phase
  int timed = 0, graph_launches = 0;
  // The first product of a batch on the lattice path: beta = 0 for every column (the init call of setup()), so the kernel
  // takes p = z and is not handed the old search direction at all -- a third of the launch's vector traffic, once per batch.
  // That launch (and its iteration's residual update) stays out of the timed set: cg_spmv_ms / cg_spmv_bytes describe
  // launches of ONE size.
  bool first_product = plan.use_dia;
  bool r0_consumed = false;  // virtual_r0: the first fused update has synthesised r0 (or setup() stored it after all)
  PcgBatchResult res;

  int real_updates() const {  // launches enqueued after every column had stopped return at once (device flag)
    int real = 0;
    for (int c = 0; c < ncols_active && c < kMaxK; ++c) real = std::max(real, res.s.iters[c]);
    return real;
  }
  std::pair<const double*, int> collapsed(double* src, int nparts, double* dst) const {
    return collapse_partials<K>(src, nparts, dst, w.collapse_min, st);
  }

  // z = M^-1 r in the subspace of the solve, partials of r'z in w.pa; every launch looks at fuse.skip
  void precondition() {
    apply_preconditioner<T, TP, K>(H, pp, fuse, resid, w.z, plan.enrich, plan.spmv_gp, st);
    fuse.bc_ready = false;
    // (the fused r'z partials are those of the projected z too: r is in the subspace, r'z = r'(Pi z))
    if (plan.projected) poly_project<TP, TP, K>(*pp.proj, w.z, (TP*)nullptr, fuse.skip, st);
    // (the fused r'z partials are unaffected by masking z afterwards: r is zero at the grounded entries)
    if (plan.grounded)
      hipLaunchKernelGGL((mask_grounds_kernel<TP, TP, K>), dim3(plan.gm), dim3(256), 0, st, pp.gptr, pp.gidx, w.z, (TP*)nullptr,
                         fuse.skip);
  }

  // r0, z0 = M^-1 r0 and the scalars of iteration 0 (with the Dirichlet probe in front); leaves host_done
  void setup() {
    const size_t vbytes = (size_t)n * K * sizeof(T);
    T* r = w.r;
    TP* rp = w.rp;
    if (plan.dirichlet) {
      const size_t cbytes = (size_t)kMaxDirComp * kMaxK * sizeof(double);
      if (W.dir_coef.bytes < cbytes) W.dir_coef.alloc(cbytes);
      double* coef = dptr<double>(W.dir_coef);
      TP* mark = w.pbuf[0];  // free until the first iteration; rp (the V-cycle's input, with its tail) takes the penalty vector
      CS_HIP(hipMemsetAsync(mark, 0, (size_t)n * K * sizeof(TP), st));
      CS_HIP(hipMemsetAsync(rp, 0, (size_t)n * K * sizeof(TP), st));
      CS_HIP(hipMemsetAsync(coef, 0, cbytes, st));
      hipLaunchKernelGGL((mark_grounds_kernel<TP, K>), dim3(plan.gm), dim3(256), 0, st, pp.gptr, pp.gidx, mark);
      hipLaunchKernelGGL((dirichlet_penalty_kernel<T, TP, K>), dim3(plan.gm), dim3(256), 0, st, A.rp(), A.ci(), A.va(), pp.gptr,
                         pp.gidx, (const TP*)mark, rp);
      H.dir_coef = coef;
      H.dir_mode = 2;
      dirichlet_guard.mode = &H.dir_mode;
      dirichlet_guard.coef = &H.dir_coef;
      apply_preconditioner<T, TP, K>(H, pp, fuse, resid, w.z, false, plan.spmv_gp, st);  // (the probe: the V-cycle alone)
      H.dir_mode = 1;
      check_launch("pcg dirichlet probe");
    }
    if (pp.need_x) CS_HIP(hipMemsetAsync(x, 0, vbytes, st));
    if (plan.nf > 0) CS_HIP(hipMemsetAsync(xf, 0, (size_t)plan.nf * K * sizeof(T), st));
    W.have_x = pp.need_x;
    CS_REQUIRE(!(pp.rhs_in_r && pp.need_x), CSGPU_INTERNAL, "rhs_in_r needs the focal-node path");
    if (!pp.rhs_in_r) CS_HIP(hipMemcpyAsync(r, b, vbytes, hipMemcpyDeviceToDevice, st));
    CS_HIP(hipMemsetAsync(w.S, 0, sizeof(CgScalars), st));
    auto store_pair_rhs = [&]() {  // r0 = e_dst - e_src
      CS_HIP(hipMemsetAsync(r, 0, vbytes, st));
      hipLaunchKernelGGL((pairs_rhs_kernel<T, K>), dim3(1), dim3(64), 0, st, r, pp.pair_src, pp.pair_dst, pp.pair_cols);
    };
    bool rp_written = pp.rhs_in_r && pp.rp_ready;
    if (pp.rhs_in_r && pp.pair_src && !plan.virtual_r0) {  // ... in both precisions
      store_pair_rhs();
      if (MIXED) {
        CS_HIP(hipMemsetAsync(rp, 0, (size_t)n * K * sizeof(TP), st));
        hipLaunchKernelGGL((pairs_rhs_kernel<TP, K>), dim3(1), dim3(64), 0, st, rp, pp.pair_src, pp.pair_dst, pp.pair_cols);
      }
      rp_written = true;
    }
    if (MIXED && !rp_written)
      hipLaunchKernelGGL((convert_kernel<T, TP>), dim3(plan.gv), dim3(256), 0, st, n * K, (const T*)r, rp);
    // polygons: r0 = Pi b (a unit current into a polygon node is spread evenly over the polygon's cells)
    if (plan.projected) poly_project<T, TP, K>(*pp.proj, r, MIXED ? rp : (TP*)nullptr, (const int*)nullptr, st);
    // z = M^-1 r with the partials of r'z fused into the last smoothing product; r'r separately (criterion 1 / init)
    if (plan.sparse_bc) {
      lattice_restrict_pairs<TP, K>(H.levels[0].Ql, pp.pair_src, pp.pair_dst, pp.pair_cols, dptr<TP>(H.levels[1].b), st);
      fuse.bc_ready = true;
      if (plan.virtual_r0) {
        ++H.virtual_rhs_solves;
        fuse.pair_src = pp.pair_src;
        fuse.pair_dst = pp.pair_dst;
        fuse.pair_cols = pp.pair_cols;
      }
    }
    precondition();
    fuse.pair_src = fuse.pair_dst = nullptr;
    int rr_rows = plan.gv;  // rows of r'r partials currently in pb
    if (pp.rhs_in_r && pp.bb_host) {
      CS_HIP(hipMemcpyAsync(w.pb, pp.bb_host, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st));
      rr_rows = 1;
    } else {
      hipLaunchKernelGGL((dot_kernel<T, K, false>), dim3(plan.gv), dim3(256), 0, st, n, (const T*)r, (const T*)r, w.pb,
                         (const T*)nullptr, (const T*)nullptr, (double*)nullptr);
    }
    auto rz = collapsed(w.pa, plan.rz_rows, w.pac);
    hipLaunchKernelGGL((cg_beta_kernel<K>), dim3(1), dim3(256), 0, st, w.S, rz.first, rz.second, (const double*)w.pb, rr_rows,
                       plan.crit0, pp.rtol, w.atol, 1, ncols_active);
    // the first iteration runs p = z + beta p with beta = 0 (set by the init call above): the lattice product takes p = z
    // whatever the old p holds (stencil.h), the CSR path's update kernel multiplies the old p by zero and needs it finite
    if (!plan.use_dia) CS_HIP(hipMemsetAsync(w.pbuf[0], 0, (size_t)n * K * sizeof(TP), st));
    check_launch("pcg init");
    CS_HIP(hipMemcpyAsync(&host_done, &w.S->all_done, sizeof(int), hipMemcpyDeviceToHost, st));
    CS_HIP(hipStreamSynchronize(st));
    if (plan.virtual_r0 && host_done) {
      // nothing will iterate (every column's right-hand side is zero): the post-check reads r, so store r0 after all
      store_pair_rhs();
      r0_consumed = true;
    }
    fuse.xa_ready = plan.fuse_xa;
    fuse.skip = &w.S->all_done;
  }

  // one PCG iteration as a sequence of launches on the stream (no host interaction: this is what gets captured)
  //   p = z + beta p ; Ap = A p, p'Ap ; alpha ; r -= alpha Ap, x += alpha p ; z = M^-1 r, r'z ; beta, stopping rule
  void iteration(bool time_it) {
    Level<TP>& L0 = H.levels[0];
    const int gv = plan.gv;
    const CgScalars* S = w.S;
    const int* done = &w.S->all_done;
    const bool short_first = first_product;
    first_product = false;
    const TP* pin = short_first ? (const TP*)nullptr : (const TP*)w.pbuf[parity];
    TP* pcur = plan.use_dia ? w.pbuf[parity ^ 1] : w.pbuf[parity];
    time_it = time_it && timed < knobs().timed_launches && !short_first;  // (timed_launches: per solve)
    const int slot = timed;
    if (plan.use_dia) {
      // fused: p = z + beta p (written to the other buffer), Ap = A p, partials of p'Ap
      if (time_it) W.ev.begin(slot, st);
      dia_cg_product<T, TP, K>(*dia, S, (const TP*)w.z, pin, pcur, plan.recompute ? (T*)nullptr : Ap, w.pc, st);
      parity ^= 1;
    } else {
      hipLaunchKernelGGL((cg_update_p_kernel<T, TP, K>), dim3(gv), dim3(256), 0, st, n, S, pin, pcur, (const TP*)w.z);
      SpmvArgs<T, TP> a = spmv_args<T, TP>(A, (const TP*)pcur, Ap);
      a.order = L0.orderA.p ? dptr<int>(L0.orderA) : nullptr;
      a.skip = done;
      a.dotw = nullptr;  // dot with x itself: p'Ap
      a.partials = w.pc;
      if (time_it) W.ev.begin(slot, st);
      spmv_launch_cg<T, K, TP>(a, st);
    }
    if (time_it) {
      W.ev.end(slot, st);
      ++timed;
    }
    auto pap = collapsed(w.pc, plan.spmv_g, w.pcc);
    hipLaunchKernelGGL((cg_alpha_kernel<K>), dim3(1), dim3(256), 0, st, w.S, pap.first, pap.second);
    // r -= alpha Ap (+ x += alpha p when the whole solution is wanted), fused with the TP copy of r, the level-0 first
    // pre-smoothing sweep xa = omega D^-1 r and (when the true residual is monitored) the partials of r'r
    TP* rpo = MIXED ? w.rp : (TP*)nullptr;
    if (time_it && plan.use_dia) W.ev2.begin(slot, st);
    if (plan.fused_rr) {
      // (the partials of r'r come for free on the recomputing paths; the focal path's post-check reads the last ones instead
      // of making another pass over r)
      if constexpr (!MIXED) {
        RupdRestrictOpts<T> o;
        if (plan.virtual_r0 && !r0_consumed) o.isrc = pp.pair_src;  // (r holds nothing yet: the kernel synthesises r0)
        o.idst = pp.need_x ? nullptr : pp.pair_dst;
        o.icols = pp.pair_cols;
        o.xsol = x;
        lattice_rupd_restrict<T, K>(*dia, L0.Ql, S, (const T*)pcur, (const T*)resid.cur(), resid.next(), dptr<T>(H.levels[1].b),
                                    w.pb, st, o);
        r0_consumed = true;
        resid.flip();
      }
    } else if (plan.recompute) {
      dia_residual_update<T, TP, K>(*dia, S, (const TP*)pcur, resid.cur(), rpo, x, w.pb, st);
    } else {
      TP* xao = plan.fuse_xa ? dptr<TP>(L0.xa) : (TP*)nullptr;
      const TP* dinv0 = dptr<TP>(L0.dinv);
      const TP omega0 = (TP)L0.omega;
      const bool rr = criterion != CSGPU_CRIT_KRYLOV;
#define CS_UPD_R(RR, XUP)                                                                                   \
    hipLaunchKernelGGL((cg_update_r_kernel<T, TP, K, RR, XUP>), dim3(gv), dim3(256), 0, st, n, S, resid.cur(), (const T*)Ap, rpo, \
                       xao, dinv0, omega0, w.pb, x, (const TP*)pcur)
      if (rr && pp.need_x) CS_UPD_R(true, true);
      else if (rr) CS_UPD_R(true, false);
      else if (pp.need_x) CS_UPD_R(false, true);
      else CS_UPD_R(false, false);
#undef CS_UPD_R
    }
    if (time_it && plan.use_dia) W.ev2.end(slot, st);
    T* r = resid.cur();
    const bool rr_after_mask = (plan.grounded || plan.projected) && criterion != CSGPU_CRIT_KRYLOV;
    auto masked_rr = [&]() {
      hipLaunchKernelGGL((dot_kernel<T, K, false>), dim3(gv), dim3(256), 0, st, n, (const T*)r, (const T*)r, w.pb,
                         (const T*)nullptr, (const T*)nullptr, (double*)nullptr);
    };
    if (plan.projected) {  // r <- Pi r: the residual of the projected system (both precisions)
      poly_project<T, TP, K>(*pp.proj, r, rpo, done, st);
      if (rr_after_mask) {
        // ||r||^2 in NODE space = the merged system's (the reference's figure): cell-space partials + one correction row
        masked_rr();
        hipLaunchKernelGGL((poly_norm_corr_kernel<K>), dim3(1), dim3(256), 0, st, *pp.proj, w.pb + (size_t)gv * K, done);
      }
    }
    if (plan.grounded) {  // the update put (A p) at the grounded rows into r: back to zero, in both precisions
      hipLaunchKernelGGL((mask_grounds_kernel<T, TP, K>), dim3(plan.gm), dim3(256), 0, st, pp.gptr, pp.gidx, r, rpo, done);
      // the partials of r'r the update wrote include alpha (A p) at the Dirichlet rows, which are not equations of the
      // reduced system: when the true residual is monitored, take the norm of the masked r instead
      if (rr_after_mask) masked_rr();
    }
    if (plan.nf > 0)
      hipLaunchKernelGGL((cg_focal_x_kernel<T, TP, K>), dim3(ceil_div(plan.nf * K, 256)), dim3(256), 0, st, S, fnode, plan.nf,
                         (const TP*)pcur, xf);
    fuse.bc_ready = plan.fused_rr;
    precondition();
    auto rz = collapsed(w.pa, plan.rz_rows, w.pac);
    // r'r partials (true-residual criterion): one row per workgroup of whichever kernel updated r
    const double* prr = w.pb;
    int nrr = (plan.projected && rr_after_mask) ? gv + 1 : gv;  // (+ the node-space correction row of a polygon handle)
    if (plan.recompute && criterion != CSGPU_CRIT_KRYLOV && !rr_after_mask) {
      auto rr = collapsed(w.pb, plan.fused_rr ? plan.rr_fused_rows : plan.spmv_g, w.pcc);
      prr = rr.first;
      nrr = rr.second;
    }
    hipLaunchKernelGGL((cg_beta_kernel<K>), dim3(1), dim3(256), 0, st, w.S, rz.first, rz.second, prr, nrr, criterion, pp.rtol,
                       w.atol, 0, ncols_active);
  }

  // The key of the chunk the loop is about to run: every non-pointer value that reaches a kernel argument of iteration()
  // comes from the plan, PcgParams or the three pieces of run state read here.
  PcgGraphKey graph_key() const {
    PcgGraphKey k;
    k.K = K;
    k.ncols_active = ncols_active;
    k.criterion = criterion;
    k.nu_pre = pp.nu_pre;
    k.nu_post = pp.nu_post;
    k.nu_coarse = pp.nu_coarse;
    k.iters = plan.chunk;
    k.rtol = pp.rtol;
    k.atol = w.atol;
    // (a raster handle without a CSR form has no values there: its lattice rows are what the chunk's kernels read)
    k.matrix = A.val.p ? (const void*)A.val.p : (plan.use_dia ? (const void*)dia->rows.p : nullptr);
    k.need_x = pp.need_x ? 1 : 0;
    k.nf = plan.nf;
    k.parity = parity | (resid.sel << 1);
    k.fused = plan.fused_rr ? 1 : 0;
    k.gptr = plan.grounded ? (const void*)pp.gptr : nullptr;
    k.gidx = plan.grounded ? (const void*)pp.gidx : nullptr;
    k.gtotal = plan.grounded ? pp.gtotal : 0;
    k.proj = plan.projected ? (const void*)pp.proj->cells : nullptr;
    return k;
  }

  // the captured chunk for the current key (captured now if need be); null = run the launches directly
  hipGraphExec_t chunk_graph() {
    const PcgGraphKey gkey = graph_key();
    for (auto& g : W.graphs)
      if (g.first == gkey) return g.second;
    check_launch("pcg before capture");
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError();
      W.graph_broken = true;
      return nullptr;
    }
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    bool ok = true;
    const int parity0 = parity, rsel0 = resid.snapshot();
    try {
      for (int c = 0; c < plan.chunk; ++c) iteration(false);
    } catch (...) {
      ok = false;
    }
    parity = parity0;  // capturing executed nothing: the launch advances the parity
    resid.restore(rsel0);
    if (hipStreamEndCapture(st, &g) != hipSuccess || !g) ok = false;
    if (ok && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) ok = false;
    if (g) hipGraphDestroy(g);
    if (!ok || !ge) {
      (void)hipGetLastError();
      W.graph_broken = true;
      return nullptr;
    }
    if (W.graphs.size() >= 8) W.drop_graphs();
    W.graphs.emplace_back(gkey, ge);
    return ge;
  }

  // chunks of `check_every` iterations, one synchronisation each, until every column stopped or itmax
  void run_loop() {
    while (!host_done && it < pp.itmax) {
      const int todo = (int)std::min<int64_t>(plan.chunk, (int64_t)pp.itmax - it);
      hipGraphExec_t ge = (plan.want_graph && it > 0 && todo == plan.chunk) ? chunk_graph() : nullptr;
      if (ge) {
        CS_HIP(hipGraphLaunch(ge, st));
        ++graph_launches;  // (want_graph asks for an even chunk: parity and the fused update's residual end where they started)
      } else {
        for (int c = 0; c < todo; ++c) iteration(true);
      }
      it += todo;
      check_launch("pcg iteration");
      CS_HIP(hipMemcpyAsync(&host_done, &w.S->all_done, sizeof(int), hipMemcpyDeviceToHost, st));
      CS_HIP(hipStreamSynchronize(st));
    }
  }

  // the reference's post-check (core.jl:640): ||A x - b|| / ||b||, explicitly when x is carried, otherwise from the
  // fp64 recurrence residual; the scalars land in res.s
  void post_check() {
    const int gv = plan.gv;
    const double* num = w.pa;  // relres = sqrt(sum of `nnum` rows of num / sum of `nden` rows of den), den null: ||b|| of start-up
    const double* den = nullptr;
    int nnum = gv, nden = 0;
    DBuf nrm;                      // block-diagonal systems: per-component norms
    double* worst = nullptr;
    if (pp.need_x) {
      if (pp.lattice_check && plan.use_dia && !plan.grounded && !plan.projected) {
        dia_apply<T, K>(*dia, (const T*)x, Ap, b, (const int*)nullptr, st);  // Ap = b - A x, no CSR array read
        res.lattice_check = 1;
      } else {
        SpmvArgs<T> a = spmv_args(A, (const T*)x, Ap);
        a.order = H.levels[0].orderA.p ? dptr<int>(H.levels[0].orderA) : nullptr;
        a.b = b;
        spmv_launch<T, K>(a, EPI_RESID, false, st);
      }
      if (plan.grounded)  // rows of the grounded nodes are not equations of the reduced system
        hipLaunchKernelGGL((mask_grounds_kernel<T, T, K>), dim3(plan.gm), dim3(256), 0, st, pp.gptr, pp.gidx, Ap, (T*)nullptr,
                           (const int*)nullptr);
      hipLaunchKernelGGL((dot_kernel<T, K, true>), dim3(gv), dim3(256), 0, st, n, (const T*)Ap, (const T*)Ap, w.pa, b, b, w.pb);
      den = w.pb;
      nden = gv;
      if (K == 1 && pp.comp_label && pp.ncomp > 1) {
        nrm = dalloc<double>((size_t)2 * pp.ncomp + 1);
        CS_HIP(hipMemsetAsync(nrm.p, 0, nrm.bytes, st));
        double* rr = dptr<double>(nrm);
        double* bb = rr + pp.ncomp;
        hipLaunchKernelGGL((comp_norms_kernel<T>), dim3(grid_for(n)), dim3(256), 0, st, (int)n, pp.comp_label, (const T*)Ap, b,
                           rr, bb);
        hipLaunchKernelGGL(comp_relres_kernel, dim3(1), dim3(256), 0, st, pp.ncomp, (const double*)rr, (const double*)bb,
                           bb + pp.ncomp);
        worst = bb + pp.ncomp;
      }
    } else if (plan.recompute && it > 0 && !plan.grounded && !plan.projected) {
      // fp64 recurrence residual against ||b|| recorded at start-up:
      // ||r||^2 partials of the last residual update that ran (surplus launches exit before writing)
      auto rr = collapsed(w.pb, plan.fused_rr ? plan.rr_fused_rows : plan.spmv_g, w.pcc);
      num = rr.first;
      nnum = rr.second;
    } else {
      const T* r = resid.cur();
      hipLaunchKernelGGL((dot_kernel<T, K, false>), dim3(gv), dim3(256), 0, st, n, r, r, w.pa, (const T*)nullptr,
                         (const T*)nullptr, (double*)nullptr);
      if (plan.projected) {
        // polygon handle: the figure of the MERGED system, ||b_m - A_m y|| / ||b_m|| (src/core.jl:640-641) -- r is
        // polygon-wise constant, its chunk sums are taken again (the last projection was z's), the correction row follows
        hipLaunchKernelGGL((poly_chunk_sum_kernel<T, K>), dim3(pp.proj->nchunks), dim3(256), 0, st, *pp.proj, r,
                           (const int*)nullptr);
        hipLaunchKernelGGL((poly_norm_corr_kernel<K>), dim3(1), dim3(256), 0, st, *pp.proj, w.pa + (size_t)gv * K,
                           (const int*)nullptr);
        nnum = gv + 1;
      }
    }
    hipLaunchKernelGGL((relres_kernel<K>), dim3(1), dim3(256), 0, st, w.S, num, nnum, den, nden);
    if (worst)  // overwrite column 0's figure with the worst component's
      CS_HIP(hipMemcpyAsync(&w.S->relres[0], worst, sizeof(double), hipMemcpyDeviceToDevice, st));
    CS_HIP(hipMemcpyAsync(&res.s, w.S, sizeof(CgScalars), hipMemcpyDeviceToHost, st));
    CS_HIP(hipStreamSynchronize(st));
  }

  // Polishing. Krylov.jl's rule stops on the PRECONDITIONED residual norm; on nearly singular grounded systems (one weak
  // ground in a large component) that norm can be 100x more optimistic than ||Ax-b||/||b||, and the reference's own 1e-4
  // check (core.jl:640) is then decided by how the preconditioner happens to weight the near-null space. A column that
  // stopped "converged" but would fail that check is re-opened and iterated on the true residual (CG restarts from x with
  // p = z: state is consistent, see cg_reopen_kernel) until ||r||/||b|| <= 2.5e-5. Columns that pass -- every case in which
  // the reference's rule is adequate -- are untouched, bit for bit.
  void polish() {
    bool reopen = false;
    for (int c = 0; c < ncols_active && c < kMaxK; ++c)
      if (res.s.done[c] == 1 && !(res.s.relres[c] < 1e-4)) reopen = true;
    if (!reopen || it >= pp.itmax) return;
    if (plan.fused_rr) {  // the polishing phase runs the two-pass update in place, from the buffer that holds the residual
      resid.rewind_to_update(real_updates());
      plan.fused_rr = false;
    }
    criterion = CSGPU_CRIT_TRUE_RESIDUAL;
    hipLaunchKernelGGL((cg_reopen_kernel<K>), dim3(1), dim3(64), 0, st, w.S, 1e-4, 2.5e-5, ncols_active);
    host_done = 0;
    run_loop();
    post_check();
    res.polished = 1;
  }

  // launch times and algorithmic byte counts of the result
  void summary() {
    // launches enqueued after every column had converged return immediately: leave them out of the average
    // (on the lattice path the timed launches are those of iterations 1, 2, ...: the first one is shorter, see first_product)
    const int counted = std::min(timed, std::max(real_updates() - (plan.use_dia ? 1 : 0), 0));
    res.spmv_ms = W.ev.sum_ms(counted);
    res.spmv_calls = counted;
    if (plan.use_dia) {
      // algorithmic bytes of one residual-update launch: the lattice rows, p, r read and written (+ its copy in the
      // preconditioner's precision); fused with the restriction: + the nine values of Q per row and the coarse right-hand side
      res.resid_ms = W.ev2.sum_ms(counted);
      res.resid_calls = counted;
      res.resid_bytes = n * 5 * (int64_t)sizeof(T) + n * K * ((int64_t)sizeof(TP) + 2 * (int64_t)sizeof(T) + (MIXED ? (int64_t)sizeof(TP) : 0));
      if (res.resid_fused && H.levels.size() > 1)
        res.resid_bytes += n * 9 * (int64_t)sizeof(T) + (int64_t)H.levels[1].A.nrows * K * (int64_t)sizeof(T);
      // (the fused pass that carries the solution: x read and written; the two-pass figure has never counted x)
      if (res.resid_fused && pp.need_x) res.resid_bytes += 2 * n * K * (int64_t)sizeof(T);
      if (!plan.recompute) res.resid_bytes = 0;  // (the generic update kernel: not this formula)
    }
    res.graph_launches = graph_launches;
    if (plan.use_dia)
      res.spmv_bytes = n * 5 * (int64_t)sizeof(T) + n * K * (3 * (int64_t)sizeof(TP) + (plan.recompute ? 0 : (int64_t)sizeof(T)));
    else
      res.spmv_bytes = A.nnz * (int64_t)(sizeof(T) + 4) + (n + 1) * 4 + n * K * (int64_t)(sizeof(TP) + sizeof(T));
  }
};

// Solve A X = B for the K interleaved columns held in W.b. With pp.need_x the solution is left in W.x; otherwise only
// the entries at W.fnode are accumulated (W.xf) and W.x is not touched (not even allocated).
// A is the matrix CG sees (precision T); H is the hierarchy (precision TP) whose level 0 has A's sparsity pattern.
// `dia`: optional symmetric-diagonal (lattice) form of A (stencil.h); when given, the product A p is evaluated from it
// with the search-direction update p = z + beta p fused in, and A's CSR form is only used by the explicit post-check.
template <class T, class TP, int K>
inline PcgBatchResult pcg_solve(const Csr<T>& A, Hierarchy<TP>& H, PcgWork<T, TP>& W, const PcgParams& pp,
                                int ncols_active, hipStream_t st, const Dia<T>* dia = nullptr) {
  const int64_t n = A.nrows;
  ensure_level_work(H, K);
  if (pp.need_x) W.need_vec(W.x);
  const PcgPtrs<T, TP> w = pcg_ptrs<T, TP>(W, pp, dia && dia->n == n);
  LaunchTimer span;
  span.begin(0, st);
  PcgRun<T, TP, K> q{A, H, W, pp, dia, ncols_active, st, n, w, pcg_plan<T, TP, K>(A, H, W, pp, dia)};
  q.fuse.b_has_tail = q.plan.two_product;
  q.fuse.partials = w.pa;
  q.res.explicit_relres = pp.need_x;
  q.res.resid_fused = q.plan.fused_rr ? 1 : 0;  // (before any polishing)
  q.setup();
  q.run_loop();
  q.post_check();
  q.polish();
  span.end(0, st);
  CS_HIP(hipStreamSynchronize(st));
  check_launch("pcg finish");
  q.res.device_ms = span.sum_ms(1);
  q.summary();
  return q.res;
}

// ---- streaming pair solves ("continuous batching") ---------------------------------------------------------------------
// pcg_solve streams all K columns of a batch until its SLOWEST column has converged (10.76 iterations on average against
// 11 on the bench raster, but 13.9 against 16 on a raster with 15 % NODATA and 82 against 91 on a log-normal sigma = 3
// one: up to 13 % of all traffic moved for columns that were done). The columns of a batch are
// independent CG recurrences that merely share the passes over the matrix, so a column can take the NEXT pair of the
// call's list the moment its own pair is done:
//   iteration t, slot c restarts:   the CG product and alpha of the slot are idle (alpha = 0, beta = 0),
//                                   the residual update writes r_c = 0 and stream_restart_kernel the two +-1 entries,
//                                   the V-cycle of the same iteration delivers z_c = M^-1 b  (a batch's separate initial
//                                   V-cycle), cg_stream_beta_kernel initialises the slot's scalars;
//   iteration t + 1:                p_c = z_c (beta = 0) -- the slot's first CG step.
// A pair therefore costs (its own iterations + 1) slots instead of max-over-the-batch iterations + an initial V-cycle.
// Every per-column quantity (dot products reduced over the workgroups in a fixed order, the V-cycle, the focal-node
// accumulation) is independent of what the neighbouring columns hold, so a pair's iterates are bit-identical to those of
// the batch path (tests/helpers.py::check_stream_pairs); only a column that needs polishing continues without the restart
// cg_reopen_kernel makes.
// Applies to resistance-only pair solves on the lattice path (x at the focal nodes only, A p recomputed by the residual
// update, two-product level 0); the host polls the slots after every iteration, so it is used in the bandwidth-bound
// regime (an iteration takes milliseconds) and when the call has more pairs than columns. CSGPU_NO_STREAM=1: A/B knob.
struct PcgStreamResult {
  bool applicable = false;
  std::vector<int> iters, status;       // per pair: iterations, CgScalars::done value (1 ok, 2 breakdown, 4 itmax)
  std::vector<double> relres;           // per pair: ||r|| / ||b|| of the fp64 recurrence residual at the end
  double device_ms = 0, spmv_ms = 0;
  int64_t spmv_calls = 0, spmv_bytes = 0;
  int64_t slots = 0;                    // iterations of the K-wide stream
  int64_t polished = 0;
};

template <class T, class TP, int K>
inline PcgStreamResult pcg_stream_pairs(Hierarchy<TP>& H, PcgWork<T, TP>& W, const PcgParams& pp, const Dia<T>& dia,
                                        const int64_t* src, const int64_t* dst, int64_t npairs, const int64_t* gather,
                                        int64_t ngather, T* resist_out, T* gathered_out, hipStream_t st) {
  constexpr bool MIXED = !std::is_same<T, TP>::value;
  PcgStreamResult res;
  Level<TP>& L0 = H.levels[0];
  const int64_t n = dia.n;
  const bool two_product = H.levels.size() > 1 && L0.two_product() && L0.lattice_two_product() && pp.nu_pre == 1 &&
                           pp.nu_post == 1 && W.tail >= H.levels[1].A.nrows;
  const bool off = knobs().stream < 0 || !knobs().recompute_ap;
  if (off || !two_product || W.n != n || W.K != K) return res;
  // focal nodes: the gathered nodes first, then every distinct node of the pair list
  std::vector<int> focal;
  std::vector<int64_t> keys;
  keys.reserve((size_t)2 * npairs);
  for (int64_t p = 0; p < npairs; ++p) {
    keys.push_back(src[p]);
    keys.push_back(dst[p]);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  if ((int64_t)keys.size() + ngather > 8192) return res;  // (a pair list over that many distinct nodes: batch path)
  for (int64_t g = 0; g < ngather; ++g) focal.push_back((int)gather[g]);
  for (int64_t k : keys) focal.push_back((int)k);
  auto focal_of = [&](int64_t node) {
    return (int)ngather + (int)(std::lower_bound(keys.begin(), keys.end(), node) - keys.begin());
  };
  res.applicable = true;
  res.iters.assign((size_t)npairs, 0);
  res.status.assign((size_t)npairs, 1);
  res.relres.assign((size_t)npairs, 0.0);
  ensure_level_work(H, K);
  const PcgPtrs<T, TP> w = pcg_ptrs<T, TP>(W, pp, true);
  W.set_focal(focal, st);
  W.have_x = false;
  const int nf = W.nf;
  TP* const* pbuf = w.pbuf;
  TP* z = w.z;
  CgScalars* S = w.S;
  if (W.part_cb.bytes < (size_t)kCollapsedParts * kMaxK * sizeof(double)) W.part_cb.alloc((size_t)kCollapsedParts * kMaxK * sizeof(double));
  double* pbc = dptr<double>(W.part_cb);
  T* xf = dptr<T>(W.xf);
  const int* fnode = dptr<int>(W.fnode);
  const int spmv_g = dia_grid<T, TP, K>(dia);
  const int spmv_gp = dia_grid<TP, TP, K>(L0.Sdia);
  auto collapsed = [&](double* from, int nparts, double* to) { return collapse_partials<K>(from, nparts, to, w.collapse_min, st); };
  LaunchTimer span;
  span.begin(0, st);
  // every vector finite before the first pass (a slot's first iteration multiplies stale values by zero)
  CS_HIP(hipMemsetAsync(w.r, 0, (size_t)n * K * sizeof(T), st));
  if (MIXED) CS_HIP(hipMemsetAsync(w.rp, 0, (size_t)n * K * sizeof(TP), st));
  CS_HIP(hipMemsetAsync(z, 0, (size_t)n * K * sizeof(TP), st));
  CS_HIP(hipMemsetAsync(pbuf[0], 0, (size_t)n * K * sizeof(TP), st));
  CS_HIP(hipMemsetAsync(pbuf[1], 0, (size_t)n * K * sizeof(TP), st));
  if (nf > 0) CS_HIP(hipMemsetAsync(xf, 0, (size_t)nf * K * sizeof(T), st));
  // slots
  CgScalars hs;
  memset(&hs, 0, sizeof(hs));
  std::vector<int64_t> slot_pair(K, -1);
  int64_t next = 0;
  int active = 0;
  auto take_next = [&](int c) {
    // pairs whose two nodes coincide have a zero right-hand side: R = 0 without a solve (the reference skips them,
    // core.jl:210)
    while (next < npairs && src[next] == dst[next]) {
      if (resist_out) resist_out[next] = T(0);
      if (gathered_out)
        for (int64_t g = 0; g < ngather; ++g) gathered_out[(size_t)next * ngather + g] = T(0);
      ++next;
    }
    if (next < npairs) {
      slot_pair[c] = next;
      hs.ctl.restart[c] = 1;
      hs.ctl.src[c] = (int)src[next];
      hs.ctl.dst[c] = (int)dst[next];
      hs.ctl.active[c] = 1;
      ++next;
      ++active;
    } else {
      slot_pair[c] = -1;
      hs.ctl.restart[c] = 0;
      hs.ctl.active[c] = 0;
    }
  };
  for (int c = 0; c < K; ++c) {
    hs.done[c] = 1;  // (alpha = 0 until the slot's scalars are initialised)
    take_next(c);
  }
  for (int c = K; c < kMaxK; ++c) hs.done[c] = 1;
  CS_HIP(hipMemcpyAsync(S, &hs, sizeof(CgScalars), hipMemcpyHostToDevice, st));
  VcycleFuse<TP> fuse;
  fuse.b_has_tail = true;
  fuse.partials = w.pa;
  // (the stream only runs on the lattice two-product path of a handle without polygons -- checked above and by the caller)
  const bool enrich = enrich_applicable<TP>(H.enr, n, two_product, pp.proj != nullptr);
  if (enrich) enrich_prepare<TP, K>(H.enr, W);
  const int rz_rows = spmv_gp + (enrich ? kEnrichParts : 0);
  // the stream's constants in the batch solve's predicate: A p recomputed, two-product lattice level, no x, no masks
  // (a second residual buffer an earlier batch solve left stays where it is)
  const int rr_fused_rows = acquire_fused_residual<T, TP, K>(H, W, pp, n, enrich, true, true, false, false, false);
  const bool fused_rr = rr_fused_rows > 0;
  const int rr_rows = fused_rr ? rr_fused_rows : spmv_g;
  ResidualPingPong<T, TP> rr{{w.r, fused_rr ? dptr<T>(W.r2) : nullptr}, w.rp};
  fuse.bc_ready = fused_rr;  // (every cycle of the loop follows a fused update)
  const RupdRestrictOpts<T> restarts{S->ctl.restart, S->ctl.src, S->ctl.dst};
  const int max_timed = knobs().timed_launches;
  int timed = 0;
  int parity = 0;
  std::vector<T> hxf;
  while (active > 0) {
    const TP* pin = pbuf[parity];
    TP* pcur = pbuf[parity ^ 1];
    const bool time_it = timed < max_timed;
    if (time_it) W.ev.begin(timed, st);
    dia_cg_product<T, TP, K>(dia, (const CgScalars*)S, (const TP*)z, pin, pcur, (T*)nullptr, w.pc, st);
    if (time_it) W.ev.end(timed++, st);
    parity ^= 1;
    auto pap = collapsed(w.pc, spmv_g, w.pcc);
    hipLaunchKernelGGL((cg_alpha_kernel<K>), dim3(1), dim3(256), 0, st, S, pap.first, pap.second);
    if (fused_rr) {
      if constexpr (!MIXED) {
        lattice_rupd_restrict<T, K>(dia, L0.Ql, (const CgScalars*)S, (const T*)pcur, (const T*)rr.cur(), rr.next(),
                                    dptr<T>(H.levels[1].b), w.pb, st, restarts);
        rr.flip();
      }
    } else {
      dia_residual_update<T, TP, K>(dia, (const CgScalars*)S, (const TP*)pcur, rr.cur(), MIXED ? w.rp : (TP*)nullptr, (T*)nullptr,
                                    w.pb, st, (const int*)S->ctl.restart);
    }
    if (nf > 0)
      hipLaunchKernelGGL((cg_focal_x_kernel<T, TP, K>), dim3(ceil_div(nf * K, 256)), dim3(256), 0, st, (const CgScalars*)S,
                         fnode, nf, (const TP*)pcur, xf);
    hipLaunchKernelGGL((stream_restart_kernel<T, TP, K>), dim3(1), dim3(256), 0, st, (const CgScalars*)S, rr.cur(),
                       MIXED ? w.rp : (TP*)nullptr, nf, xf);
    apply_preconditioner<T, TP, K>(H, pp, fuse, rr, z, enrich, spmv_gp, st);
    auto rz = collapsed(w.pa, rz_rows, w.pac);
    auto rrp = collapsed(w.pb, rr_rows, pbc);
    hipLaunchKernelGGL((cg_stream_beta_kernel<K>), dim3(1), dim3(256), 0, st, S, rz.first, rz.second, rrp.first, rrp.second,
                       pp.criterion, pp.rtol, w.atol, pp.itmax);
    check_launch("pcg stream iteration");
    ++res.slots;
    CS_HIP(hipMemcpyAsync(&hs, S, sizeof(CgScalars), hipMemcpyDeviceToHost, st));
    CS_HIP(hipStreamSynchronize(st));
    bool any = false;
    for (int c = 0; c < K; ++c)
      if (slot_pair[c] >= 0 && hs.done[c] != 0 && !hs.ctl.restart[c]) any = true;
    if (!any) continue;
    hxf.resize((size_t)nf * K);
    CS_HIP(hipMemcpyAsync(hxf.data(), xf, hxf.size() * sizeof(T), hipMemcpyDeviceToHost, st));
    CS_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < K; ++c) {
      const int64_t p = slot_pair[c];
      if (p < 0 || hs.done[c] == 0 || hs.ctl.restart[c]) continue;
      const T vs = hxf[(size_t)focal_of(src[p]) * K + c];
      if (resist_out) resist_out[p] = hxf[(size_t)focal_of(dst[p]) * K + c] - vs;
      if (gathered_out)
        for (int64_t g = 0; g < ngather; ++g) gathered_out[(size_t)p * ngather + g] = hxf[(size_t)g * K + c] - vs;
      res.iters[(size_t)p] = hs.iters[c];
      res.status[(size_t)p] = hs.done[c];
      res.relres[(size_t)p] = hs.relres[c];
      res.polished += hs.polish[c] ? 1 : 0;
      --active;
      take_next(c);
    }
    hs.all_done = 0;
    // the control block and the flags the next iteration's kernels look at (done stays set for a restarting slot: its
    // alpha must be zero until cg_stream_beta_kernel has initialised it)
    CS_HIP(hipMemcpyAsync(&S->ctl, &hs.ctl, sizeof(hs.ctl), hipMemcpyHostToDevice, st));
    CS_HIP(hipMemcpyAsync(&S->all_done, &hs.all_done, sizeof(int), hipMemcpyHostToDevice, st));
  }
  span.end(0, st);
  CS_HIP(hipStreamSynchronize(st));
  check_launch("pcg stream finish");
  res.device_ms = span.sum_ms(1);
  res.spmv_ms = W.ev.sum_ms(timed);
  res.spmv_calls = timed;
  res.spmv_bytes = n * 5 * (int64_t)sizeof(T) + n * K * 3 * (int64_t)sizeof(TP);
  return res;
}

}  // namespace csgpu
