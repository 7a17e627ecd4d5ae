// lattice_currents.h -- node currents of a batch of pair solves straight from the lattice form (no CSR matrix).
//
// The same post-processing as currents.h (src/out.jl:178-290: branch currents b_e = |g_e| (v_row - v_col) per upper-triangular
// entry, entries below 1e-8 of the largest one dropped per orientation, node current = max(inflow, outflow)), evaluated on
// the marching skeleton of dia_cg_kernel (stencil.h): a workgroup owns TI raster rows of `seg` raster columns, stages x and
// the five lattice values of a column through the 4-slot LDS ring and keeps the 3 x 3 window of x in registers. Every number
// equals what branch_max_kernel / node_current_kernel / current_accumulate_kernel return on the CSR form dia_to_csr builds
// from the same lattice form: a ZERO lattice value is an absent edge there (the last row's +1, the diagonals of a
// four-neighbour raster, everything around a NODATA cell, the halo) and is skipped here, not multiplied; a row's neighbours
// are visited in ascending column order; all sums are taken in double in that order.
//
// Algorithmic bytes (T = value type, K = batch width):
//   pass 1 (dia_branch_max_kernel):    n*5*T + n*K*T                       read
//   pass 2 (dia_node_current_kernel):  n*5*T + n*K*T                       read
//                                      + n*K*T written                     (currents wanted, epilogue a)
//                                      + n*T read and written per map      (cumulative / maximum map only, epilogue b)
// against nnz*(T+4) + (n+1)*4 + n*K*T per CSR pass (nnz ~ 9 n) plus the separate accumulation pass over n*K*T.
#pragma once
#include "currents.h"
#include "stencil.h"

namespace csgpu {

template <class T>
struct DiaCurrArgs {
  int64_t n;
  int R, C;
  int nstrips, nseg, seg;  // tiles, as in DiaArgs
  const T* rows;           // lattice form [n][5]
  const T* x;              // voltages, interleaved [n][K]
  double* part;            // pass 1: [gridDim.x][K][2] partial maxima (pos, neg orientation)
  const double* maxcur;    // pass 2: [K][2]
  T* curr;                 // pass 2, epilogue (a): node currents, interleaved [n][K]; null = epilogue (b)
  T* cum;                  // epilogue (b): cum[row] += sum_c weight[c] * curr[row, c] (may be null)
  T* mx;                   // epilogue (b): mx[row] = max(mx[row], max_{c: weight[c] > 0} curr[row, c]) (may be null)
  const int* weight;       // epilogue (b): [K]
  int ncols;               // epilogue (b): columns that hold a pair
};

// Drop test of out.jl:250-290, `fabs(b / m) < 1e-8`, without the division where its outcome is certain. With
// t = fl(1e-8 * |m|) (a normal number): |b| < t (1 - 2^-40) makes the rounded quotient |b| / |m| smaller than the double 1e-8,
// |b| > t (1 + 2^-40) makes it larger (the two roundings involved move a value by 2^-52 at most); in between -- and for
// every m whose t is zero, subnormal, huge or NaN (m <= 0 included: |m| is what the quotient's magnitude depends on) -- the
// division itself decides.
struct DropBound {
  double m, lo, hi;
};
__device__ __forceinline__ DropBound drop_bound(double m) {
  DropBound d;
  d.m = m;
  const double t = 1e-8 * fabs(m);
  const bool ok = t >= 1e-290 && t <= 1e290;
  d.lo = ok ? t * (1.0 - 0x1p-40) : -1.0;
  d.hi = ok ? t * (1.0 + 0x1p-40) : __longlong_as_double(0x7ff0000000000000ll);
  return d;
}
__device__ __forceinline__ bool dropped(double b, const DropBound& d) {
  const double ab = fabs(b);
  if (ab < d.lo) return true;
  if (ab > d.hi) return false;
  return fabs(b / d.m) < 1e-8;
}

// PASS 0: partial maxima of the signed branch currents; PASS 1: node currents
template <class T, int K, int PASS>
__device__ __forceinline__ void dia_currents_body(const DiaCurrArgs<T>& a) {
  typedef DiaShape<T, T, K> SH;
  constexpr int CPL = SH::CPL, LPR = SH::LPR, TI = SH::TI, MELEMS = SH::MELEMS, MU = SH::MU;
  typedef SpmvVec<T, CPL> XV;
  __shared__ XV s_x[4][(TI + 2) * LPR];
  __shared__ T s_m[4][MELEMS];
  __shared__ T s_c[PASS == 1 ? 256 * CPL : 1];       // epilogue (b): the T-rounded currents of the column step, [TI][K]
  __shared__ double s_red[PASS == 0 ? 2 * 4 * K : 1];
  const int tid = threadIdx.x;
  const int t = tid / LPR;   // row of the tile owned by this lane
  const int lq = tid % LPR;  // which CPL-wide slice of the K columns
  const int c0 = lq * CPL;
  double mpos[CPL], mneg[CPL];
  DropBound dp[PASS == 1 ? CPL : 1], dn[PASS == 1 ? CPL : 1];
#pragma unroll
  for (int q = 0; q < CPL; ++q) mpos[q] = mneg[q] = -1e300;
  if (PASS == 1) {
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      dp[PASS == 1 ? q : 0] = drop_bound(a.maxcur[2 * (c0 + q)]);
      dn[PASS == 1 ? q : 0] = drop_bound(a.maxcur[2 * (c0 + q) + 1]);
    }
  }
  const bool accumulate = PASS == 1 && a.curr == nullptr;  // (block-uniform)

  const int ntiles = a.nstrips * a.nseg;
  // XCD-aware tile walk (see dia_cg_kernel)
  int t_first = blockIdx.x, t_last = ntiles, t_step = gridDim.x;
  if ((gridDim.x & 7) == 0) {
    const int xcd = blockIdx.x & 7, chunk = (ntiles + 7) >> 3;
    t_first = xcd * chunk + (blockIdx.x >> 3);
    t_last = min(ntiles, (xcd + 1) * chunk);
    t_step = gridDim.x >> 3;
  }
  for (int tile = t_first; tile < t_last; tile += t_step) {
    const int si = tile % a.nstrips, sj = tile / a.nstrips;
    const int i0 = si * TI;
    const int j0 = sj * a.seg, j1 = min(a.C, j0 + a.seg);
    const bool row_on = i0 + t < a.R;  // rows past the raster's last row belong to no tile
    XV xr, xh;  // the column in flight: vector entries of the tile's rows / of the two halo rows
    T mr[MU];
    auto load_column = [&](int jc) {
      // node id of tile row -1 (the halo row above) in raster column jc; ids outside [0, n) read as zero
      const int64_t base = (int64_t)jc * a.R + i0 - 1;
      {
        const int64_t id = base + 1 + t;
#pragma unroll
        for (int q = 0; q < CPL; ++q) xr.e[q] = T(0);
        if (id >= 0 && id < a.n) xr = *reinterpret_cast<const XV*>(a.x + (size_t)id * K + c0);
      }
      if (tid < 2 * LPR) {  // halo rows: tile row -1 (lanes 0..LPR-1) and tile row TI (lanes LPR..2LPR-1)
        const int64_t id = base + (tid < LPR ? 0 : TI + 1);
#pragma unroll
        for (int q = 0; q < CPL; ++q) xh.e[q] = T(0);
        if (id >= 0 && id < a.n) xh = *reinterpret_cast<const XV*>(a.x + (size_t)id * K + c0);
      }
#pragma unroll
      for (int u = 0; u < MU; ++u) {
        const int e = tid + u * 256;
        const int64_t g = base * 5 + e;
        mr[u] = (e < MELEMS && g >= 0 && g < a.n * 5) ? a.rows[g] : T(0);
      }
    };
    auto store_column = [&](int jc) {
      const int slot = jc & 3;
      s_x[slot][(t + 1) * LPR + lq] = xr;
      if (tid < 2 * LPR) s_x[slot][(tid < LPR ? 0 : TI + 1) * LPR + lq] = xh;
#pragma unroll
      for (int u = 0; u < MU; ++u) {
        const int e = tid + u * 256;
        if (e < MELEMS) s_m[slot][e] = mr[u];
      }
    };
    __syncthreads();  // previous tile finished with the ring
    load_column(j0 - 1);
    store_column(j0 - 1);
    load_column(j0);
    store_column(j0);
    load_column(j0 + 1);
    __syncthreads();
    // sliding 3x3 window of x: xw[dj][di] = x(row t-1+di of the tile, raster column j-1+dj)
    XV xw[3][3];
#pragma unroll
    for (int di = 0; di < 3; ++di) {
      xw[1][di] = s_x[(j0 - 1) & 3][(t + di) * LPR + lq];
      xw[2][di] = s_x[j0 & 3][(t + di) * LPR + lq];
    }
    for (int j = j0; j < j1; ++j) {
      store_column(j + 1);                  // the column loaded one step ago
      if (j + 2 <= j1) load_column(j + 2);  // next one in flight while this column is computed
      __syncthreads();
#pragma unroll
      for (int di = 0; di < 3; ++di) {
        xw[0][di] = xw[1][di];
        xw[1][di] = xw[2][di];
        xw[2][di] = s_x[(j + 1) & 3][(t + di) * LPR + lq];
      }
      const int64_t id = (int64_t)j * a.R + i0 + t;
      if (row_on) {
        const T* mc = s_m[j & 3];        // matrix rows of raster column j   (tile rows -1 .. TI at 5*(row+1))
        const T* mp = s_m[(j - 1) & 3];  // matrix rows of raster column j-1
        const int me = 5 * (t + 1);
        if (PASS == 0) {
          // the row's own stored entries: neighbours i+1, i+R-1, i+R, i+R+1
          const T w[4] = {mc[me + 1], mc[me + 2], mc[me + 3], mc[me + 4]};
          const XV* xn[4] = {&xw[1][2], &xw[2][0], &xw[2][1], &xw[2][2]};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (w[k] == T(0)) continue;
            const double g = fabs((double)w[k]);
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
              const double b = g * ((double)xw[1][1].e[q] - (double)xn[k]->e[q]);
              mpos[q] = b > mpos[q] ? b : mpos[q];
              mneg[q] = -b > mneg[q] ? -b : mneg[q];
            }
          }
        } else {
          // ascending column order, like the CSR row: i-R-1, i-R, i-R+1, i-1, i+1, i+R-1, i+R, i+R+1
          const T w[8] = {mp[me - 5 + 4], mp[me + 3], mp[me + 5 + 2], mc[me - 5 + 1], mc[me + 1], mc[me + 2], mc[me + 3], mc[me + 4]};
          const XV* xn[8] = {&xw[0][0], &xw[0][1], &xw[0][2], &xw[1][0], &xw[1][2], &xw[2][0], &xw[2][1], &xw[2][2]};
          XV cv;
#pragma unroll
          for (int q = 0; q < CPL; ++q) {
            const double vr = (double)xw[1][1].e[q];
            double in = 0.0, out = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              if (w[k] == T(0)) continue;
              const double g = fabs((double)w[k]);
              const bool up = k >= 4;  // the neighbour's id is larger than the row's
              const double xc = (double)xn[k]->e[q];
              // signed branch current of the edge in the reference's upper-triangular orientation (node_current_kernel)
              const double bpos = up ? g * (vr - xc) : g * (xc - vr);
              const double keep_pos = !dropped(bpos, dp[PASS == 1 ? q : 0]) ? bpos : 0.0;
              const double keep_neg = !dropped(bpos, dn[PASS == 1 ? q : 0]) ? -bpos : 0.0;
              const double into = up ? -keep_pos : keep_pos;
              const double outof = up ? -keep_neg : keep_neg;
              if (into > 0.0) in += into;
              if (outof > 0.0) out += outof;
            }
            cv.e[q] = (T)(in > out ? in : out);
          }
          if (!accumulate) {
            dia_store(reinterpret_cast<XV*>(a.curr + (size_t)id * K + c0), cv);
          } else {
#pragma unroll
            for (int q = 0; q < CPL; ++q) s_c[tid * CPL + q] = cv.e[q];  // = s_c[t * K + c0 + q]
          }
        }
      }
      if (accumulate) {
        // cum / max exactly as current_accumulate_kernel: one lane per node adds the node's columns in column order
        __syncthreads();
        if (row_on && lq == 0) {
          T s = a.cum ? a.cum[id] : T(0);
          T m = a.mx ? a.mx[id] : T(0);
          for (int c = 0; c < a.ncols; ++c) {
            const T v = s_c[t * K + c];
            const int wt = a.weight[c];
            for (int r = 0; r < wt; ++r) s += v;
            if (wt > 0 && v > m) m = v;
          }
          if (a.cum) a.cum[id] = s;
          if (a.mx) a.mx[id] = m;
        }
        // (the next write of s_c comes after the next step's barrier)
      }
    }
  }
  if (PASS == 0) {
    // lanes owning the same columns sit LPR apart: reduce over lane bits >= log2(LPR), then across the 4 waves via LDS
    const int lane = tid & 63, wv = tid >> 6;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      double vp = mpos[q], vn = mneg[q];
#pragma unroll
      for (int o = 32; o >= LPR; o >>= 1) {
        const double op = __shfl_xor(vp, o, 64), on = __shfl_xor(vn, o, 64);
        vp = op > vp ? op : vp;
        vn = on > vn ? on : vn;
      }
      if (lane < LPR) {
        s_red[(0 * 4 + wv) * K + lane * CPL + q] = vp;
        s_red[(1 * 4 + wv) * K + lane * CPL + q] = vn;
      }
    }
    __syncthreads();
    if (tid < K) {
      double vp = s_red[tid], vn = s_red[4 * K + tid];
      for (int ww = 1; ww < 4; ++ww) {
        const double op = s_red[ww * K + tid], on = s_red[(4 + ww) * K + tid];
        vp = op > vp ? op : vp;
        vn = on > vn ? on : vn;
      }
      a.part[((size_t)blockIdx.x * K + tid) * 2 + 0] = vp;
      a.part[((size_t)blockIdx.x * K + tid) * 2 + 1] = vn;
    }
  }
}

// pass 1: per-workgroup partial maxima of the signed branch currents in both orientations -> part[gridDim.x][K][2]
// (finished by branch_max_final_kernel)
template <class T, int K>
__global__ __launch_bounds__(256) void dia_branch_max_kernel(DiaCurrArgs<T> a) {
  dia_currents_body<T, K, 0>(a);
}

// pass 2: node currents -- stored interleaved like the voltages (a.curr), or accumulated into the cumulative / maximum map
// without ever being stored (a.curr == nullptr)
template <class T, int K>
__global__ __launch_bounds__(256) void dia_node_current_kernel(DiaCurrArgs<T> a) {
  dia_currents_body<T, K, 1>(a);
}

template <class T, int K>
inline DiaCurrArgs<T> dia_curr_args(const Dia<T>& D, const T* x, int& grid) {
  DiaCurrArgs<T> a;
  a.n = D.n;
  a.R = D.R;
  a.C = (int)(D.n / D.R);
  dia_tiling<T, T, K>(D, a.nstrips, a.nseg, a.seg, grid);
  a.rows = D.data();
  CS_REQUIRE(x != nullptr, CSGPU_INTERNAL, "lattice currents without a solution vector");
  a.x = x;
  a.part = nullptr;
  a.maxcur = nullptr;
  a.curr = a.cum = a.mx = nullptr;
  a.weight = nullptr;
  a.ncols = 0;
  return a;
}

// workgroups of the two passes (= rows of the partial maxima pass 1 writes)
template <class T, int K>
inline int dia_currents_grid(const Dia<T>& D) {
  return dia_grid<T, T, K>(D);
}

// maxcur[K][2] = largest signed branch current of every column in both orientations; part: dia_currents_grid rows of [K][2]
template <class T, int K>
inline void dia_branch_max(const Dia<T>& D, const T* x, double* part, double* maxcur, hipStream_t st) {
  int grid;
  DiaCurrArgs<T> a = dia_curr_args<T, K>(D, x, grid);
  a.part = part;
  hipLaunchKernelGGL((dia_branch_max_kernel<T, K>), dim3(grid), dim3(256), 0, st, a);
  hipLaunchKernelGGL((branch_max_final_kernel<K>), dim3(1), dim3(256), 0, st, (const double*)part, grid, maxcur);
}

// curr != null: curr[n][K] = node currents. curr == null: cum / mx (either may be null) take the columns c < ncols with their
// weights, as current_accumulate_kernel would from stored currents.
template <class T, int K>
inline void dia_node_currents(const Dia<T>& D, const T* x, const double* maxcur, T* curr, T* cum, T* mx, const int* weight,
                              int ncols, hipStream_t st) {
  int grid;
  DiaCurrArgs<T> a = dia_curr_args<T, K>(D, x, grid);
  a.maxcur = maxcur;
  a.curr = curr;
  a.cum = cum;
  a.mx = mx;
  a.weight = weight;
  a.ncols = ncols;
  CS_REQUIRE(curr != nullptr || (weight != nullptr && ncols <= K), CSGPU_INTERNAL, "lattice currents: nothing to write");
  hipLaunchKernelGGL((dia_node_current_kernel<T, K>), dim3(grid), dim3(256), 0, st, a);
}

}  // namespace csgpu
