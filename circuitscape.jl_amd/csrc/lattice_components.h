// lattice_components.h -- connected components of a raster graph straight from the lattice form (no CSR matrix).
//
// The algorithm of raster.h (connected_components: min-label hooking + pointer jumping, invariant f[x] <= x and f[x] in
// x's component, fixed point = every row carries its component's smallest row id) with the hooking pass driven by
// Dia<T>::rows[n][5] instead of rp / ci / va. Row i stores its own diagonal and its four FORWARD couplings, to rows
// i + 1, i + R - 1, i + R, i + R + 1 (R = lattice period); a coupling is an edge iff its stored value is NEGATIVE -- the rule
// of cc_hook_kernel. A zero is an absent edge: the +1 slot of a column's last row, the +R-1 slot of its first row, the
// +R+1 slot of its last row, the diagonal slots of a four-neighbour raster, everything around a NODATA cell, the halo. The
// slots wrap in the numbering (i + 1 of a column's last row is the next column's first row), so the stored value decides,
// never the offset.
//
// One thread per row reads the row's four forward values and hooks BOTH endpoints of every edge it finds, so every edge
// is seen exactly once per round and no neighbour's row of values is fetched. Algorithmic bytes of a round (T = value
// type): n*5*T of matrix (the four values of a row share their cache lines with its diagonal; consecutive lanes read
// consecutive rows) + the labels: f[i] and up to four neighbours' f, all within 2 raster columns of i, and the atomics
// of the rows that changed. The CSR pass reads nnz*(T+4) + (n+1)*4 (nnz ~ 9 n) and the same labels twice over (both
// directions of every edge).
#pragma once
#include "raster.h"

namespace csgpu {

// No barrier, no LDS, no cross-lane operation: lanes of a wave may leave the loop at different trip counts.
template <class T>
__global__ __launch_bounds__(256) void dia_cc_hook_kernel(int64_t n, int R, const T* __restrict__ rows, int* __restrict__ f,
                                                          int* __restrict__ changed) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const T* __restrict__ r = rows + i * 5;
    const int64_t nb[4] = {i + 1, i + R - 1, i + R, i + R + 1};
    const int fi = f[i];
    int lab[4];
    int m = fi;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool edge = nb[s] < n && r[s + 1] < T(0);
      lab[s] = edge ? f[nb[s]] : -1;  // (-1: no edge; labels are row ids >= 0)
      if (edge) m = min(m, lab[s]);
    }
    bool any = false;
    if (m < fi) {
      atomicMin(&f[fi], m);  // hook i's current representative under the smallest label seen across its forward edges
      atomicMin(&f[i], m);
      any = true;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (lab[s] > m) {      // the far end of the edge holds the larger label: the same pair of hooks on its side
        atomicMin(&f[lab[s]], m);
        atomicMin(&f[nb[s]], m);
        any = true;
      }
    if (any) *changed = 1;
  }
}

// label[row] = dense component index (components ordered by their smallest row id) -- what connected_components returns
// on the CSR form dia_to_csr builds from the same lattice form; returns the number of components.
template <class T>
inline int dia_connected_components(const Dia<T>& dia, int* label, hipStream_t st) {
  CS_REQUIRE(dia.n < ((int64_t)1 << 31) - 1, CSGPU_INTERNAL, "lattice form with more rows than int32 labels can number");
  const int64_t n = dia.n;
  const int R = dia.R;
  const T* rows = dia.data();
  return connected_components_rounds((int)n, label, st, [&](int g, int* f, int* changed) {
    hipLaunchKernelGGL((dia_cc_hook_kernel<T>), dim3(g), dim3(256), 0, st, n, R, rows, f, changed);
  });
}

}  // namespace csgpu
