// reorder.h -- locality reordering of a network graph on the device (csgpu_opts.reorder).
//
// Network mode hands the solver a graph whose node ids are whatever the edge-list file used (the reference builds it with
// sparse(i, j, v) straight from the file, src/network/pairwise.jl:31-65): no locality, and the CSR products gather x through
// columns that are all over the vector. This file computes perm[node] = device row at set-up and the matrix B = P A P' in CSR;
// csgpu.hip translates ids and n-vectors at the C ABI (the translation cell space already has), so that a caller never
// sees the device numbering.
//
// Ordering: level sets of a breadth-first search from one seed per connected component, Cuthill-McKee style.
//   1. components (raster.h, connected_components) -> seed of component c = its LEAST CENTRAL node: the one with the fewest
//      walks of length 4 (four passes over the entries; ties to the smallest id). That is a node at the rim of the graph,
//      where a Cuthill-McKee order wants to start: levels from the rim are about half as wide as from the middle (CPU check on
//      bench.geometric_network, mean |col - row| against scipy's reverse Cuthill-McKee: 1.84 / 2.02 x from the smallest id at
//      n = 3000 / 6e4; 1.18 / 1.30 / 1.30 x from this seed at n = 3000 / 6e4 / 1e6, 0.93 / 1.02 / 1.02 x after step 4). The
//      classic way to such a seed -- search from anywhere, start again from the last level -- costs a whole search more.
//   2. frontier-driven BFS from all seeds at once: level[v] = distance to the seed of v's component. Every node enters ONE
//      queue of n entries exactly once; one small launch per level, sixteen lanes a node, launched in chunks without a host
//      round trip per level (the host looks at the last level of a chunk only).
//   3. stable sort of the nodes by key = (component, level) -- dense: key = first key of the component + level, at most n keys.
//   4. one Cuthill-McKee refinement: inside a level the nodes are ordered by the position of their FIRST neighbour in the order
//      of step 3 (a node of level L has it in level L - 1, so one stable sort by that position keeps components and levels in
//      place).
// Determinism: the walk counts are sums in row order, level[] is the BFS distance (whatever order the atomics arrive in),
// seeds and last levels come from atomicMin / atomicMax, the
// sort is a stable LSD radix sort without atomics, ties fall to the node id. The order of the BFS queue is NOT deterministic
// and is never used for anything but the traversal.
//
// Sort: least-significant-digit radix sort of (key, node) pairs, 4 bits a pass. Every thread owns a contiguous run of
// kRadixRun pairs: pass 1 counts its digits, the counts are laid out digit-major and scanned (prims.h), pass 2 walks the run
// again in order and writes every pair to its place -- stable by construction, no atomics, no shared memory.
//
// Permutation: row lengths gathered through the order -> scan -> columns relabelled into the new rows (unsorted) -> every
// entry is put at the rank of its new column inside its row (eight lanes a row; a row of length L costs L^2 / 8 comparisons
// per lane, which is nothing at the mean degree of 10 - 20 of a network and merely slow for the hub of a star). Values are
// moved, never recomputed. The same two kernels, run the other way, give entry_map[k of the caller] = k on the device.
#pragma once
#include <chrono>

#include "raster.h"

namespace csgpu {

static const int kRadixRun = 16;    // pairs per thread of the radix sort
static const int kBfsGridCap = 512;  // workgroups of one BFS level
static const int kWalkRounds = 4;    // rounds of walk counting that pick the seeds

// the seeds are level 0 and the first ncomp entries of the queue
__global__ __launch_bounds__(256) void reorder_seed_kernel(int ncomp, const int* __restrict__ seed, int* __restrict__ level,
                                                           int* __restrict__ queue, int* __restrict__ cnt) {
  for (int c = blockIdx.x * 256 + threadIdx.x; c < ncomp; c += gridDim.x * 256) {
    queue[c] = seed[c];
    level[seed[c]] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[0] = ncomp;
}

// One BFS level. The nodes queue[lo .. hi), lo = bounds[L], hi = lo + cnt[L], claim their unvisited neighbours for level
// L + 1 and append them behind hi: level L + 1 starts where level L ends, so an append is queue[hi + cnt[L + 1]++] and the
// launch of level L + 1 finds its own range without anybody having to wait for the last workgroup of this one (cnt is
// zeroed before the search; bounds[L + 1] = hi is written by one thread for the next launch). Sixteen lanes share a node:
// a row of a network (10 - 20 entries) is ONE round of loads -- with a thread per node the level took as long as the
// longest row's chain of dependent loads and atomics, 50 us at n = 1e6, where this form takes about 10. A launch whose level
// is empty falls straight through, which is how the launches past the last level end.
// An off-diagonal entry that is not negative is no edge (raster.h, cc_hook_kernel): the search walks the graph the components
// were found on, so that the levels of a component are 0 .. its last one without a gap. level[] is read plainly first: a
// stale -1 only costs a CAS that fails (a node's level is written once, by the CAS that wins).
static const int kBfsLanes = 16;
template <class T>
__global__ __launch_bounds__(256) void reorder_bfs_kernel(const int* __restrict__ rp, const int* __restrict__ ci,
                                                          const T* __restrict__ va, int L, int* level, int* queue, int* bounds,
                                                          int* cnt) {
  const int lo = bounds[L], hi = lo + cnt[L];
  if (blockIdx.x == 0 && threadIdx.x == 0) bounds[L + 1] = hi;
  const int lane = threadIdx.x % kBfsLanes;
  const int groups = gridDim.x * (256 / kBfsLanes);
  for (int q = lo + (blockIdx.x * 256 + threadIdx.x) / kBfsLanes; q < hi; q += groups) {
    const int u = queue[q];
    const int e = rp[u + 1];
    for (int k = rp[u] + lane; k < e; k += kBfsLanes) {
      if (!(va[k] < T(0))) continue;
      const int v = ci[k];
      if (level[v] < 0 && atomicCAS(&level[v], -1, L + 1) == -1) queue[hi + atomicAdd(&cnt[L + 1], 1)] = v;
    }
  }
}

// ---- the seeds: the least central node of every component ---------------------------------------------------------------
// x_out[u] = sum of x_in over u's neighbours (x_in null: ones): after k rounds the number of walks of length k from u. A
// node at the rim of a graph with locality has a fraction of the walks of a node inside it (half the disc at an edge of the
// geometric network, a quarter in a corner), and four rounds average over enough nodes for the smallest count to sit at the
// rim -- the peripheral start a Cuthill-McKee order wants, for four passes over the entries instead of a search of its own
// (the classic way: search from anywhere, start again from the last level; 11 ms of 30 at n = 1e6).
template <class T>
__global__ __launch_bounds__(256) void reorder_walks_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci,
                                                            const T* __restrict__ va, const double* __restrict__ x_in,
                                                            double* __restrict__ x_out) {
  for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) {
    double s = 0.0;
    for (int k = rp[u]; k < rp[u + 1]; ++k)
      if (va[k] < T(0)) s += x_in ? x_in[ci[k]] : 1.0;  // (entries in row order: the same sum on every run)
    x_out[u] = s;
  }
}
// least[c] = smallest walk count in component c, as the bits of the (non-negative) double: ordered like the value
__global__ __launch_bounds__(256) void reorder_least_kernel(int n, const int* __restrict__ comp, const double* __restrict__ x,
                                                            unsigned long long* least) {
  for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) {
    const unsigned long long key = (unsigned long long)__double_as_longlong(x[u]);
    if (key < least[comp[u]]) atomicMin(&least[comp[u]], key);
  }
}
// seed[c] = smallest node id among the nodes of component c with that count (seed pre-set to INT_MAX)
__global__ __launch_bounds__(256) void reorder_least_node_kernel(int n, const int* __restrict__ comp, const double* __restrict__ x,
                                                                 const unsigned long long* __restrict__ least, int* seed) {
  for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256)
    if ((unsigned long long)__double_as_longlong(x[u]) == least[comp[u]] && u < seed[comp[u]]) atomicMin(&seed[comp[u]], u);
}
__global__ __launch_bounds__(256) void fill_ull_kernel(unsigned long long* __restrict__ p, int64_t n, unsigned long long v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}

// maxlev[c] = last level of component c
__global__ __launch_bounds__(256) void reorder_maxlev_kernel(int n, const int* __restrict__ comp, const int* __restrict__ level,
                                                             int* maxlev) {
  for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256)
    if (level[u] > maxlev[comp[u]]) atomicMax(&maxlev[comp[u]], level[u]);
}
// nlev[c] = maxlev[c] + 1 (one trailing 0 for the scan's total)
__global__ __launch_bounds__(256) void reorder_nlev_kernel(int ncomp, const int* __restrict__ maxlev, int* __restrict__ nlev) {
  for (int c = blockIdx.x * 256 + threadIdx.x; c <= ncomp; c += gridDim.x * 256) nlev[c] = c < ncomp ? maxlev[c] + 1 : 0;
}
// key[u] = first key of u's component + level[u];  id[u] = u
__global__ __launch_bounds__(256) void reorder_level_key_kernel(int n, const int* __restrict__ comp, const int* __restrict__ level,
                                                                const int* __restrict__ keybase, int* __restrict__ key,
                                                                int* __restrict__ id) {
  for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) {
    key[u] = keybase[comp[u]] + level[u];
    id[u] = u;
  }
}
// pos[order[r]] = r
__global__ __launch_bounds__(256) void reorder_invert_kernel(int n, const int* __restrict__ order, int* __restrict__ pos) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) pos[order[r]] = r;
}
// Cuthill-McKee key of step 5: a seed keeps its position, every other node gets 1 + the smallest position among its neighbours
template <class T>
__global__ __launch_bounds__(256) void reorder_first_neighbour_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci,
                                                                      const T* __restrict__ va, const int* __restrict__ level, const int* __restrict__ pos,
                                                                      int* __restrict__ key, int* __restrict__ id) {
  for (int u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) {
    int m = pos[u];
    if (level[u] > 0) {
      for (int k = rp[u]; k < rp[u + 1]; ++k) {
        const int v = ci[k];
        if (v != u && va[k] < T(0)) m = min(m, pos[v] + 1);
      }
    }
    key[u] = m;
    id[u] = u;
  }
}
// cell2node-style inverse for the boundary kernels of raster.h: out[r] = order[r] + 1
__global__ __launch_bounds__(256) void reorder_plus_one_kernel(int n, const int* __restrict__ order, int* __restrict__ out) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) out[r] = order[r] + 1;
}
// out[map[i]] = in[i]
__global__ __launch_bounds__(256) void reorder_scatter_int_kernel(int n, const int* __restrict__ map, const int* __restrict__ in,
                                                                  int* __restrict__ out) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[map[i]] = in[i];
}

// ---- stable LSD radix sort of (key, id) pairs, 4 bits a pass ------------------------------------------------------------
// hist[d * G + g] = pairs with digit d in the run of thread g
__global__ __launch_bounds__(256) void radix_count_kernel(int n, const int* __restrict__ key, int shift, int G,
                                                          int* __restrict__ hist) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  int cnt[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) cnt[d] = 0;
  const int i0 = g * kRadixRun, i1 = min(n, i0 + kRadixRun);
  for (int i = i0; i < i1; ++i) {
    const int dig = (key[i] >> shift) & 15;
#pragma unroll
    for (int d = 0; d < 16; ++d) cnt[d] += dig == d ? 1 : 0;
  }
#pragma unroll
  for (int d = 0; d < 16; ++d) hist[(size_t)d * G + g] = cnt[d];
}
// hist scanned: first place of the run's pairs with digit d
__global__ __launch_bounds__(256) void radix_place_kernel(int n, const int* __restrict__ key_in, const int* __restrict__ id_in,
                                                          int shift, int G, const int* __restrict__ hist,
                                                          int* __restrict__ key_out, int* __restrict__ id_out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  int pos[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) pos[d] = hist[(size_t)d * G + g];
  const int i0 = g * kRadixRun, i1 = min(n, i0 + kRadixRun);
  for (int i = i0; i < i1; ++i) {
    const int k = key_in[i];
    const int dig = (k >> shift) & 15;
    int p = 0;
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      p = dig == d ? pos[d] : p;
      pos[d] += dig == d ? 1 : 0;
    }
    key_out[p] = k;
    id_out[p] = id_in[i];
  }
}

// Sorts the n pairs (key, id) by key (keys in [0, 2^bits)), equal keys in their incoming order. key / id and the two spare
// buffers are n ints each; returns true when the result lies in (key2, id2).
inline bool radix_sort_pairs(int n, int bits, int* key, int* id, int* key2, int* id2, hipStream_t st) {
  const int G = ceil_div(n, kRadixRun);
  DBuf hist = dalloc<int>((size_t)16 * G);
  bool flipped = false;
  for (int shift = 0; shift < bits; shift += 4) {
    hipLaunchKernelGGL(radix_count_kernel, dim3(ceil_div(G, 256)), dim3(256), 0, st, n, (const int*)(flipped ? key2 : key), shift,
                       G, dptr<int>(hist));
    exclusive_scan_i32(dptr<int>(hist), (int64_t)16 * G, st);
    hipLaunchKernelGGL(radix_place_kernel, dim3(ceil_div(G, 256)), dim3(256), 0, st, n, (const int*)(flipped ? key2 : key),
                       (const int*)(flipped ? id2 : id), shift, G, (const int*)dptr<int>(hist), flipped ? key : key2,
                       flipped ? id : id2);
    flipped = !flipped;
  }
  check_launch("radix sort");
  CS_HIP(hipStreamSynchronize(st));  // `hist` is released on return
  return flipped;
}

inline int bits_for(int64_t nkeys) {
  int b = 1;
  while (((int64_t)1 << b) < nkeys) ++b;
  return b;
}

// level[] of the BFS from `seed` (one per component); returns the number of launches (diagnostics). bounds, cnt: n + 2 ints.
// The levels are launched in chunks without a host round trip per level: the host looks at the last level of a chunk only,
// to see whether the search is over and how wide the frontier has become (which sizes the launches of the next chunk).
template <class T>
inline int reorder_bfs(int n, const int* rp, const int* ci, const T* va, int ncomp, const int* seed, int* level, int* queue,
                       int* bounds, int* cnt, hipStream_t st) {
  hipLaunchKernelGGL(fill_int_kernel, dim3(grid_for(n)), dim3(256), 0, st, level, (int64_t)n, -1);
  CS_HIP(hipMemsetAsync(cnt, 0, ((size_t)n + 2) * sizeof(int), st));
  CS_HIP(hipMemsetAsync(bounds, 0, sizeof(int), st));
  hipLaunchKernelGGL(reorder_seed_kernel, dim3(grid_for(ncomp)), dim3(256), 0, st, ncomp, seed, level, queue, cnt);
  auto grid_of = [](int width) { return std::max(16, std::min(grid_for((int64_t)width * kBfsLanes * 2), kBfsGridCap)); };
  int L = 0, chunk = 32, g = grid_of(ncomp);
  // launch L reads cnt[L], appends through cnt[L + 1] and writes bounds[L + 1]: L <= n (a graph of n nodes has at most n
  // levels, so level n is empty and its launch appends nothing)
  while (L <= n) {
    const int end = (int)std::min<int64_t>((int64_t)n + 1, (int64_t)L + chunk);
    for (; L < end; ++L) hipLaunchKernelGGL((reorder_bfs_kernel<T>), dim3(g), dim3(256), 0, st, rp, ci, va, L, level, queue, bounds, cnt);
    int width = 0;  // of the last level launched
    CS_HIP(hipMemcpyAsync(&width, cnt + (L - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    CS_HIP(hipStreamSynchronize(st));
    if (width == 0) break;  // an empty level: the search is over
    g = grid_of(width);
    chunk = std::min(chunk * 2, 128);
  }
  check_launch("reorder BFS");
  return L;
}

struct ReorderResult {
  DBuf perm;     // [n] node -> device row
  DBuf order;    // [n] device row -> node
  DBuf comp;     // [n] component of every NODE (dense index, components ordered by their smallest node id)
  int ncomp = 0;
  int levels = 0;  // BFS launches of the second search (diagnostics)
};

// The ordering (steps 1 - 4 above) of the symmetric CSR graph (rp, ci); va decides what is an edge for the components only
// and the searches alike (raster.h: negative off-diagonal entries).
template <class T>
inline void reorder_compute(int n, const int* rp, const int* ci, const T* va, ReorderResult& out, hipStream_t st) {
  const bool verbose = knobs().verbose;
  auto t_last = std::chrono::steady_clock::now();
  auto phase = [&](const char* what) {  // (verbose only: one line per phase, host clock after a sync)
    if (!verbose) return;
    CS_HIP(hipStreamSynchronize(st));
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "csgpu: reorder: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  };
  out.comp = dalloc<int>((size_t)n);
  out.ncomp = connected_components<T>(n, rp, ci, va, dptr<int>(out.comp), st);
  phase("components");
  const int ncomp = out.ncomp;
  const int* comp = dptr<int>(out.comp);
  DBuf seed = dalloc<int>((size_t)ncomp), maxlev = dalloc<int>((size_t)ncomp), nlev = dalloc<int>((size_t)ncomp + 1);
  DBuf level = dalloc<int>((size_t)n), queue = dalloc<int>((size_t)n), bounds = dalloc<int>((size_t)n + 2), cnt = dalloc<int>((size_t)n + 2);
  const int gn = grid_for(n), gc = grid_for(ncomp);
  // minimum / maximum per component through one address each: a SMALL grid, so that all but the first few thousand threads find
  // the running value in their plain read and skip the atomic (a full grid: 6.2 ms of contention at n = 5e6, one component)
  const int gs = std::min(gn, 64);
  {  // seeds: the node with the fewest walks of length kWalkRounds in its component
    DBuf xa = dalloc<double>((size_t)n), xb = dalloc<double>((size_t)n), least = dalloc<unsigned long long>((size_t)ncomp);
    double *x0 = dptr<double>(xa), *x1 = dptr<double>(xb);
    for (int r = 0; r < kWalkRounds; ++r) {
      hipLaunchKernelGGL((reorder_walks_kernel<T>), dim3(gn), dim3(256), 0, st, n, rp, ci, va, r == 0 ? (const double*)nullptr : (const double*)x0, x1);
      std::swap(x0, x1);
    }
    hipLaunchKernelGGL(fill_ull_kernel, dim3(gc), dim3(256), 0, st, dptr<unsigned long long>(least), (int64_t)ncomp, ~0ull);
    hipLaunchKernelGGL(reorder_least_kernel, dim3(gs), dim3(256), 0, st, n, comp, (const double*)x0, dptr<unsigned long long>(least));
    hipLaunchKernelGGL(fill_int_kernel, dim3(gc), dim3(256), 0, st, dptr<int>(seed), (int64_t)ncomp, 0x7fffffff);
    hipLaunchKernelGGL(reorder_least_node_kernel, dim3(gn), dim3(256), 0, st, n, comp, (const double*)x0,
                       (const unsigned long long*)dptr<unsigned long long>(least), dptr<int>(seed));
    check_launch("reorder seeds");
    CS_HIP(hipStreamSynchronize(st));  // xa / xb / least are released here
  }
  phase("seeds");
  out.levels = reorder_bfs<T>(n, rp, ci, va, ncomp, dptr<int>(seed), dptr<int>(level), dptr<int>(queue), dptr<int>(bounds),
                              dptr<int>(cnt), st);
  phase("search");
  // dense keys (component, level)
  hipLaunchKernelGGL(fill_int_kernel, dim3(gc), dim3(256), 0, st, dptr<int>(maxlev), (int64_t)ncomp, 0);
  hipLaunchKernelGGL(reorder_maxlev_kernel, dim3(gs), dim3(256), 0, st, n, comp, (const int*)dptr<int>(level), dptr<int>(maxlev));
  hipLaunchKernelGGL(reorder_nlev_kernel, dim3(grid_for(ncomp + 1)), dim3(256), 0, st, ncomp, (const int*)dptr<int>(maxlev),
                     dptr<int>(nlev));
  DBuf total = dalloc<int>(1);
  exclusive_scan_i32(dptr<int>(nlev), (int64_t)ncomp + 1, st, dptr<int>(total));
  const int nkeys = read_int(dptr<int>(total), st);
  CS_REQUIRE(nkeys >= 1 && nkeys <= n, CSGPU_INTERNAL, "reorder: level keys out of range");
  // queue / bounds are free again: they serve as the sort's second pair of buffers
  DBuf key = dalloc<int>((size_t)n), id = dalloc<int>((size_t)n);
  int *k1 = dptr<int>(key), *i1 = dptr<int>(id), *k2 = dptr<int>(queue), *i2 = dptr<int>(bounds);
  hipLaunchKernelGGL(reorder_level_key_kernel, dim3(gn), dim3(256), 0, st, n, comp, (const int*)dptr<int>(level),
                     (const int*)dptr<int>(nlev), k1, i1);
  const int* order = radix_sort_pairs(n, bits_for(nkeys), k1, i1, k2, i2, st) ? i2 : i1;
  phase("sort by (component, level)");
  // Cuthill-McKee refinement inside the levels
  DBuf pos = dalloc<int>((size_t)n);
  hipLaunchKernelGGL(reorder_invert_kernel, dim3(gn), dim3(256), 0, st, n, order, dptr<int>(pos));
  hipLaunchKernelGGL((reorder_first_neighbour_kernel<T>), dim3(gn), dim3(256), 0, st, n, rp, ci, va, (const int*)dptr<int>(level),
                     (const int*)dptr<int>(pos), k1, i1);
  order = radix_sort_pairs(n, bits_for((int64_t)n + 1), k1, i1, k2, i2, st) ? i2 : i1;
  out.order = dalloc<int>((size_t)n);
  out.perm = dalloc<int>((size_t)n);
  CS_HIP(hipMemcpyAsync(out.order.p, order, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(reorder_invert_kernel, dim3(gn), dim3(256), 0, st, n, order, dptr<int>(out.perm));
  check_launch("reorder");
  CS_HIP(hipStreamSynchronize(st));
  phase("sort by first neighbour");
}

// ---- B = P A P' ---------------------------------------------------------------------------------------------------------
// dst row r is src row rowsrc[r]; a src column c becomes colmap[c]
__global__ __launch_bounds__(256) void permute_rowlen_kernel(int n, const int* __restrict__ rowsrc, const int* __restrict__ src_rp,
                                                             int* __restrict__ dst_rp) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r <= n; r += gridDim.x * 256) {
    const int s = r < n ? rowsrc[r] : 0;
    dst_rp[r] = r < n ? src_rp[s + 1] - src_rp[s] : 0;
  }
}
// eight lanes a row: the new columns, still in the order of the source row
__global__ __launch_bounds__(256) void permute_relabel_kernel(int n, const int* __restrict__ rowsrc, const int* __restrict__ src_rp,
                                                              const int* __restrict__ src_ci, const int* __restrict__ colmap,
                                                              const int* __restrict__ dst_rp, int* __restrict__ newcol) {
  const int lane = threadIdx.x & 7;
  for (int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3; r < n; r += ((int64_t)gridDim.x * 256) >> 3) {
    const int s0 = src_rp[rowsrc[r]], d0 = dst_rp[r], len = dst_rp[r + 1] - d0;
    for (int j = lane; j < len; j += 8) newcol[d0 + j] = colmap[src_ci[s0 + j]];
  }
}
// every entry to the rank of its new column in its row (ties -- duplicate columns -- keep their order); dst_ci / dst_va /
// map may be null; map[k in dst] = k in src. col_base >= 0: the new columns are col_base-based and map = -1 where dst row >=
// dst column (the entries below and on the diagonal).
template <class T>
__global__ __launch_bounds__(256) void permute_place_kernel(int n, const int* __restrict__ rowsrc, const int* __restrict__ src_rp,
                                                            const T* __restrict__ src_va, const int* __restrict__ dst_rp,
                                                            const int* __restrict__ newcol, int* __restrict__ dst_ci,
                                                            T* __restrict__ dst_va, int* __restrict__ map, int col_base) {
  const int lane = threadIdx.x & 7;
  for (int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3; r < n; r += ((int64_t)gridDim.x * 256) >> 3) {
    const int s0 = src_rp[rowsrc[r]], d0 = dst_rp[r], len = dst_rp[r + 1] - d0;
    for (int j = lane; j < len; j += 8) {
      const int c = newcol[d0 + j];
      int rank = 0;
      for (int i = 0; i < len; ++i) {
        const int ci = newcol[d0 + i];
        rank += (ci < c || (ci == c && i < j)) ? 1 : 0;
      }
      if (dst_ci) dst_ci[d0 + rank] = c;
      if (dst_va) dst_va[d0 + rank] = src_va[s0 + j];
      if (map) map[d0 + rank] = (col_base >= 0 && (int)r + col_base >= c) ? -1 : s0 + j;
    }
  }
}

// B = P A P' with sorted rows; B's values are A's, moved
template <class T>
inline void permute_symmetric(const Csr<T>& A, const int* perm, const int* order, Csr<T>& B, hipStream_t st) {
  const int n = A.nrows;
  B.nrows = B.ncols = n;
  B.nnz = A.nnz;
  B.rowptr.alloc((size_t)(n + 1) * sizeof(int));
  B.col.alloc((size_t)std::max<int64_t>(A.nnz, 1) * sizeof(int));
  B.val.alloc((size_t)std::max<int64_t>(A.nnz, 1) * sizeof(T));
  hipLaunchKernelGGL(permute_rowlen_kernel, dim3(grid_for(n + 1)), dim3(256), 0, st, n, order, A.rp(), B.rp());
  exclusive_scan_i32(B.rp(), (int64_t)n + 1, st);
  if (A.nnz > 0) {
    DBuf newcol = dalloc<int>((size_t)A.nnz);
    const int g = grid_for((int64_t)n * 8);
    hipLaunchKernelGGL(permute_relabel_kernel, dim3(g), dim3(256), 0, st, n, order, A.rp(), A.ci(), perm, (const int*)B.rp(),
                       dptr<int>(newcol));
    hipLaunchKernelGGL((permute_place_kernel<T>), dim3(g), dim3(256), 0, st, n, order, A.rp(), A.va(), (const int*)B.rp(),
                       (const int*)dptr<int>(newcol), B.ci(), B.va(), (int*)nullptr, -1);
    check_launch("symmetric permutation");
    CS_HIP(hipStreamSynchronize(st));  // newcol is released on return
  }
}

// entry_map[k of the caller's matrix] = k of the device matrix B for the caller's upper-triangular entries (row < col),
// -1 elsewhere: the permutation run backwards (the caller's row i is B's row perm[i], B's column d is the caller's
// order1[d] - 1; order1 is the 1-based inverse the boundary kernels keep)
template <class T>
inline void build_entry_map(const Csr<T>& B, const int* perm, const int* order1, DBuf& entry_map, hipStream_t st) {
  const int n = B.nrows;
  entry_map = dalloc<int>((size_t)std::max<int64_t>(B.nnz, 1));
  if (B.nnz == 0) return;
  DBuf rp_api = dalloc<int>((size_t)n + 1), newcol = dalloc<int>((size_t)B.nnz);
  hipLaunchKernelGGL(permute_rowlen_kernel, dim3(grid_for(n + 1)), dim3(256), 0, st, n, perm, B.rp(), dptr<int>(rp_api));
  exclusive_scan_i32(dptr<int>(rp_api), (int64_t)n + 1, st);
  const int g = grid_for((int64_t)n * 8);
  hipLaunchKernelGGL(permute_relabel_kernel, dim3(g), dim3(256), 0, st, n, perm, B.rp(), B.ci(), order1,
                     (const int*)dptr<int>(rp_api), dptr<int>(newcol));
  hipLaunchKernelGGL((permute_place_kernel<T>), dim3(g), dim3(256), 0, st, n, perm, B.rp(), (const T*)nullptr,
                     (const int*)dptr<int>(rp_api), (const int*)dptr<int>(newcol), (int*)nullptr, (T*)nullptr,
                     dptr<int>(entry_map), 1);  // (1-based columns)
  check_launch("entry map");
  CS_HIP(hipStreamSynchronize(st));
}

// out[p * nnz + k] = map[k] >= 0 ? in[p * nnz + map[k]] : 0   (branch currents back at the caller's entry positions)
template <class T>
__global__ __launch_bounds__(256) void gather_entries_kernel(int64_t nnz, int ncols, const int* __restrict__ map,
                                                             const T* __restrict__ in, T* __restrict__ out) {
  const int64_t total = nnz * ncols;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t p = t / nnz, k = t % nnz;
    const int m = map[k];
    out[t] = m >= 0 ? in[p * nnz + m] : T(0);
  }
}

// mean |col - row| of the stored entries: per-workgroup partial sums (the host adds them in order)
__global__ __launch_bounds__(256) void span_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci,
                                                   double* __restrict__ part) {
  __shared__ double sm[4];
  double s = 0.0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256)
    for (int k = rp[r]; k < rp[r + 1]; ++k) s += (double)abs(ci[k] - r);
  s = block_sum_256(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
template <class T>
inline double mean_span(const Csr<T>& A, hipStream_t st) {
  if (A.nnz <= 0 || A.nrows <= 0) return 0.0;
  const int g = std::min(grid_for(A.nrows), 1024);
  DBuf part = dalloc<double>((size_t)g);
  hipLaunchKernelGGL(span_kernel, dim3(g), dim3(256), 0, st, A.nrows, A.rp(), A.ci(), dptr<double>(part));
  std::vector<double> h((size_t)g);
  CS_HIP(hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  CS_HIP(hipStreamSynchronize(st));
  double s = 0.0;
  for (double v : h) s += v;
  return s / (double)A.nnz / (double)A.nrows;
}

}  // namespace csgpu
