// Every assembled product y = A x (+ the fused dot x.Ax) of the library, and the one place that chooses among them.
//
// CSR stays the canonical storage (assembly output, host access).  Eight kernel families multiply from it (ProductKind, pyn_internal.h):
//   PK_RAW      spmv_kernel<32>: 32 lanes per scalar row, any block shape, needs nothing but the graph
//   PK_SELL, PK_SELLP, PK_SELLB_X, PK_SELLB_D
//               a SELL-64 image of the values (sliced ELLPACK, slice height = one wavefront, lane == scalar row: 512-B value loads, no
//               cross-lane reduction), scalar / block, explicit columns / node-level column-pattern dictionary.  The image is a
//               solver-side copy rebuilt when values change (PETSc analogue: MatAssemblyEnd building the inode structures of MatMult)
//   PK_CSRL, PK_CSRLB
//               lane per scalar row over LDS-staged contiguous runs of the CSR values, columns from the dictionary: no image
//   PK_BCSR     8 .. 64 lanes per node row straight from the block-CSR values: no image, the only product of a compact matrix
// pyn_sell_ensure resolves one ProductPlan per matrix and value version: shared structure (dictionary per graph, slices per block shape),
// then product_choose -- a pure host function of a few facts and the knobs, the only reader of the product knobs -- then the image, if
// the choice needs one.  pyn_sell_spmv_range2 launches from a plan: ranges, grid, one switch over the kind, the record.
#include <hipcub/hipcub.hpp>

#include "pyn_internal.h"

namespace {

constexpr int PAT_MAX = 256;   // dictionary size limit (LDS: PAT_MAX * PAT_W * 4 B = 32 KB)
constexpr int PAT_W = 32;      // max row length in dictionary mode

constexpr int SH = 64;  // slice height

// Block matrices (br x bc per graph edge) are handled as their scalar expansion: scalar row
// r = i*br + p has len_i*bc entries, contiguous in the canonical value array at
// (rowptr[i]*br + p*len_i)*bc, entry k -> column colidx[rowptr[i] + k/bc]*bc + k%bc.
__global__ void sell_width_kernel(const int32_t* __restrict__ rowptr, int64_t n_rows, int br, int bc, int64_t n_slices,
                                  int* __restrict__ w) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_slices; s += (int64_t)gridDim.x * blockDim.x) {
    int64_t r0 = s * SH, r1 = r0 + SH < n_rows ? r0 + SH : n_rows;
    int m = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t i = r / br;
      m = max(m, (rowptr[i + 1] - rowptr[i]) * bc);
    }
    w[s] = m;
  }
}

// block matrices: direct (strided) reads, one lane per scalar row -- a one-off per assembly
template <bool WITH_COLS>
__global__ void __launch_bounds__(256) sell_fill_block_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                              const double* __restrict__ val, int64_t n_rows, int br, int bc,
                                                              int64_t n_slices, const int64_t* __restrict__ sptr,
                                                              const int* __restrict__ sw, double* __restrict__ sval,
                                                              int32_t* __restrict__ scol) {
  const int lane = threadIdx.x & 63;
  for (int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; s < n_slices; s += ((int64_t)gridDim.x * blockDim.x) >> 6) {
    const int64_t row = s * SH + lane;
    int64_t off = 0;
    int len = 0, lo = 0;
    if (row < n_rows) {
      const int64_t i = row / br;
      const int p = (int)(row - i * br);
      lo = rowptr[i];
      const int ln = rowptr[i + 1] - lo;
      off = ((int64_t)lo * br + (int64_t)p * ln) * bc;
      len = ln * bc;
    }
    const int64_t base = sptr[s];
    const int wd = sw[s];
    for (int k = 0; k < wd; ++k) {
      sval[base + (int64_t)k * SH + lane] = k < len ? val[off + k] : 0.0;
      if (WITH_COLS) scol[base + (int64_t)k * SH + lane] = k < len ? colidx[lo + k / bc] * bc + k % bc : 0;
    }
  }
}

// block matrices through LDS: the 64 scalar rows of a slice are ONE contiguous chunk of the block-CSR values (rows (i, p)
// follow each other: (rowptr[i] br + p len_i) bc), read with coalesced loads by the whole workgroup and written back as
// 512-B k-columns.  (The strided variant above touches a different cache line per lane and load: 8x the traffic.)
template <bool WITH_COLS>
__global__ void __launch_bounds__(256) sell_fill_block_lds_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                                  const double* __restrict__ val, int64_t n_rows, int br, int bc,
                                                                  int64_t n_slices, const int64_t* __restrict__ sptr,
                                                                  const int* __restrict__ sw, double* __restrict__ sval,
                                                                  int32_t* __restrict__ scol) {
  extern __shared__ __align__(16) double lv[];   // [64 * maxw]
  __shared__ int roff[SH + 1];                   // chunk-relative first entry of every scalar row of the slice
  __shared__ int rlo[SH];                        // rowptr of the row's node (columns)
  __shared__ int64_t base0;
  const int tid = threadIdx.x;
  const int64_t n_nodes = n_rows / br;
  for (int64_t s = blockIdx.x; s < n_slices; s += gridDim.x) {
    const int64_t r0 = s * SH;
    auto row_off = [&](int64_t row) -> int64_t {
      if (row >= n_rows) return (int64_t)rowptr[n_nodes] * br * bc;
      const int64_t i = row / br;
      const int p = (int)(row - i * br);
      const int lo = rowptr[i];
      return ((int64_t)lo * br + (int64_t)p * (rowptr[i + 1] - lo)) * bc;
    };
    const int64_t b0 = row_off(r0);
    if (tid <= SH) {
      roff[tid] = (int)(row_off(r0 + tid) - b0);
      if (tid < SH) rlo[tid] = r0 + tid < n_rows ? rowptr[(r0 + tid) / br] : 0;
    }
    if (tid == 0) base0 = b0;
    __syncthreads();
    const int total = roff[SH];
    const double* __restrict__ src = val + base0;
    for (int e = tid; e < total; e += 256) lv[e] = src[e];
    __syncthreads();
    const int wd = sw[s];
    const int64_t ob = sptr[s];
    for (int idx = tid; idx < wd * SH; idx += 256) {
      const int k = idx >> 6, ln = idx & 63;
      const int st = roff[ln], len = roff[ln + 1] - st;
      sval[ob + idx] = k < len ? lv[st + k] : 0.0;
      if (WITH_COLS) scol[ob + idx] = k < len ? colidx[rlo[ln] + k / bc] * bc + k % bc : 0;
    }
    __syncthreads();
  }
}

// One WAVE per slice, independent waves (single-wave workgroups: 11 fit a CU's LDS; no workgroup barrier: a slice's staging area in LDS belongs to
// its wave, and the LDS executes a wave's instructions in order).  The slice's CSR chunk is contiguous: staged through LDS
// with coalesced loads -- all of a batch in flight before the first LDS write -- and written back as 512-B k-columns.  The
// row offsets of the 64 rows come from ONE coalesced pair of loads (lane = row), so a slice costs two dependent global
// latencies (offsets, values) instead of three.
template <bool WITH_COLS>
__global__ void __launch_bounds__(64) sell_fill_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                        const double* __restrict__ val, int64_t n_rows, int64_t n_slices,
                                                        const int64_t* __restrict__ sptr, const int* __restrict__ sw,
                                                        int maxw, double* __restrict__ sval, int32_t* __restrict__ scol) {
  extern __shared__ __align__(16) unsigned char sm[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t per_wave = (size_t)SH * maxw * (WITH_COLS ? 12 : 8);
  double* lv = reinterpret_cast<double*>(sm + wv * per_wave);
  int32_t* lc = reinterpret_cast<int32_t*>(lv + (size_t)SH * maxw);
  const int nwb = blockDim.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * nwb + wv, nw = (int64_t)gridDim.x * nwb;
  for (int64_t s = w0; s < n_slices; s += nw) {
    const int64_t row = s * SH + lane;
    const int a = rowptr[row < n_rows ? row : n_rows], b = rowptr[row + 1 < n_rows ? row + 1 : n_rows];
    const int lo0 = __builtin_amdgcn_readfirstlane(a);
    const int cnt = __builtin_amdgcn_readlane(b, 63) - lo0;
    const int lo = a - lo0, len = b - a;
    constexpr int U = 8;
    for (int i0 = 0; i0 < cnt; i0 += 64 * U) {
      double v[U];
      int32_t cc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + 64 * u + lane;
        v[u] = i < cnt ? val[lo0 + i] : 0.0;
        if (WITH_COLS) cc[u] = i < cnt ? colidx[lo0 + i] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + 64 * u + lane;
        if (i < cnt) {
          lv[i] = v[u];
          if (WITH_COLS) lc[i] = cc[u];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the LDS writes above are ordered before the reads below
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t base = sptr[s];
    const int wd = sw[s];
    for (int k = 0; k < wd; ++k) {
      sval[base + (int64_t)k * SH + lane] = k < len ? lv[lo + k] : 0.0;
      if (WITH_COLS) scol[base + (int64_t)k * SH + lane] = k < len ? lc[lo + k] : (row < n_rows ? (int32_t)row : 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // ... and these reads before the next slice's writes
    __builtin_amdgcn_wave_barrier();
  }
}

__device__ inline double wsum64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool DOT>
__global__ void __launch_bounds__(256) sell_spmv_kernel(const int64_t* __restrict__ sptr, const int* __restrict__ sw,
                                                        const int32_t* __restrict__ scol, const double* __restrict__ sval,
                                                        const double* __restrict__ x, double* __restrict__ y, int64_t n_rows,
                                                        int64_t n_slices, const int* __restrict__ flag, double* __restrict__ part, int64_t s_begin, int part_off, int64_t hole_begin, int64_t hole_len) {
  if (flag && flag[0]) return;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  double dot = 0.0;
  for (int64_t sq = s_begin + w0; sq < n_slices; sq += nw) {   // n_slices: logical end (hole removed)
    const int64_t s = sq >= hole_begin ? sq + hole_len : sq;
    const int64_t base = sptr[s] + lane;
    const int wd = sw[s];
    const double* __restrict__ v = sval + base;
    const int32_t* __restrict__ ci = scol + base;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int k = 0;
    for (; k + 4 <= wd; k += 4) {
      const double v0 = v[(k + 0) * SH], v1 = v[(k + 1) * SH], v2 = v[(k + 2) * SH], v3 = v[(k + 3) * SH];
      const int c0 = ci[(k + 0) * SH], c1 = ci[(k + 1) * SH], c2 = ci[(k + 2) * SH], c3 = ci[(k + 3) * SH];
      a0 = fma(v0, x[c0], a0);
      a1 = fma(v1, x[c1], a1);
      a2 = fma(v2, x[c2], a2);
      a3 = fma(v3, x[c3], a3);
    }
    for (; k < wd; ++k) a0 = fma(v[k * SH], x[ci[k * SH]], a0);
    const double acc = (a0 + a1) + (a2 + a3);
    const int64_t row = s * SH + lane;
    if (row < n_rows) {
      y[row] = acc;
      if (DOT) dot += acc * x[row];
    }
  }
  if (DOT) {
    __shared__ double smd[4];
    dot = wsum64(dot);
    if (lane == 0) smd[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) part[part_off + blockIdx.x] = smd[0] + smd[1] + smd[2] + smd[3];
  }
}


// ---- column-pattern dictionary ---------------------------------------------------------------
// On lattice-numbered meshes almost every row has one of a handful of relative column patterns
// (col - row for k = 0..len-1).  When the graph has <= PAT_MAX distinct patterns the SpMV reads a
// 4-byte pattern id per ROW instead of a 4-byte column index per ENTRY (12 -> ~8 B per nonzero);
// otherwise (unstructured numbering) the explicit column array is used.
__global__ void pat_hash_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int64_t n_rows,
                                unsigned long long* __restrict__ h) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int lo = rowptr[r], len = rowptr[r + 1] - lo;
    unsigned long long x = 1469598103934665603ull ^ (unsigned long long)len;
    for (int k = 0; k < len; ++k) {
      const long long off = (long long)colidx[lo + k] - (long long)r;
      x ^= (unsigned long long)off + 0x9e3779b97f4a7c15ull + (x << 6) + (x >> 2);
      x *= 1099511628211ull;
    }
    h[r] = x & ~(1ull << 63);  // keep clear of the all-ones pad value
  }
}

__global__ void pat_assign_kernel(const unsigned long long* __restrict__ h, int64_t n_rows,
                                  const unsigned long long* __restrict__ uniq, int nu, int32_t* __restrict__ pid,
                                  int32_t* __restrict__ rep) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long x = h[r];
    int l = 0, hgh = nu;
    while (l < hgh) {
      int m = (l + hgh) >> 1;
      if (uniq[m] < x)
        l = m + 1;
      else
        hgh = m;
    }
    pid[r] = l;
    rep[l] = (int32_t)r;  // any representative row (benign race)
  }
}

__global__ void pat_table_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                 const int32_t* __restrict__ rep, int nu, int32_t* __restrict__ tab, int32_t* __restrict__ tlen) {
  const int p = blockIdx.x;
  if (p >= nu) return;
  const int r = rep[p];
  const int lo = rowptr[r], len = rowptr[r + 1] - lo;
  if (threadIdx.x == 0) tlen[p] = len;
  for (int k = threadIdx.x; k < PAT_W; k += blockDim.x) tab[p * PAT_W + k] = k < len ? colidx[lo + k] - r : 0;
}

__global__ void pat_verify_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int64_t n_rows,
                                  const int32_t* __restrict__ pid, const int32_t* __restrict__ tab,
                                  const int32_t* __restrict__ tlen, int* __restrict__ bad) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int lo = rowptr[r], len = rowptr[r + 1] - lo;
    const int p = pid[r];
    bool ok = len == tlen[p];
    for (int k = 0; ok && k < len; ++k) ok = colidx[lo + k] == (int32_t)r + tab[p * PAT_W + k];
    if (!ok) *bad = 1;
  }
}

template <bool DOT>
__global__ void __launch_bounds__(256) sellp_spmv_kernel(const int64_t* __restrict__ sptr, const int* __restrict__ sw,
                                                         const int32_t* __restrict__ pid, const int32_t* __restrict__ tab,
                                                         int npat, const double* __restrict__ sval,
                                                         const double* __restrict__ x, double* __restrict__ y, int64_t n_rows,
                                                         int64_t n_slices, const int* __restrict__ flag,
                                                         double* __restrict__ part, int64_t s_begin, int part_off, int64_t hole_begin, int64_t hole_len) {
  extern __shared__ int32_t ltab[];  // [npat][PAT_W]
  __shared__ double smd[4];
  if (flag && flag[0]) return;
  // slot `npat` is an all-zero pattern for the padding lanes of the last slice (their values are
  // zero, but the gather must stay inside x: another pattern's negative offsets would not)
  for (int i = threadIdx.x; i < (npat + 1) * PAT_W; i += 256) ltab[i] = i < npat * PAT_W ? tab[i] : 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  double dot = 0.0;
  for (int64_t sq = s_begin + w0; sq < n_slices; sq += nw) {   // n_slices: logical end (hole removed)
    const int64_t s = sq >= hole_begin ? sq + hole_len : sq;
    const int64_t row = s * SH + lane;
    const int wd = sw[s];
    const double* __restrict__ v = sval + sptr[s] + lane;
    const int32_t* __restrict__ t = ltab + (row < n_rows ? pid[row] : npat) * PAT_W;
    const int64_t rb = row < n_rows ? row : 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int k = 0;
    for (; k + 4 <= wd; k += 4) {
      const double v0 = v[(k + 0) * SH], v1 = v[(k + 1) * SH], v2 = v[(k + 2) * SH], v3 = v[(k + 3) * SH];
      a0 = fma(v0, x[rb + t[k + 0]], a0);
      a1 = fma(v1, x[rb + t[k + 1]], a1);
      a2 = fma(v2, x[rb + t[k + 2]], a2);
      a3 = fma(v3, x[rb + t[k + 3]], a3);
    }
    for (; k < wd; ++k) a0 = fma(v[k * SH], x[rb + t[k]], a0);
    const double acc = (a0 + a1) + (a2 + a3);
    if (row < n_rows) {
      y[row] = acc;
      if (DOT) dot += acc * x[row];
    }
  }
  if (DOT) {
    dot = wsum64(dot);
    if (lane == 0) smd[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) part[part_off + blockIdx.x] = smd[0] + smd[1] + smd[2] + smd[3];
  }
}

// The same product straight from the CSR value array (no SELL image): one wave per 64 consecutive rows.  Their CSR entries are ONE
// contiguous run (<= 64 W doubles): it is read with fully coalesced loads (lane l takes the entries 64 j + l), parked in LDS, and
// every lane then walks its own row there (row offsets differ by the row length: odd for the 27-point stencil, i.e. free of bank
// conflicts).  The gathers of x depend only on the column pattern, not on the values: they are issued together with the value loads.
// Traffic = 8 B per stored entry (no slice padding) + 4 B pattern id + x, y per row.
// The matrix values of the lane-per-row kernels that stage a slice's run through LDS are read ONCE per product, in whole contiguous
// runs: non-temporal loads, so that they pass through L2 / the Infinity Cache without pushing out the x entries every row gathers
// (same-box A/B: 10 M-row CSR product 0.541 -> 0.522 ms, CG +3 %; 1024^2 second-order 2x2 blocks 0.548 -> 0.483-0.507 ms).  NOT in
// bcsr_spmv_kernel (several lanes per node row, three value rows per lane: 2.20 -> 2.65 ms with them) nor on the SELL images (+-0).
template <typename T_>
__device__ __forceinline__ T_ ld_stream(const T_* p) {
  return __builtin_nontemporal_load(p);
}

constexpr int CSRL_WAVES = 4;   // waves per workgroup (LDS: W x 512 B per wave): two workgroups = eight waves per CU measured best
template <int W, bool DOT>
__global__ void __launch_bounds__(64 * CSRL_WAVES) csrl_spmv_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ pid,
                                                                    const int32_t* __restrict__ tab, int npat, const double* __restrict__ val,
                                                                    const double* __restrict__ x, double* __restrict__ y, int64_t n_rows,
                                                                    int64_t n_slices, const int* __restrict__ flag, double* __restrict__ part,
                                                                    int64_t s_begin, int part_off, int64_t hole_begin, int64_t hole_len) {
  extern __shared__ double csrl_lds[];   // [CSRL_WAVES][64 W] values | [(npat + 1)][PAT_W] pattern table
  __shared__ double smd[CSRL_WAVES];
  if (flag && flag[0]) return;
  int32_t* ltab = reinterpret_cast<int32_t*>(csrl_lds + CSRL_WAVES * 64 * W);
  for (int i = threadIdx.x; i < (npat + 1) * PAT_W; i += 64 * CSRL_WAVES) ltab[i] = i < npat * PAT_W ? tab[i] : 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ buf = csrl_lds + wv * 64 * W;
  const int64_t w0 = (int64_t)blockIdx.x * CSRL_WAVES + wv;
  const int64_t nw = (int64_t)gridDim.x * CSRL_WAVES;
  double dot = 0.0;
  // row offsets one slice ahead: the value loads of a slice then start without a dependent load in front of them
  int nrp0 = 0, nrp1 = 0;
  {
    const int64_t sq = s_begin + w0;
    if (sq < n_slices) {
      const int64_t r = (sq >= hole_begin ? sq + hole_len : sq) * SH + lane;
      nrp0 = rowptr[r < n_rows ? r : n_rows];
      nrp1 = rowptr[r < n_rows ? r + 1 : n_rows];
    }
  }
  for (int64_t sq = s_begin + w0; sq < n_slices; sq += nw) {   // n_slices: logical end (hole removed)
    const int64_t s = sq >= hole_begin ? sq + hole_len : sq;
    const int64_t row = s * SH + lane;
    const bool live = row < n_rows;
    const int rp0 = nrp0, rp1 = nrp1;
    if (sq + nw < n_slices) {
      const int64_t r = ((sq + nw) >= hole_begin ? sq + nw + hole_len : sq + nw) * SH + lane;
      nrp0 = rowptr[r < n_rows ? r : n_rows];
      nrp1 = rowptr[r < n_rows ? r + 1 : n_rows];
    }
    const int base = __builtin_amdgcn_readfirstlane(rp0);
    const int total = __builtin_amdgcn_readlane(rp1, 63) - base;
    const int off = rp0 - base, len = rp1 - rp0;
    const double* __restrict__ v = val + base;
    // the run of the 64 rows, coalesced; zero beyond its end
    double vr[W];
#pragma unroll
    for (int j = 0; j < W; ++j) vr[j] = (64 * j + lane < total) ? ld_stream(v + 64 * j + lane) : 0.0;
    // the row's x entries (pattern table: column = row + t[k])
    const int32_t* __restrict__ t = ltab + (live ? pid[row] : npat) * PAT_W;
    const int64_t rb = live ? row : 0;
    double xg[W];
#pragma unroll
    for (int k = 0; k < W; ++k) xg[k] = x[rb + (k < len ? t[k] : 0)];
#pragma unroll
    for (int j = 0; j < W; ++j) buf[64 * j + lane] = vr[j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < W; k += 2) {
      a0 = fma(k < len ? buf[off + k] : 0.0, xg[k], a0);
      a1 = fma(k + 1 < len ? buf[off + k + 1] : 0.0, xg[k + 1], a1);
    }
    if (W & 1) a0 = fma(W - 1 < len ? buf[off + W - 1] : 0.0, xg[W - 1], a0);
    const double acc = a0 + a1;
    if (live) {
      y[row] = acc;
      if (DOT) dot += acc * x[row];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // every lane has read its row before the next run overwrites the buffer
  }
  if (DOT) {
    dot = wsum64(dot);
    if (lane == 0) smd[wv] = dot;
    __syncthreads();
    if (threadIdx.x == 0) {
      double sm = 0.0;
      for (int i = 0; i < CSRL_WAVES; ++i) sm += smd[i];
      part[part_off + blockIdx.x] = sm;
    }
  }
}

// The same for BLOCK matrices whose node rows follow the dictionary (2-D second-order elements: 25 / 15 / 9 column nodes, 2x2 blocks, i.e.
// 50 / 30 / 18 entries per scalar row): lane = scalar row (i, p), the 64 rows of a slice are one contiguous run of the block-CSR values
// ((rowptr[i] BR + p len_i) BC), read coalesced, parked in LDS, walked per lane; x entries from the node pattern: (i + t[k / BC]) BC + k % BC.
// No image (the SELL image of such a matrix pads every slice to its longest row: 20 % on alternating vertex / edge rows), no refresh.
constexpr int CSRLB_WAVES = 2;
template <int W, int BR, int BC, bool GL, bool DOT>
__global__ void __launch_bounds__(64 * CSRLB_WAVES) csrlb_spmv_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ pid,
                                                                      const int32_t* __restrict__ tab, int npat, const double* __restrict__ val,
                                                                      const double* __restrict__ x, double* __restrict__ y, int64_t n_rows,
                                                                      int64_t n_slices, const int* __restrict__ flag, double* __restrict__ part,
                                                                      int64_t s_begin, int part_off, int64_t hole_begin, int64_t hole_len) {
  extern __shared__ double csrl_lds[];   // [CSRLB_WAVES][64 W] values | [(npat + 1)][PAT_W] node pattern table
  __shared__ double smd[CSRLB_WAVES];
  if (flag && flag[0]) return;
  int32_t* ltab = reinterpret_cast<int32_t*>(csrl_lds + CSRLB_WAVES * 64 * W);
  for (int i = threadIdx.x; i < (npat + 1) * PAT_W; i += 64 * CSRLB_WAVES) ltab[i] = i < npat * PAT_W ? tab[i] : 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* __restrict__ buf = csrl_lds + wv * 64 * W;
  const int64_t w0 = (int64_t)blockIdx.x * CSRLB_WAVES + wv;
  const int64_t nw = (int64_t)gridDim.x * CSRLB_WAVES;
  const int64_t n_nodes = n_rows / BR;
  double dot = 0.0;
  for (int64_t sq = s_begin + w0; sq < n_slices; sq += nw) {   // n_slices: logical end (hole removed)
    const int64_t s = sq >= hole_begin ? sq + hole_len : sq;
    const int64_t row = s * SH + lane;
    const bool live = row < n_rows;
    const int64_t node = live ? row / BR : n_nodes;
    const int p = live ? (int)(row - node * BR) : 0;
    const int rp0 = rowptr[node], len = live ? rowptr[node + 1] - rp0 : 0;
    const int64_t off64 = ((int64_t)rp0 * BR + (int64_t)p * len) * BC;
    const int L1 = len * BC;
    // first entry of the slice and its length (lane 0 is always live; dead lanes sit at the end of the array)
    const int64_t base = ((int64_t)__builtin_amdgcn_readfirstlane((int)(off64 >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)(off64 & 0xffffffff));
    const int my = (int)(off64 - base);
    const int total = __builtin_amdgcn_readlane(my + L1, 63);
    const double* __restrict__ v = val + base;
    const int32_t* __restrict__ t = ltab + (live ? pid[node] : npat) * PAT_W;
    const int64_t nb = live ? node : 0;
    double xg[W];
    if (GL) {
      // long rows (W = 50): the run goes global -> LDS without passing through registers (LDS-DMA, 16 B per lane = 1 KiB per wave
      // instruction, destination = wave base + lane x 16: exactly the contiguous image wanted); an odd last entry by one plain load
#pragma unroll
      for (int j = 0; j < (W + 1) / 2; ++j) {
        const int e = 128 * j + 2 * lane;
        if (e + 1 < total)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(v + e),
                                           (__attribute__((address_space(3))) void*)(buf + 128 * j), 16, 0, 2);   // aux 2: nt
      }
      if (BC == 2 && W % 2 == 0) {   // the two x entries of a column node by one 16-byte load
#pragma unroll
        for (int kk = 0; kk < W / 2; ++kk) {
          const double2 xv = *reinterpret_cast<const double2*>(x + (nb + (2 * kk < L1 ? t[kk] : 0)) * 2);
          xg[2 * kk] = xv.x;
          xg[2 * kk + 1] = xv.y;
        }
      } else {
#pragma unroll
        for (int k = 0; k < W; ++k) xg[k] = x[(nb + (k < L1 ? t[k / BC] : 0)) * BC + (k < L1 ? k % BC : 0)];
      }
      if ((total & 1) && lane == 0) buf[total - 1] = v[total - 1];
      __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0): the DMA writes and the one plain LDS write have landed
    } else {
      double vr[W];
#pragma unroll
      for (int j = 0; j < W; ++j) vr[j] = (64 * j + lane < total) ? ld_stream(v + 64 * j + lane) : 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) xg[k] = x[(nb + (k < L1 ? t[k / BC] : 0)) * BC + (k < L1 ? k % BC : 0)];
#pragma unroll
      for (int j = 0; j < W; ++j) buf[64 * j + lane] = vr[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < W; k += 2) {
      a0 = fma(k < L1 ? buf[my + k] : 0.0, xg[k], a0);
      a1 = fma(k + 1 < L1 ? buf[my + k + 1] : 0.0, xg[k + 1], a1);
    }
    if (W & 1) a0 = fma(W - 1 < L1 ? buf[my + W - 1] : 0.0, xg[W - 1], a0);
    const double acc = a0 + a1;
    if (live) {
      y[row] = acc;
      if (DOT) dot += acc * x[row];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // every lane has read its row before the next run overwrites the buffer
  }
  if (DOT) {
    dot = wsum64(dot);
    if (lane == 0) smd[wv] = dot;
    __syncthreads();
    if (threadIdx.x == 0) {
      double sm = 0.0;
      for (int i = 0; i < CSRLB_WAVES; ++i) sm += smd[i];
      part[part_off + blockIdx.x] = sm;
    }
  }
}

// Block matrices: lane = scalar row (i,p); columns come from the NODE-level dictionary
// (col = (i + off[k / BC]) * BC + k % BC) or from the explicit expanded column array.
template <int BC, bool PAT, bool DOT>
__global__ void __launch_bounds__(256) sellb_spmv_kernel(const int64_t* __restrict__ sptr, const int* __restrict__ sw,
                                                         const int32_t* __restrict__ pid, const int32_t* __restrict__ tab,
                                                         int npat, const int32_t* __restrict__ scol,
                                                         const double* __restrict__ sval, const double* __restrict__ x,
                                                         double* __restrict__ y, int64_t n_rows, int br, int64_t n_slices,
                                                         const int* __restrict__ flag, double* __restrict__ part, int64_t s_begin, int part_off, int64_t hole_begin, int64_t hole_len) {
  extern __shared__ int32_t ltab[];  // [npat][PAT_W]
  __shared__ double smd[4];
  if (flag && flag[0]) return;
  if (PAT) {  // slot `npat` = all-zero pattern for padding lanes (see sellp_spmv_kernel)
    for (int i = threadIdx.x; i < (npat + 1) * PAT_W; i += 256) ltab[i] = i < npat * PAT_W ? tab[i] : 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  double dot = 0.0;
  for (int64_t sq = s_begin + w0; sq < n_slices; sq += nw) {   // n_slices: logical end (hole removed)
    const int64_t s = sq >= hole_begin ? sq + hole_len : sq;
    const int64_t row = s * SH + lane;
    const bool live = row < n_rows;
    const int64_t node = live ? row / br : 0;
    const int nk = sw[s] / BC;  // widths are multiples of BC
    const double* __restrict__ v = sval + sptr[s] + lane;
    const int32_t* __restrict__ ci = scol + (PAT ? 0 : sptr[s] + lane);
    const int32_t* __restrict__ t = ltab + (PAT ? (live ? pid[node] : npat) : 0) * PAT_W;
    double a0 = 0.0, a1 = 0.0;
    for (int kk = 0; kk < nk; ++kk) {
      const int64_t cb = PAT ? (node + t[kk]) * BC : 0;
#pragma unroll
      for (int q = 0; q < BC; ++q) {
        const int k = kk * BC + q;
        const int64_t col = PAT ? cb + q : (int64_t)ci[(int64_t)k * SH];
        if (q & 1)
          a1 = fma(v[(int64_t)k * SH], x[col], a1);
        else
          a0 = fma(v[(int64_t)k * SH], x[col], a0);
      }
    }
    const double acc = a0 + a1;
    if (live) {
      y[row] = acc;
      if (DOT) dot += acc * x[row];
    }
  }
  if (DOT) {
    dot = wsum64(dot);
    if (lane == 0) smd[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) part[part_off + blockIdx.x] = smd[0] + smd[1] + smd[2] + smd[3];
  }
}

// Block matrices (and scalar matrices with long rows) straight from the block-CSR values: G lanes per NODE row, 64 / G node rows per
// wave.  The br scalar rows of a node are one contiguous piece (rowptr[i] br + p len_i) bc of the value array: lane g of the group takes
// the entries r = g, g + G, ... of EVERY scalar row p (br coalesced loads per step), the x entry (col[r / BC] BC + r % BC) is gathered
// once per step and serves the br rows, a shuffle tree ends the row.  No image of the matrix, nothing to refresh after an assembly
// (the SELL image of a 128^3 3x3-block matrix cost 2.5 ms and 8.3 GB of traffic per assembly, and 8 % of padding in every product).
// Traffic = the block-CSR bytes: 8 B per value + 4 B per BLOCK of column index + x, y.
template <int BR, int BC, int U, bool DOT>
__global__ void __launch_bounds__(256) bcsr_spmv_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                        const double* __restrict__ val, const double* __restrict__ x, double* __restrict__ y,
                                                        int lg, int64_t n0, int64_t n1, int64_t hole_begin, int64_t hole_len,
                                                        const int* __restrict__ flag, double* __restrict__ part, int part_off,
                                                        const int32_t* __restrict__ rsel, const int32_t* __restrict__ cptr) {
  // rsel / cptr: COMPACT matrix (pyn_rhs.hip) -- logical row t is node row rsel[t], its values start at block cptr[t]
  __shared__ double smd[4];
  if (flag && flag[0]) return;
  // U entries per lane and trip: U column loads, U x gathers and U BR value loads in flight
  const int G = 1 << lg, npw = 64 >> lg;
  const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane >> lg;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
  double dot = 0.0;
  // row offsets one step ahead: a node's loads start without a dependent load in front of them
  int nlo = 0, nhi = 0, nvl = 0;
  int64_t ni = 0;
  {
    const int64_t tl = n0 + w0 * npw + sub;
    if (tl < n1) {
      const int64_t tq = tl >= hole_begin ? tl + hole_len : tl;
      ni = rsel ? rsel[tq] : tq;
      nlo = rowptr[ni];
      nhi = rowptr[ni + 1];
      nvl = rsel ? cptr[tq] : nlo;
    }
  }
  for (int64_t tb = n0 + w0 * npw; tb < n1; tb += nw * npw) {   // n1: logical end (hole removed)
    const int64_t tl = tb + sub;
    const bool live = tl < n1;
    const int64_t i = ni;
    const int lo = nlo, len = nhi - nlo, vlo = nvl;
    {
      const int64_t t2 = tl + nw * npw;
      nlo = nhi = nvl = 0;
      if (t2 < n1) {
        const int64_t tq = t2 >= hole_begin ? t2 + hole_len : t2;
        ni = rsel ? rsel[tq] : tq;
        nlo = rowptr[ni];
        nhi = rowptr[ni + 1];
        nvl = rsel ? cptr[tq] : nlo;
      }
    }
    const int L1 = len * BC;
    const double* __restrict__ v = val + (int64_t)vlo * (BR * BC);
    const int32_t* __restrict__ ci = colidx + lo;
    double acc[BR];
#pragma unroll
    for (int p = 0; p < BR; ++p) acc[p] = 0.0;
    int cn[U];   // column nodes of the next trip
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = g + u * G;
      cn[u] = r < L1 ? ci[r / BC] : 0;
    }
    for (int r0 = g; r0 < L1; r0 += U * G) {
      double a[U][BR], xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = r0 + u * G;
        const bool in = r < L1;
#pragma unroll
        for (int p = 0; p < BR; ++p) a[u][p] = in ? v[p * L1 + r] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = r0 + u * G;
        const int q = r % BC;
        xv[u] = r < L1 ? x[(int64_t)cn[u] * BC + q] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = r0 + (U + u) * G;
        cn[u] = r < L1 ? ci[r / BC] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int p = 0; p < BR; ++p) acc[p] = fma(a[u][p], xv[u], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < BR; ++p)
      for (int o = G >> 1; o > 0; o >>= 1) acc[p] += __shfl_xor(acc[p], o, 64);
    if (live && g == 0) {
#pragma unroll
      for (int p = 0; p < BR; ++p) {
        y[i * BR + p] = acc[p];
        if (DOT) dot = fma(acc[p], x[i * BC + p], dot);
      }
    }
  }
  if (DOT) {
    dot = wsum64(dot);
    if (lane == 0) smd[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) part[part_off + blockIdx.x] = smd[0] + smd[1] + smd[2] + smd[3];
  }
}

// Any block shape without dictionary, slices or image: LPR lanes per scalar row, rows of one node are contiguous in `val`
// y[(i,p)] = sum_k sum_q val[(rowptr[i]*br + p*len + k)*bc + q] * x[colidx[rowptr[i]+k]*bc + q]
template <int LPR, bool DOT>
__global__ void __launch_bounds__(256) spmv_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                   const double* __restrict__ val, const double* __restrict__ x,
                                                   double* __restrict__ y, int64_t n_rows, int br, int bc,
                                                   const int* __restrict__ flag, double* __restrict__ part) {
  if (flag && flag[0]) return;   // slot 0: the solver's done flag
  const int lane = threadIdx.x % LPR;
  const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPR;
  const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / LPR;
  double dot = 0.0;
  for (int64_t r = grp; r < n_rows; r += ngrp) {
    int64_t i = r / br;
    int p = (int)(r - i * br);
    int lo = rowptr[i];
    int len = rowptr[i + 1] - lo;
    const double* v = val + ((int64_t)lo * br + (int64_t)p * len) * bc;
    const int n = len * bc;
    double acc = 0.0;
    if (bc == 1) {
      for (int idx = lane; idx < n; idx += LPR) acc += v[idx] * x[colidx[lo + idx]];
    } else {
      for (int idx = lane; idx < n; idx += LPR) {
        int k = idx / bc, q = idx - k * bc;
        acc += v[idx] * x[(int64_t)colidx[lo + k] * bc + q];
      }
    }
    for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, LPR);
    if (lane == 0) {
      y[r] = acc;
      if (DOT) dot += acc * x[r];
    }
  }
  if (DOT) block_partial(dot, part);
}

}  // namespace

namespace {
// pattern id of a lattice row in closed form: per axis the class of the coordinate (ngl 2: first / inner / last; ngl 3: even-first /
// even-inner / even-last / odd), id = (cls_z ncls + cls_y) ncls + cls_x
__device__ __forceinline__ int lat_axis_class(int ngl, int c, int N) {
  if (ngl == 2) return c == 0 ? 0 : (c == N - 1 ? 2 : 1);
  if (c & 1) return 3;
  return c == 0 ? 0 : (c == N - 1 ? 2 : 1);
}
__global__ void pat_lattice_pid_kernel(int ngl, int dim, int NX, int NY, int NZ, int64_t n_rows, int32_t* __restrict__ pid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const int ncls = ngl == 2 ? 3 : 4;
  const int x = (int)(i % NX), y = (int)((i / NX) % NY), z = (int)(i / ((int64_t)NX * NY));
  int id = lat_axis_class(ngl, y, NY) * ncls + lat_axis_class(ngl, x, NX);
  if (dim == 3) id += lat_axis_class(ngl, z, NZ) * ncls * ncls;
  pid[i] = id;
}
// every `stride`-th row (and the last one) against its pattern
__global__ void pat_verify_sample_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int64_t n_rows, int64_t stride,
                                         const int32_t* __restrict__ pid, const int32_t* __restrict__ tab, const int32_t* __restrict__ tlen,
                                         int* __restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t r = t * stride;
  if (r >= n_rows) {
    if (r - stride >= n_rows || t == 0) return;
    r = n_rows - 1;      // the thread just past the end takes the last row
  }
  const int lo = rowptr[r], len = rowptr[r + 1] - lo;
  const int p = pid[r];
  bool ok = len == tlen[p];
  for (int k = 0; ok && k < len; ++k) ok = colidx[lo + k] == (int32_t)r + tab[p * PAT_W + k];
  if (!ok) *bad = 1;
}
}  // namespace

// The dictionary of a single-rank lattice in closed form (no hash / sort / full verification passes over the graph: 20 + 8 GB of set-up
// reads at 10 M rows): first-order hexahedra (27 patterns), first-order quadrilaterals (9), second-order quadrilaterals (16); a sample of
// rows is checked against the graph.  Slabs of a rank and every other numbering keep the hash-based construction below.
static int lattice_pattern_dictionary(pyn_ctx* c, bool* done) {
  *done = false;
  if (getenv("PYNAMA_NO_LATTICE_PATTERNS")) return PYN_OK;
  const BoxLattice& B = c->box;
  if (!(c->lat.valid || c->ho3.valid) || (B.ngl == 3 && B.dim == 3) || c->n_ghost != 0 || !B.natural()) return PYN_OK;
  const int ngl = B.ngl, dim = B.dim, NX = B.NX, NY = B.ny(), NZ = B.nz();
  const int ncls = ngl == 2 ? 3 : 4;
  const int npat = dim == 3 ? ncls * ncls * ncls : ncls * ncls;
  // offsets of one axis per class
  auto axis_offs = [&](int cls, int* out) {
    int lo, hi;
    if (ngl == 2) {
      lo = cls == 0 ? 0 : -1;
      hi = cls == 2 ? 0 : 1;
    } else if (cls == 3) {
      lo = -1;
      hi = 1;
    } else {
      lo = cls == 0 ? 0 : -2;
      hi = cls == 2 ? 0 : 2;
    }
    int n = 0;
    for (int d = lo; d <= hi; ++d) out[n++] = d;
    return n;
  };
  std::vector<int32_t> tab((size_t)PAT_MAX * PAT_W, 0), tlen((size_t)PAT_MAX, 0);
  for (int p = 0; p < npat; ++p) {
    const int cx = p % ncls, cy = (p / ncls) % ncls, cz = p / (ncls * ncls);
    int ox[5], oy[5], oz[5] = {0, 0, 0, 0, 0};
    const int nxo = axis_offs(cx, ox), nyo = axis_offs(cy, oy), nzo = dim == 3 ? axis_offs(cz, oz) : 1;
    int k = 0;
    if (nxo * nyo * nzo > PAT_W) return PYN_OK;
    for (int iz = 0; iz < nzo; ++iz)
      for (int iy = 0; iy < nyo; ++iy)
        for (int ix = 0; ix < nxo; ++ix) tab[(size_t)p * PAT_W + k++] = (int32_t)((int64_t)oz[iz] * NX * NY + (int64_t)oy[iy] * NX + ox[ix]);
    tlen[p] = k;
  }
  hipStream_t s = c->stream;
  const int64_t n = c->n_owned;
  DevBuf<int32_t> pid, ptab;   // installed only when the closed form describes the graph
  PYN_HIP(pid.alloc(n));
  PYN_HIP(ptab.alloc((size_t)PAT_MAX * PAT_W));
  DevTmp t_len, t_bad;
  PYN_HIP(t_len.alloc(PAT_MAX * sizeof(int32_t)));
  PYN_HIP(t_bad.alloc(sizeof(int)));
  PYN_HIP(hipMemsetAsync(t_bad.get(), 0, sizeof(int), s));
  PYN_HIP(hipMemcpyAsync(ptab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  PYN_HIP(hipMemcpyAsync(t_len.get(), tlen.data(), tlen.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  pat_lattice_pid_kernel<<<(int)((n + 255) / 256), 256, 0, s>>>(ngl, dim, NX, NY, NZ, n, pid);
  const int64_t stride = std::max<int64_t>(1, n / 65521);      // (a prime-ish count: the sample walks through every class)
  const int64_t ns = (n + stride - 1) / stride + 1;
  pat_verify_sample_kernel<<<(int)((ns + 255) / 256), 256, 0, s>>>(c->d_rowptr, c->d_colidx, n, stride, pid, ptab,
                                                                  t_len.as<int32_t>(), t_bad.as<int>());
  int hbad = 0;
  PYN_HIP(hipMemcpyAsync(&hbad, t_bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  if (hbad) return PYN_OK;   // not the graph this closed form describes: let the general construction decide
  c->sell_pid = std::move(pid);
  c->sell_tab = std::move(ptab);
  c->sell_npat = npat;
  *done = true;
  return PYN_OK;
}

static int build_pattern_dictionary(pyn_ctx* c, int maxw) {
  c->sell_npat = 0;
  if (maxw > PAT_W || getenv("PYNAMA_NO_PATTERNS")) return PYN_OK;
  {
    bool done = false;
    PYN_TRY(lattice_pattern_dictionary(c, &done));
    if (done) return PYN_OK;
  }
  hipStream_t s = c->stream;
  const int64_t n = c->n_owned;
  DevTmp t_h, t_hs, t_hu, t_nu, t_tmp, t_rep, t_len, t_bad;  // scratch, released on every exit path
  PYN_HIP(t_h.alloc(n * sizeof(unsigned long long)));
  PYN_HIP(t_hs.alloc(n * sizeof(unsigned long long)));
  PYN_HIP(t_hu.alloc(n * sizeof(unsigned long long)));
  PYN_HIP(t_nu.alloc(sizeof(int64_t)));
  unsigned long long *h = t_h.as<unsigned long long>(), *hs = t_hs.as<unsigned long long>(), *hu = t_hu.as<unsigned long long>();
  int64_t* d_nu = t_nu.as<int64_t>();
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 16384);
  pat_hash_kernel<<<grid, 256, 0, s>>>(c->d_rowptr, c->d_colidx, n, h);
  size_t tb = 0;
  PYN_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, h, hs, n, 0, 64, s));
  PYN_HIP(t_tmp.alloc(tb));
  PYN_HIP(hipcub::DeviceRadixSort::SortKeys(t_tmp.get(), tb, h, hs, n, 0, 64, s));
  tb = 0;
  PYN_HIP(hipcub::DeviceSelect::Unique(nullptr, tb, hs, hu, d_nu, n, s));
  PYN_HIP(hipStreamSynchronize(s));
  PYN_HIP(t_tmp.alloc(tb));
  PYN_HIP(hipcub::DeviceSelect::Unique(t_tmp.get(), tb, hs, hu, d_nu, n, s));
  int64_t nu = 0;
  PYN_HIP(hipMemcpyAsync(&nu, d_nu, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  if (nu < 1 || nu > PAT_MAX) return PYN_OK;  // irregular numbering: explicit columns
  DevBuf<int32_t> pid, ptab;   // installed only when every row matches its pattern
  PYN_HIP(pid.alloc(n));
  PYN_HIP(ptab.alloc((size_t)PAT_MAX * PAT_W));
  PYN_HIP(t_rep.alloc(PAT_MAX * sizeof(int32_t)));
  PYN_HIP(t_len.alloc(PAT_MAX * sizeof(int32_t)));
  PYN_HIP(t_bad.alloc(sizeof(int)));
  PYN_HIP(hipMemsetAsync(t_bad.get(), 0, sizeof(int), s));
  PYN_HIP(hipMemsetAsync(ptab, 0, (size_t)PAT_MAX * PAT_W * sizeof(int32_t), s));
  pat_assign_kernel<<<grid, 256, 0, s>>>(h, n, hu, (int)nu, pid, t_rep.as<int32_t>());
  pat_table_kernel<<<(int)nu, 64, 0, s>>>(c->d_rowptr, c->d_colidx, t_rep.as<int32_t>(), (int)nu, ptab, t_len.as<int32_t>());
  pat_verify_kernel<<<grid, 256, 0, s>>>(c->d_rowptr, c->d_colidx, n, pid, ptab, t_len.as<int32_t>(), t_bad.as<int>());
  int hbad = 0;
  PYN_HIP(hipMemcpyAsync(&hbad, t_bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  if (hbad != 0) return PYN_OK;  // a hash collision shows up here: fall back to explicit columns
  c->sell_pid = std::move(pid);
  c->sell_tab = std::move(ptab);
  c->sell_npat = (int)nu;
  return PYN_OK;
}

// slice s needs ghost entries of x iff one of its nodes has a column >= n_owned (rows are sorted: the last one)
__global__ void slice_ghost_flag_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int64_t n_owned,
                                        int br, int64_t ns, int* __restrict__ flags) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r0 = s * SH, r1 = std::min<int64_t>(r0 + SH, n_owned * br) - 1;
    int f = 0;
    for (int64_t i = r0 / br; i <= r1 / br; ++i) f |= colidx[rowptr[i + 1] - 1] >= n_owned;
    flags[s] = f;
  }
}

// ---- the choice ---------------------------------------------------------------------------------------------------------------------
// Every rule that picks a family and its launch shape is in product_choose: a host function of a few facts about the matrix and of
// the knobs, without a HIP call (exported as pyn_product_choose, so it is tested without a device).
struct ProductFacts {
  int br, bc, npat, maxw;    // block shape, patterns of the node dictionary (0: none), longest scalar row
  int64_t nnzb, n_owned;
  bool rhs_compact, solver, image;   // solver: the product will be repeated; image: a SELL image of the current values exists
};
struct ProductKnobs {   // the environment, read once per resolve; an integer knob that is not set is -1
  bool sell_image, block_sell, no_csrlb, no_sell;
  double bcsr_min_avg;
  int bcsr_lanes, bcsr_unroll, bcsr_wgs, csrlb_wgs, csr_wgs, max_grid;
};
static int env_int(const char* name) {
  const char* e = getenv(name);
  return e ? std::max(0, atoi(e)) : -1;
}
static ProductKnobs read_knobs() {
  const char* avg = getenv("PYNAMA_BCSR_MIN_AVG");
  return {getenv("PYNAMA_SELL_IMAGE") != nullptr, getenv("PYNAMA_BLOCK_SELL") != nullptr, getenv("PYNAMA_NO_CSRLB") != nullptr,
          getenv("PYNAMA_NO_SELL") != nullptr, avg ? atof(avg) : 128.0, env_int("PYNAMA_BCSR_LANES"), env_int("PYNAMA_BCSR_UNROLL"),
          env_int("PYNAMA_BCSR_WGS_PER_CU"), env_int("PYNAMA_CSRLB_WGS_PER_CU"), env_int("PYNAMA_CSR_SPMV_WGS_PER_CU"),
          env_int("PYNAMA_SPMV_MAX_GRID")};   // (the last one, tests: persistent loops turn at small sizes)
}

static bool sell_shape(int bc) { return bc == 1 || bc == 2 || bc == 3 || bc == 6; }
static bool bcsr_shape(int br, int bc) {
  return (br == bc && (br == 1 || br == 2 || br == 3)) || (bc == 1 && (br == 2 || br == 3)) || (br == 1 && (bc == 2 || bc == 3)) ||
         (br == 3 && bc == 2) || (br == 2 && bc == 3) || (br == 6 && bc == 3) || (br == 3 && bc == 6);
}
// the 32-lane kernel needs neither dictionary nor slices: decided from the block shape and PYNAMA_NO_SELL alone
static bool raw_only(const ProductFacts& f, const ProductKnobs& k) { return !f.rhs_compact && (k.no_sell || !sell_shape(f.bc)); }

// kind (PK_NONE: no product for this block shape), W, lg and unroll of the plan; *keep_image false: never an image, every product of
// the matrix reads A.val
static ProductPlan product_choose(const ProductFacts& f, const ProductKnobs& k, bool* keep_image) {
  auto pick = [&](ProductPlan p, bool keep) { *keep_image = keep; return p; };   // p: {kind, W, lg, unroll}
  const double avg = (double)f.nnzb * f.bc / (double)std::max<int64_t>(1, f.n_owned);   // entries per scalar row
  auto bcsr = [&](bool keep) {
    // measured (tools/block_spmv_case.py): 16 lanes for 81 .. 375 entries per scalar row, 8 below; 32 / 64 lanes lose 5-10 % even on
    // the longest rows (fewer node rows, i.e. fewer independent load streams, per wave)
    const int g = k.bcsr_lanes, lg = g >= 0 ? (g >= 64 ? 6 : g >= 32 ? 5 : g >= 16 ? 4 : 3) : (avg >= 56.0 ? 4 : 3);
    const int u = k.bcsr_unroll >= 0 ? k.bcsr_unroll : (avg >= 24.0 ? 8 : 4);   // whole rows in one trip where the registers allow
    return pick({PK_BCSR, 0, lg, (u == 2 || u == 3 || u == 8) ? u : 4}, keep);
  };
  const bool scalar = f.br == 1 && f.bc == 1;
  if (f.rhs_compact) return bcsr_shape(f.br, f.bc) ? bcsr(true) : pick({}, true);   // stored rows only, from their block-CSR values
  if (raw_only(f, k)) return pick({PK_RAW}, true);
  // Scalar matrices whose rows follow the dictionary (at most PAT_W entries) are multiplied straight from their CSR values: no SELL
  // image, no refresh after an assembly.  PYNAMA_SELL_IMAGE=1 keeps the image-based kernel.
  if (scalar && f.npat > 0 && f.maxw <= PAT_W && !k.sell_image) return pick({PK_CSRL, f.maxw <= 27 ? 27 : 32}, false);
  // 2x2 blocks in dictionary mode: lane per scalar row over LDS-staged runs of the block-CSR values
  if (f.br == 2 && f.bc == 2 && f.npat > 0 && f.maxw <= 50 && !k.block_sell && !k.no_csrlb)
    return pick({PK_CSRLB, f.maxw <= 18 ? 18 : (f.maxw <= 32 ? 32 : 50)}, false);
  // Block matrices, and scalar matrices whose rows are too long for the dictionary (second-order elements: up to 125 entries), are
  // multiplied from the block-CSR values as well.  1: every product of A (long rows: the SELL image would carry 20 % of padding and
  // cost a refresh per assembly); 2: only one-off products (pyn_spmv of a matrix without a current image: Krhs v, Rw w, the operators
  // -- a refresh costs three products), solvers build the image, whose lane-per-row kernel is 20-25 % faster on the short rows of
  // first-order elements; 0: never (PYNAMA_BLOCK_SELL=1: A/B, tests).  Scalar rows inside the dictionary's width keep their kernels.
  int bm = (k.block_sell || !bcsr_shape(f.br, f.bc)) ? 0 : (avg >= k.bcsr_min_avg ? 1 : 2);
  if (scalar && !(f.maxw > PAT_W && !k.sell_image)) bm = 0;
  if (bm == 1) return bcsr(false);
  if (bm == 2 && !f.solver && !f.image) return bcsr(true);
  return pick({scalar ? (f.npat > 0 ? PK_SELLP : PK_SELL) : (f.npat > 0 ? PK_SELLB_D : PK_SELLB_X)}, true);
}

extern "C" int pyn_product_choose(int br, int bc, int npat, int maxw, int64_t nnzb, int64_t n_owned, int rhs_compact, int solver,
                                  int image, int sell_image, int block_sell, int no_csrlb, int no_sell, double bcsr_min_avg,
                                  int bcsr_lanes, int bcsr_unroll, int* kind, int* W, int* lanes, int* unroll) {
  PYN_CHECK(kind && W && lanes && unroll, "pyn_product_choose: NULL output");
  PYN_CHECK(br > 0 && bc > 0 && npat >= 0 && maxw >= 0 && nnzb >= 0 && n_owned >= 0, "pyn_product_choose: bad argument");
  const ProductKnobs k{sell_image != 0, block_sell != 0, no_csrlb != 0, no_sell != 0, bcsr_min_avg >= 0.0 ? bcsr_min_avg : 128.0,
                       std::max(-1, bcsr_lanes), std::max(-1, bcsr_unroll), -1, -1, -1, -1};
  bool keep_image;
  const ProductPlan ch = product_choose({br, bc, npat, maxw, nnzb, n_owned, rhs_compact != 0, solver != 0, image != 0}, k, &keep_image);
  *kind = ch.kind;
  *W = ch.W;
  *lanes = ch.kind == PK_BCSR ? 1 << ch.lg : 0;
  *unroll = ch.unroll;
  return PYN_OK;
}

// ---- shared structure ---------------------------------------------------------------------------------------------------------------
// The node-level dictionary once per graph, and per block shape the slice pointers and widths (the explicit columns come with the first
// image that needs them) and the interior slice range.
static int sell_structure(pyn_ctx* c, const DMat& A, SellShape** out) {
  hipStream_t s = c->stream;
  const int64_t n = c->n_owned * A.br;  // scalar rows
  const int64_t ns = (n + SH - 1) / SH;
  if (!c->sell_dict_built) {
    std::vector<int32_t> rp((size_t)c->n_owned + 1);
    PYN_HIP(hipMemcpyAsync(rp.data(), c->d_rowptr, (c->n_owned + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PYN_HIP(hipStreamSynchronize(s));
    int maxlen = 0;
    for (int64_t i = 0; i < c->n_owned; ++i) maxlen = std::max(maxlen, rp[i + 1] - rp[i]);
    PYN_TRY(build_pattern_dictionary(c, maxlen));
    c->sell_dict_built = true;
  }
  *out = const_cast<SellShape*>(pyn_sell_shape(c, A));
  if (*out) return PYN_OK;
  SellShape q;
  q.br = A.br;
  q.bc = A.bc;
  q.ns = ns;
  PYN_HIP(q.w.alloc(ns));
  sell_width_kernel<<<(int)std::min<int64_t>((ns + 255) / 256, 4096), 256, 0, s>>>(c->d_rowptr, n, A.br, A.bc, ns, q.w);
  std::vector<int> w((size_t)ns);
  PYN_HIP(hipMemcpyAsync(w.data(), q.w, ns * sizeof(int), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  std::vector<int64_t> ptr((size_t)ns + 1);
  ptr[0] = 0;
  for (int64_t i = 0; i < ns; ++i) {
    ptr[i + 1] = ptr[i] + (int64_t)w[i] * SH;
    q.maxw = std::max(q.maxw, w[i]);
  }
  q.total = ptr[ns];
  PYN_HIP(q.ptr.alloc(ns + 1));
  PYN_HIP(hipMemcpyAsync(q.ptr, ptr.data(), (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  PYN_HIP(hipStreamSynchronize(s));
  if (c->n_ghost > 0) {
    // interior slices (no ghost columns) can be multiplied while the halo exchange is in flight: usable when
    // they form ONE contiguous range (z-slabs: everything between the first and the last node plane)
    DevTmp tf;
    PYN_HIP(tf.alloc(ns * sizeof(int)));
    slice_ghost_flag_kernel<<<(int)std::min<int64_t>((ns + 255) / 256, 4096), 256, 0, s>>>(c->d_rowptr, c->d_colidx, c->n_owned, A.br,
                                                                                       ns, tf.as<int>());
    std::vector<int> fl((size_t)ns);
    PYN_HIP(hipMemcpyAsync(fl.data(), tf.get(), ns * sizeof(int), hipMemcpyDeviceToHost, s));
    PYN_HIP(hipStreamSynchronize(s));
    int64_t i0 = 0, i1 = ns;
    while (i0 < ns && fl[i0]) ++i0;
    while (i1 > i0 && fl[i1 - 1]) --i1;
    bool contiguous = i1 > i0;
    for (int64_t i = i0; i < i1 && contiguous; ++i) contiguous = !fl[i];
    if (contiguous) {
      q.int_begin = i0;
      q.int_end = i1;
    }
  }
  c->sell_shapes.push_back(std::move(q));
  *out = &c->sell_shapes.back();
  return PYN_OK;
}

// the SELL image of A holds the current values (the structure is shared by all matrices of the block shape)
static int sell_image(pyn_ctx* c, DMat& A, SellShape* S, bool fresh) {
  hipStream_t s = c->stream;
  const int64_t n = c->n_owned * A.br, ns = S->ns;
  if (!A.sell_val) {
    PYN_HIP(A.sell_val.alloc(S->total));
    A.sell_valid = false;
  }
  const bool cols = c->sell_npat == 0 && !S->col;   // this image also writes the shape's explicit column array
  if (cols) PYN_HIP(S->col.alloc(S->total));
  if (A.sell_valid && !fresh && !cols) return PYN_OK;
  if (A.br == 1 && A.bc == 1 && (size_t)SH * S->maxw * 12 <= 64 * 1024) {
    const size_t lds = (size_t)SH * S->maxw * (cols ? 12 : 8);
    const int grid = (int)std::min<int64_t>(ns, 256 * 32);
    auto fill = cols ? sell_fill_kernel<true> : sell_fill_kernel<false>;
    fill<<<grid, 64, lds, s>>>(c->d_rowptr, c->d_colidx, A.val, n, ns, S->ptr, S->w, S->maxw, A.sell_val, cols ? S->col.get() : nullptr);
  } else if ((size_t)SH * S->maxw * sizeof(double) <= 96 * 1024 && !getenv("PYNAMA_SELL_FILL_STRIDED")) {
    const size_t lds = (size_t)SH * S->maxw * sizeof(double);
    const int grid = (int)std::min<int64_t>(ns, 256 * 8);
    PYN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sell_fill_block_lds_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PYN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sell_fill_block_lds_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto fill = cols ? sell_fill_block_lds_kernel<true> : sell_fill_block_lds_kernel<false>;
    fill<<<grid, 256, lds, s>>>(c->d_rowptr, c->d_colidx, A.val, n, A.br, A.bc, ns, S->ptr, S->w, A.sell_val, cols ? S->col.get() : nullptr);
  } else {
    const int grid = (int)std::min<int64_t>((ns + 3) / 4, 256 * 16);
    auto fill = cols ? sell_fill_block_kernel<true> : sell_fill_block_kernel<false>;
    fill<<<grid, 256, 0, s>>>(c->d_rowptr, c->d_colidx, A.val, n, A.br, A.bc, ns, S->ptr, S->w, A.sell_val, cols ? S->col.get() : nullptr);
  }
  PYN_HIP(hipGetLastError());
  A.sell_valid = true;
  return PYN_OK;
}

// ---- resolve: facts -> choice -> A.plan (and the image, where the choice is an image kernel) ----------------------------------------
int pyn_sell_ensure(pyn_ctx* c, DMat& A, bool solver) {
  const ProductKnobs k = read_knobs();
  ProductFacts f{A.br, A.bc, 0, 0, c->nnzb, c->n_owned, A.rhs_compact, solver, A.sell_val && A.sell_valid};
  SellShape* S = nullptr;
  const size_t shapes = c->sell_shapes.size();
  if (!raw_only(f, k)) {
    PYN_CHECK(sell_shape(A.bc), "no SELL kernel for block shape %dx%d", A.br, A.bc);
    PYN_TRY(sell_structure(c, A, &S));
    f.npat = c->sell_npat;
    f.maxw = S->maxw;
  }
  bool keep_image;
  ProductPlan P = product_choose(f, k, &keep_image);
  PYN_CHECK(P.kind != PK_NONE, "no block-CSR product for block shape %dx%d", A.br, A.bc);
  if (!keep_image) {   // the products read A.val
    A.sell_val.reset();
    A.sell_valid = false;
  }
  if (P.kind >= PK_SELL && P.kind <= PK_SELLB_D) PYN_TRY(sell_image(c, A, S, c->sell_shapes.size() != shapes));
  // what the launches need beyond the choice: LDS (staged runs, dictionary), the resident-workgroup cap, the grid clamp
  const int waves = P.kind == PK_CSRL ? CSRL_WAVES : (P.kind == PK_CSRLB ? CSRLB_WAVES : 0);
  if (waves || P.kind == PK_SELLP || P.kind == PK_SELLB_D)
    P.lds = (size_t)waves * 64 * P.W * sizeof(double) + (size_t)(c->sell_npat + 1) * PAT_W * sizeof(int32_t);
  // csrl: persistent waves, exactly the workgroups that are resident together (LDS: 160 KB per CU; 160-190 VGPRs: three / two waves per
  // SIMD), so that every wave walks the same number of slices -- a grid of 1.6 x that capacity runs 20 % longer
  const int csrl_per_cu = std::max(1, std::min((int)(163840 / (P.lds + 64)), 8 / CSRL_WAVES));   // eight waves per CU (ten: +3 %, twelve: +12 %)
  const int wgs = P.kind == PK_CSRL ? (k.csr_wgs >= 0 ? k.csr_wgs : csrl_per_cu)
                                    : (P.kind == PK_CSRLB ? k.csrlb_wgs : (P.kind == PK_BCSR ? k.bcsr_wgs : -1));
  if (wgs >= 0) P.wg_cap = 256 * wgs;   // else: what the occupancy query of the kernel says (csrlb, bcsr)
  if (k.max_grid >= 0) P.max_grid = std::max(1, k.max_grid);
  A.plan = P;
  return PYN_OK;
}

const SellShape* pyn_sell_shape(pyn_ctx* c, const DMat& A) {
  for (auto& q : c->sell_shapes)
    if (q.br == A.br && q.bc == A.bc) return &q;
  return nullptr;
}

// ---- launchers: one per family ------------------------------------------------------------------------------------------------------
namespace {
struct Launch {   // one product launch: the logical range [s0, s1) with the hole [hb, hb + hl) cut out -- slices; PK_BCSR: node rows
  pyn_ctx* c;
  const DMat& A;
  const SellShape* S;
  const ProductPlan& P;
  const double* x;
  double* y;
  const int* flag;   // fused dot: the solver's done flag and the partials (c->d_flag, c->d_part), else null
  double* part;
  int64_t s0, s1, hb, hl;
  int poff, max_grid;
  hipStream_t st;
};

// persistent waves: at most the workgroups that are resident together (a grid of 1.6 x that capacity runs a second, half-empty round)
int persistent_grid(const Launch& L, int64_t want, int resident) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, L.max_grid), L.P.wg_cap >= 0 ? L.P.wg_cap : resident));
}

template <bool DOT>
int launch_raw(const Launch& L, int* grid) {
  const int64_t rows = L.c->n_owned * L.A.br;
  *grid = pyn_raw_grid(rows);
  spmv_kernel<32, DOT><<<*grid, 256, 0, L.st>>>(L.c->d_rowptr, L.c->d_colidx, L.A.val, L.x, L.y, rows, L.A.br, L.A.bc, L.flag, L.part);
  return PYN_OK;
}

template <bool DOT>
int launch_sell(const Launch& L, int grid) {   // scalar image
  pyn_ctx* c = L.c;
  const SellShape& S = *L.S;
  if (L.P.kind == PK_SELLP)
    sellp_spmv_kernel<DOT><<<grid, 256, L.P.lds, L.st>>>(S.ptr, S.w, c->sell_pid, c->sell_tab, c->sell_npat, L.A.sell_val, L.x, L.y, c->n_owned,
                                                         L.s1, L.flag, L.part, L.s0, L.poff, L.hb, L.hl);
  else
    sell_spmv_kernel<DOT><<<grid, 256, 0, L.st>>>(S.ptr, S.w, S.col, L.A.sell_val, L.x, L.y, c->n_owned, L.s1, L.flag, L.part, L.s0, L.poff, L.hb,
                                                  L.hl);
  return PYN_OK;
}

template <int BC, bool DOT>
int launch_sellb(const Launch& L, int grid) {   // block image
  pyn_ctx* c = L.c;
  const SellShape& S = *L.S;
  const int64_t n = c->n_owned * L.A.br;
  if (L.P.kind == PK_SELLB_D)
    sellb_spmv_kernel<BC, true, DOT><<<grid, 256, L.P.lds, L.st>>>(S.ptr, S.w, c->sell_pid, c->sell_tab, c->sell_npat, nullptr, L.A.sell_val, L.x,
                                                                   L.y, n, L.A.br, L.s1, L.flag, L.part, L.s0, L.poff, L.hb, L.hl);
  else
    sellb_spmv_kernel<BC, false, DOT><<<grid, 256, 0, L.st>>>(S.ptr, S.w, nullptr, nullptr, 0, S.col, L.A.sell_val, L.x, L.y, n, L.A.br, L.s1,
                                                              L.flag, L.part, L.s0, L.poff, L.hb, L.hl);
  return PYN_OK;
}

template <int W, bool DOT>
int launch_csrl(const Launch& L, int* grid) {
  static bool attr = false;
  if (!attr) {
    PYN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(csrl_spmv_kernel<W, DOT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(CSRL_WAVES * 64 * W * sizeof(double) + (PAT_MAX + 1) * PAT_W * sizeof(int32_t))));
    attr = true;
  }
  pyn_ctx* c = L.c;
  *grid = persistent_grid(L, (L.s1 - L.s0 + CSRL_WAVES - 1) / CSRL_WAVES, 0);   // (the plan always carries the cap of this family)
  PYN_CHECK(L.poff + *grid <= PYN_MAX_PARTIALS, "partial buffer overflow");
  csrl_spmv_kernel<W, DOT><<<*grid, 64 * CSRL_WAVES, L.P.lds, L.st>>>(c->d_rowptr, c->sell_pid, c->sell_tab, c->sell_npat, L.A.val, L.x, L.y,
                                                                      c->n_owned, L.s1, L.flag, L.part, L.s0, L.poff, L.hb, L.hl);
  return PYN_OK;
}

template <int W, bool DOT>
int launch_csrlb(const Launch& L, int* grid) {
  constexpr bool GL = W > 32;
  static int per_cu = 0;
  if (!per_cu) {
    PYN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(csrlb_spmv_kernel<W, 2, 2, GL, DOT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(CSRLB_WAVES * 64 * W * sizeof(double) + (PAT_MAX + 1) * PAT_W * sizeof(int32_t))));
    PYN_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, csrlb_spmv_kernel<W, 2, 2, GL, DOT>, 64 * CSRLB_WAVES, L.P.lds));
    per_cu = std::max(1, per_cu);
  }
  pyn_ctx* c = L.c;
  *grid = persistent_grid(L, (L.s1 - L.s0 + CSRLB_WAVES - 1) / CSRLB_WAVES, 256 * per_cu);
  PYN_CHECK(L.poff + *grid <= PYN_MAX_PARTIALS, "partial buffer overflow");
  csrlb_spmv_kernel<W, 2, 2, GL, DOT><<<*grid, 64 * CSRLB_WAVES, L.P.lds, L.st>>>(c->d_rowptr, c->sell_pid, c->sell_tab, c->sell_npat, L.A.val,
                                                                                  L.x, L.y, c->n_owned * L.A.br, L.s1, L.flag, L.part, L.s0,
                                                                                  L.poff, L.hb, L.hl);
  return PYN_OK;
}

// block-CSR values, G lanes per node row
template <int BR, int BC, int U, bool DOT>
int launch_bcsr_u(const Launch& L, int* grid) {
  static int per_cu = 0;
  if (!per_cu) {
    PYN_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bcsr_spmv_kernel<BR, BC, U, DOT>, 256, 0));
    per_cu = std::max(1, std::min(per_cu, 8));
  }
  pyn_ctx* c = L.c;
  const int npw = 64 >> L.P.lg;
  *grid = persistent_grid(L, (L.s1 - L.s0 + 4 * npw - 1) / (4 * npw), 256 * per_cu);
  PYN_CHECK(L.poff + *grid <= PYN_MAX_PARTIALS, "partial buffer overflow");
  bcsr_spmv_kernel<BR, BC, U, DOT><<<*grid, 256, 0, L.st>>>(c->d_rowptr, c->d_colidx, L.A.val, L.x, L.y, L.P.lg, L.s0, L.s1, L.hb, L.hl, L.flag,
                                                            L.part, L.poff, L.A.rhs_compact ? L.A.c_rsel : nullptr,
                                                            L.A.rhs_compact ? L.A.c_cptr : nullptr);
  return PYN_OK;
}
template <int BR, int BC, bool DOT>
int launch_bcsr(const Launch& L, int* grid) {
  switch (L.P.unroll) {
    case 2: return launch_bcsr_u<BR, BC, 2, DOT>(L, grid);
    case 3: return launch_bcsr_u<BR, BC, 3, DOT>(L, grid);
    case 8: return launch_bcsr_u<BR, BC, 8, DOT>(L, grid);
    default: return launch_bcsr_u<BR, BC, 4, DOT>(L, grid);
  }
}
}  // namespace

// Every assembled product launch: range checks and hole arithmetic, the grid, the family's launcher, the record.
int pyn_sell_spmv_range2(pyn_ctx* c, const DMat& A, const ProductPlan& P, const double* x, double* y, bool dot, int64_t a0, int64_t a1,
                         int64_t b0, int64_t b1, int poff, int max_grid, hipStream_t st, int* grid_out) {
  const SellShape* S = pyn_sell_shape(c, A);
  const int64_t ns = (c->n_owned * A.br + SH - 1) / SH;
  PYN_CHECK(P.kind == PK_RAW || (P.kind != PK_NONE && S), "pyn_sell_ensure first");
  PYN_CHECK(!dot || A.br == A.bc, "fused dot needs a square block shape");
  PYN_CHECK(a0 >= 0 && a0 <= a1 && a1 <= b0 && b0 <= b1 && b1 <= ns, "bad slice ranges");
  const int64_t hb = a1, hl = b0 - a1;        // hole in logical coordinates
  const int64_t s0 = a0, s1 = b1 - hl;        // logical range
  if (grid_out) *grid_out = 0;
  if (s0 == s1 && P.kind != PK_RAW) return PYN_OK;   // (the raw product of an empty rank keeps its one workgroup: a zero partial)
  max_grid = std::min(max_grid, P.max_grid);
  int grid = (int)std::max<int64_t>(1, std::min<int64_t>((s1 - s0 + 3) / 4, max_grid));   // the image kernels: four slices per workgroup
  PYN_CHECK(poff + grid <= PYN_MAX_PARTIALS, "partial buffer overflow");
  Launch L{c, A, S, P, x, y, dot ? c->d_flag : nullptr, dot ? c->d_part : nullptr, s0, s1, hb, hl, poff, max_grid, st};
  int p1 = P.W, rc = PYN_OK;
  switch (P.kind) {
    case PK_RAW:
      PYN_CHECK(s0 == 0 && s1 == ns && poff == 0, "32-lane block-CSR product: whole products only");
      rc = dot ? launch_raw<true>(L, &grid) : launch_raw<false>(L, &grid);
      break;
    case PK_SELL:
    case PK_SELLP: rc = dot ? launch_sell<true>(L, grid) : launch_sell<false>(L, grid); break;
    case PK_SELLB_X:
    case PK_SELLB_D:
      p1 = A.bc;
      switch (A.bc) {
        case 1: rc = dot ? launch_sellb<1, true>(L, grid) : launch_sellb<1, false>(L, grid); break;
        case 2: rc = dot ? launch_sellb<2, true>(L, grid) : launch_sellb<2, false>(L, grid); break;
        case 3: rc = dot ? launch_sellb<3, true>(L, grid) : launch_sellb<3, false>(L, grid); break;
        default: rc = dot ? launch_sellb<6, true>(L, grid) : launch_sellb<6, false>(L, grid);
      }
      break;
    case PK_CSRL:
      rc = P.W == 27 ? (dot ? launch_csrl<27, true>(L, &grid) : launch_csrl<27, false>(L, &grid))
                     : (dot ? launch_csrl<32, true>(L, &grid) : launch_csrl<32, false>(L, &grid));
      break;
    case PK_CSRLB:
      rc = P.W == 18   ? (dot ? launch_csrlb<18, true>(L, &grid) : launch_csrlb<18, false>(L, &grid))
           : P.W == 32 ? (dot ? launch_csrlb<32, true>(L, &grid) : launch_csrlb<32, false>(L, &grid))
                       : (dot ? launch_csrlb<50, true>(L, &grid) : launch_csrlb<50, false>(L, &grid));
      break;
    case PK_BCSR: {
      // slice boundaries become node boundaries (floor: a node that straddles an interior and a boundary slice has no ghost column,
      // either side may take it)
      auto node_of = [&](int64_t sl) { return std::min<int64_t>(c->n_owned, sl * SH / A.br); };
      int64_t na0 = node_of(a0), na1 = node_of(a1), nb0 = node_of(b0), nb1 = node_of(b1);
      if (A.rhs_compact) {   // whole products only (a right-hand-side operator is never split for a halo overlap): all stored rows
        PYN_CHECK(a0 == 0 && b1 == S->ns && a1 == b0 && !dot, "compact imposed-column matrix: whole products only");
        na0 = 0;
        na1 = nb0 = nb1 = A.c_nr;
      }
      L.s0 = na0, L.s1 = nb1 - (nb0 - na1), L.hb = na1, L.hl = nb0 - na1;   // node rows from here on
      if (L.s0 >= L.s1) return PYN_OK;
      p1 = 1 << P.lg;
      switch (A.br * 8 + A.bc) {
        case 1 * 8 + 1: rc = dot ? launch_bcsr<1, 1, true>(L, &grid) : launch_bcsr<1, 1, false>(L, &grid); break;
        case 2 * 8 + 2: rc = dot ? launch_bcsr<2, 2, true>(L, &grid) : launch_bcsr<2, 2, false>(L, &grid); break;
        case 3 * 8 + 3: rc = dot ? launch_bcsr<3, 3, true>(L, &grid) : launch_bcsr<3, 3, false>(L, &grid); break;
        case 2 * 8 + 1: rc = launch_bcsr<2, 1, false>(L, &grid); break;
        case 3 * 8 + 1: rc = launch_bcsr<3, 1, false>(L, &grid); break;
        case 1 * 8 + 2: rc = launch_bcsr<1, 2, false>(L, &grid); break;
        case 1 * 8 + 3: rc = launch_bcsr<1, 3, false>(L, &grid); break;
        case 3 * 8 + 2: rc = launch_bcsr<3, 2, false>(L, &grid); break;
        case 2 * 8 + 3: rc = launch_bcsr<2, 3, false>(L, &grid); break;
        case 6 * 8 + 3: rc = launch_bcsr<6, 3, false>(L, &grid); break;
        case 3 * 8 + 6: rc = launch_bcsr<3, 6, false>(L, &grid); break;
        default: PYN_CHECK(false, "no block-CSR product for block shape %dx%d", A.br, A.bc);
      }
      break;
    }
    case PK_NONE: break;
  }
  PYN_TRY(rc);
  PYN_HIP(hipGetLastError());
  pyn_product_record(c, P.kind, p1, P.unroll, dot, grid, P.kind == PK_RAW ? 0 : S->maxw);
  if (grid_out) *grid_out = grid;
  return PYN_OK;
}

int pyn_sell_spmv(pyn_ctx* c, const DMat& A, const ProductPlan& P, const double* x, double* y, bool dot, int* grid_out) {
  const int64_t ns = (c->n_owned * A.br + SH - 1) / SH;
  return pyn_sell_spmv_range2(c, A, P, x, y, dot, 0, ns, ns, ns, 0, PYN_MAX_PARTIALS, c->stream, grid_out);
}
