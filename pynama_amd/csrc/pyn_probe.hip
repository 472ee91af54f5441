// Point probes: the finite-element interpolant of a nodal vector at arbitrary points of any quadrilateral / hexahedral mesh of order
// ngl <= pyn_ho_matfree_max_ngl(dim).  A probe set is located once, on the device, and sampled as often as wanted:
//
//   location   the cell e and reference position xi of every point solve x(xi) = sum_c N_c(xi) X_c over the 2^dim corners (the first
//              2^dim entries of the connectivity row; corner c sits at reference position ref_local_lattice(2, dim)[c])
//     path 0   rectilinear box lattice (c->box.valid and every node the tensor product of per-axis lines bit for bit, checked on the
//              device): a binary search over the cell edges per axis, xi in closed form; a point on an interior face goes to the
//              lower cell
//     path 1   every other mesh: a uniform bin grid over the bounding box holds, per bin, the cells whose corner bounding box overlaps
//              it (count / scan / fill with integer atomics); every point walks the candidates of its bin with Newton from xi = 0
//              on coordinates taken relative to the cell's first corner (the residual rounds at eps h, wherever the mesh lies;
//              at most 16 steps, stop at |d xi|_inf < 1e-13), accepts a cell at |xi|_inf <= 1 + 1e-10 and keeps the LOWEST accepting
//              cell index, so the result does not depend on the fill order of the bins; the accepted xi then takes two more steps with
//              the residual in double-double, which leaves it at its own rounding (a field's gradient multiplies the error of xi)
//   sampling   out[k][c] = sum_a phi_a(xi_k) u[conn[e_k][a]][c], phi_a = prod_d l_{t_a,d}(xi_d), t_a = ref_local_lattice(ngl, dim)[a],
//              l the Lagrange functions of the ascending Lobatto(ngl) nodes: 16 lanes per point while ngl^dim <= 64, one wave above;
//              the group's first dim * ngl lanes evaluate the 1-D values once, every lane walks its share of the connectivity row,
//              a fixed xor tree sums.  No floating-point atomics: two calls on the same state give identical bits.
//
// A point in no cell has cell -1 and samples NaN; no kernel forms an index from it.
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>
#include <vector>

#include "pyn_ho_tables.h"
#include "pyn_internal.h"

namespace {

constexpr int PROBE_NEWTON_CAP = 16;
constexpr double PROBE_NEWTON_TOL = 1e-13, PROBE_ACCEPT = 1e-10, PROBE_PAD = 1e-9;
constexpr int64_t PROBE_MAX_POINTS = (int64_t)1 << 28;
enum { ST_FOUND = 0, ST_NEWTON = 1, ST_CAND = 2, ST_BAD = 3, ST_COUNT = 4 };

// the corner basis: bit d of sbits[c] is set where corner c sits at xi_d = +1
struct ProbeCorners {
  int sbits[8];
};

// path 0: the lattice, its axis lines (x | y | z in one buffer) and the orientation of the reference axes against the lattice's
struct ProbeBox {
  int dim, m;
  int E[3], N[3];      // cells / nodes per lattice axis
  int off[3];          // first line of axis d in the buffer
  double flip[3];      // xi_d = flip[d] * (lattice-oriented coordinate in [-1, 1])
};

// path 1: the bin grid
struct ProbeBins {
  int nb[3];
  double lo[3], hi[3], inv[3], pad[3];   // bounding box of the corners, bins per unit length, pad of the box
};

__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// order-preserving map of a double to an unsigned integer, for integer atomicMin / atomicMax
__device__ __forceinline__ unsigned long long ord_key(double x) {
  const long long b = __double_as_longlong(x);
  return b < 0 ? ~(unsigned long long)b : (unsigned long long)b | 0x8000000000000000ull;
}
inline double ord_value(unsigned long long k) {
  const unsigned long long b = (k & 0x8000000000000000ull) ? k & 0x7fffffffffffffffull : ~k;
  double x;
  memcpy(&x, &b, sizeof(x));
  return x;
}

// ---- path 0 --------------------------------------------------------------------------------------------------------------------
// node id of lattice position (i, j, k): planes of NX * NY ids along the slow axis
__device__ __forceinline__ int64_t box_node(const ProbeBox& B, const int32_t* __restrict__ P, int i, int j, int k) {
  return B.dim == 3 ? (int64_t)P[k] + (int64_t)j * B.N[0] + i : (int64_t)P[j] + i;
}

// the axis lines: coordinate d of the nodes along lattice axis d through the lattice's first node
__global__ void probe_axes_kernel(ProbeBox B, const int32_t* __restrict__ P, const double* __restrict__ xyz, double* __restrict__ axes) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  for (int d = 0; d < B.dim; ++d)
    if (t < B.N[d]) axes[B.off[d] + t] = xyz[box_node(B, P, d == 0 ? t : 0, d == 1 ? t : 0, d == 2 ? t : 0) * B.dim + d];
}

// every node against the tensor product of the lines, bit for bit (plain store: every writer writes the same value)
__global__ void probe_rect_check_kernel(ProbeBox B, const int32_t* __restrict__ P, const double* __restrict__ xyz,
                                        const double* __restrict__ axes, int64_t n_node, int* __restrict__ stats) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_node) return;
  int ijk[3] = {0, 0, 0};
  int64_t r = t;
  for (int d = 0; d < B.dim; ++d) {
    ijk[d] = (int)(r % B.N[d]);
    r /= B.N[d];
  }
  const int64_t node = box_node(B, P, ijk[0], ijk[1], ijk[2]);
  bool off = false;
  for (int d = 0; d < B.dim; ++d)
    if (__double_as_longlong(xyz[node * B.dim + d]) != __double_as_longlong(axes[B.off[d] + ijk[d]])) off = true;
  if (off) stats[ST_BAD] = 1;
}

// one thread per point: per axis the lowest cell whose upper edge is not below the point, xi in closed form
template <int DIM>
__global__ void __launch_bounds__(256) probe_locate_box_kernel(ProbeBox B, int64_t n, const double* __restrict__ X,
                                                               const double* __restrict__ axes, int32_t* __restrict__ cell,
                                                               double* __restrict__ xi, int* __restrict__ stats) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool hit = k < n;
  int64_t e = 0, stride = 1;
  double x[DIM];
  if (hit) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const double p = X[k * DIM + d];
      const double* ax = axes + B.off[d];
      int lo = 0, hi = B.E[d] - 1;          // first cell with edge[cell + 1] >= p; the last cell when there is none
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ax[(mid + 1) * B.m] >= p) hi = mid;
        else lo = mid + 1;
      }
      double a = ax[lo * B.m], b = ax[(lo + 1) * B.m];
      double v = 2.0 * ((p - a) / (b - a)) - 1.0;
      if (lo > 0) {                         // a rounding error above a face: the lower cell still accepts the point, as on path 1
        const double a0 = ax[(lo - 1) * B.m];
        const double v0 = 2.0 * ((p - a0) / (a - a0)) - 1.0;
        if (v0 <= 1.0 + PROBE_ACCEPT) {
          lo -= 1;
          v = v0;
        }
      }
      if (!(fabs(v) <= 1.0 + PROBE_ACCEPT)) hit = false;
      x[d] = B.flip[d] * fmin(1.0, fmax(-1.0, v));
      e += (int64_t)lo * stride;
      stride *= B.E[d];
    }
  }
  if (k < n) {
    cell[k] = hit ? (int32_t)e : -1;
#pragma unroll
    for (int d = 0; d < DIM; ++d) xi[k * DIM + d] = hit ? x[d] : __longlong_as_double(0x7ff8000000000000ll);
  }
  const int found = wave_sum_i(hit ? 1 : 0);
  if ((threadIdx.x & 63) == 0 && found) atomicAdd(&stats[ST_FOUND], found);
}

// ---- path 1 --------------------------------------------------------------------------------------------------------------------
// bounding box of all cell corners: wave minimum / maximum, then one integer atomic per wave and bound.  box[0..2] min, box[3..5] max
template <int DIM>
__global__ void __launch_bounds__(256) probe_bbox_kernel(int64_t n_elem, int nn, const int32_t* __restrict__ conn,
                                                         const double* __restrict__ xyz, unsigned long long* __restrict__ box) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t e = t < n_elem ? t : n_elem - 1;
  double lo[DIM], hi[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    lo[d] = INFINITY;
    hi[d] = -INFINITY;
  }
#pragma unroll
  for (int c = 0; c < (1 << DIM); ++c) {
    const int64_t node = conn[e * nn + c];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const double v = xyz[node * DIM + d];
      lo[d] = fmin(lo[d], v);
      hi[d] = fmax(hi[d], v);
    }
  }
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    for (int o = 32; o > 0; o >>= 1) {
      lo[d] = fmin(lo[d], __shfl_xor(lo[d], o, 64));
      hi[d] = fmax(hi[d], __shfl_xor(hi[d], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&box[d], ord_key(lo[d]));
      atomicMax(&box[3 + d], ord_key(hi[d]));
    }
  }
}

// bin of coordinate x on axis d: monotone in x and clamped, the same function for the cells' boxes and for the points
__device__ __forceinline__ int probe_bin(const ProbeBins& G, int d, double x) {
  const double f = floor((x - G.lo[d]) * G.inv[d]);
  return f > 0.0 ? (f < (double)(G.nb[d] - 1) ? (int)f : G.nb[d] - 1) : 0;   // NaN (none reaches here) would give 0
}

// corners and padded bounding box of cell e
template <int DIM>
__device__ __forceinline__ void probe_cell_box(int64_t e, int nn, const int32_t* __restrict__ conn, const double* __restrict__ xyz,
                                               double* Xc, double* lo, double* hi) {
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    lo[d] = INFINITY;
    hi[d] = -INFINITY;
  }
#pragma unroll
  for (int c = 0; c < (1 << DIM); ++c) {
    const int64_t node = conn[e * nn + c];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const double v = xyz[node * DIM + d];
      Xc[c * DIM + d] = v;
      lo[d] = fmin(lo[d], v);
      hi[d] = fmax(hi[d], v);
    }
  }
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const double pad = PROBE_PAD * (hi[d] - lo[d]);
    lo[d] -= pad;
    hi[d] += pad;
  }
}

// FILL 0: count[bin] += 1 for every bin the cell's padded box overlaps; FILL 1: the cell into a slot of each of those bins
template <int DIM, int FILL>
__global__ void __launch_bounds__(256) probe_bin_kernel(ProbeBins G, int64_t n_elem, int nn, const int32_t* __restrict__ conn,
                                                        const double* __restrict__ xyz, int32_t* __restrict__ count,
                                                        const int32_t* __restrict__ ptr, int32_t* __restrict__ list) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elem) return;
  double Xc[(1 << DIM) * DIM], lo[DIM], hi[DIM];
  probe_cell_box<DIM>(e, nn, conn, xyz, Xc, lo, hi);
  int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    b0[d] = probe_bin(G, d, lo[d]);
    b1[d] = probe_bin(G, d, hi[d]);
  }
  for (int k = b0[2]; k <= b1[2]; ++k)
    for (int j = b0[1]; j <= b1[1]; ++j)
      for (int i = b0[0]; i <= b1[0]; ++i) {
        const int64_t b = i + (int64_t)G.nb[0] * (j + (int64_t)G.nb[1] * k);
        const int slot = atomicAdd(&count[b], 1);
        if (FILL) list[ptr[b] + slot] = (int32_t)e;
      }
}

// Newton works from differences: the cell's first corner is taken off every corner and off the point.  Differences of nearby doubles
// are exact (or exact to eps h), so the residual p - x(xi) rounds at eps h and not at eps |x|, and the stopping rule in reference
// coordinates can be met at any distance from the origin.  N sums to one and dN to zero over the corners: x(xi) - p and J are unchanged
template <int DIM>
__device__ __forceinline__ void probe_recentre(double* Xc, const double* p, double* q) {
  double o[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    o[d] = Xc[d];
    q[d] = p[d] - o[d];
  }
#pragma unroll
  for (int c = 0; c < (1 << DIM); ++c)
#pragma unroll
    for (int d = 0; d < DIM; ++d) Xc[c * DIM + d] -= o[d];
}

// double-double arithmetic for the residual of the refinement steps (error-free sums and products; one rounding per intrinsic)
struct dd {
  double h, l;
};
__device__ __forceinline__ dd dd_two_sum(double a, double b) {
  const double s = __dadd_rn(a, b), bb = __dsub_rn(s, a);
  return {s, __dadd_rn(__dsub_rn(a, __dsub_rn(s, bb)), __dsub_rn(b, bb))};
}
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
  const double p = __dmul_rn(a.h, b.h);
  const double e = __dadd_rn(fma(a.h, b.h, -p), __dadd_rn(__dmul_rn(a.h, b.l), __dmul_rn(a.l, b.h)));
  return dd_two_sum(p, e);
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
  const dd s = dd_two_sum(a.h, b.h);
  return dd_two_sum(s.h, __dadd_rn(s.l, __dadd_rn(a.l, b.l)));
}

// One Newton step xi += J^-1 (p - x(xi)) on the multilinear map; false where det J <= 0 (or not a number).  EXACT: the residual in
// double-double, so that the step ends at the rounding of xi itself and not at that of evaluating the map
template <int DIM, bool EXACT = false>
__device__ __forceinline__ bool probe_newton_step(const ProbeCorners& Cn, const double* Xc, const double* p, double* xi, double* dmax) {
  double fm[DIM], fp[DIM], r[DIM], J[DIM][DIM];   // J[x][r] = d x_x / d xi_r
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    fm[d] = 0.5 * (1.0 - xi[d]);
    fp[d] = 0.5 * (1.0 + xi[d]);
    r[d] = p[d];
#pragma unroll
    for (int q = 0; q < DIM; ++q) J[d][q] = 0.0;
  }
#pragma unroll
  for (int c = 0; c < (1 << DIM); ++c) {
    const int sb = Cn.sbits[c];
    double N = 1.0, dN[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) N *= ((sb >> d) & 1) ? fp[d] : fm[d];
#pragma unroll
    for (int q = 0; q < DIM; ++q) {
      double v = ((sb >> q) & 1) ? 0.5 : -0.5;
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        if (d != q) v *= ((sb >> d) & 1) ? fp[d] : fm[d];
      dN[q] = v;
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      r[d] = fma(-N, Xc[c * DIM + d], r[d]);
#pragma unroll
      for (int q = 0; q < DIM; ++q) J[d][q] = fma(dN[q], Xc[c * DIM + d], J[d][q]);
    }
  }
  if constexpr (EXACT) {
    dd acc[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) acc[d] = {p[d], 0.0};
#pragma unroll
    for (int c = 0; c < (1 << DIM); ++c) {
      const int sb = Cn.sbits[c];
      dd N = {1.0, 0.0};
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        dd f = dd_two_sum(1.0, ((sb >> d) & 1) ? xi[d] : -xi[d]);
        f.h *= 0.5;
        f.l *= 0.5;
        N = dd_mul(N, f);
      }
#pragma unroll
      for (int d = 0; d < DIM; ++d) acc[d] = dd_add(acc[d], dd_mul(N, dd{-Xc[c * DIM + d], 0.0}));
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) r[d] = acc[d].h + acc[d].l;
  }
  double dx[DIM], det;
  if constexpr (DIM == 2) {
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    if (!(det > 0.0)) return false;
    dx[0] = (J[1][1] * r[0] - J[0][1] * r[1]) / det;
    dx[1] = (J[0][0] * r[1] - J[1][0] * r[0]) / det;
  } else {
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    if (!(det > 0.0)) return false;
    dx[0] = (c00 * r[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r[2]) / det;
    dx[1] = (c01 * r[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r[2]) / det;
    dx[2] = (c02 * r[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r[2]) / det;
  }
  double m = 0.0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    xi[d] += dx[d];
    m = fmax(m, fabs(dx[d]));
  }
  *dmax = m;
  return m == m;
}

// one thread per point: the candidates of its bin, Newton on each, the lowest accepting cell
template <int DIM>
__global__ void __launch_bounds__(256) probe_locate_kernel(ProbeBins G, ProbeCorners Cn, int64_t n, const double* __restrict__ X, int nn,
                                                           const int32_t* __restrict__ conn, const double* __restrict__ xyz,
                                                           const int32_t* __restrict__ ptr, const int32_t* __restrict__ list,
                                                           int32_t* __restrict__ cell, double* __restrict__ xi_out,
                                                           int* __restrict__ stats) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int best = -1, best_steps = 0, ncand = 0;
  double bxi[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) bxi[d] = __longlong_as_double(0x7ff8000000000000ll);
  if (k < n) {
    double p[DIM];
    bool inside = true;
    int64_t b = 0, stride = 1;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      p[d] = X[k * DIM + d];
      if (!(p[d] >= G.lo[d] - G.pad[d] && p[d] <= G.hi[d] + G.pad[d])) inside = false;
    }
    if (inside) {     // only now is a bin formed
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        b += (int64_t)probe_bin(G, d, p[d]) * stride;
        stride *= G.nb[d];
      }
      const int q0 = ptr[b], q1 = ptr[b + 1];
      for (int q = q0; q < q1; ++q) {
        const int e = list[q];
        if (best >= 0 && e > best) continue;
        double Xc[(1 << DIM) * DIM], lo[DIM], hi[DIM];
        probe_cell_box<DIM>(e, nn, conn, xyz, Xc, lo, hi);
        bool in = true;
#pragma unroll
        for (int d = 0; d < DIM; ++d)
          if (!(p[d] >= lo[d] && p[d] <= hi[d])) in = false;
        if (!in) continue;
        ncand += 1;
        double xi[DIM], pc[DIM], dmax = 1.0, amax = 0.0;
        probe_recentre<DIM>(Xc, p, pc);
#pragma unroll
        for (int d = 0; d < DIM; ++d) xi[d] = 0.0;
        int steps = 0;
        bool ok = true;
        while (ok && steps < PROBE_NEWTON_CAP) {
          ok = probe_newton_step<DIM>(Cn, Xc, pc, xi, &dmax);
          steps += 1;
          if (dmax < PROBE_NEWTON_TOL) break;
        }
        if (!ok || !(dmax < PROBE_NEWTON_TOL)) continue;
#pragma unroll
        for (int d = 0; d < DIM; ++d) amax = fmax(amax, fabs(xi[d]));
        if (!(amax <= 1.0 + PROBE_ACCEPT)) continue;
        best = e;
        best_steps = steps;
#pragma unroll
        for (int d = 0; d < DIM; ++d) bxi[d] = xi[d];
      }
      if (best >= 0) {   // the accepted cell: two steps with an exact residual (what a field's gradient multiplies is the error of xi)
        double Xc[(1 << DIM) * DIM], lo[DIM], hi[DIM], dmax, xi[DIM], pc[DIM];
        probe_cell_box<DIM>(best, nn, conn, xyz, Xc, lo, hi);
        probe_recentre<DIM>(Xc, p, pc);
#pragma unroll
        for (int d = 0; d < DIM; ++d) xi[d] = bxi[d];
        const bool ok = probe_newton_step<DIM, true>(Cn, Xc, pc, xi, &dmax) && probe_newton_step<DIM, true>(Cn, Xc, pc, xi, &dmax);
#pragma unroll
        for (int d = 0; d < DIM; ++d) bxi[d] = fmin(1.0, fmax(-1.0, ok ? xi[d] : bxi[d]));
      }
    }
    cell[k] = best;
#pragma unroll
    for (int d = 0; d < DIM; ++d) xi_out[k * DIM + d] = bxi[d];
  }
  const int found = wave_sum_i(best >= 0 ? 1 : 0), smax = wave_max_i(best_steps), cmax = wave_max_i(ncand);
  if ((threadIdx.x & 63) == 0) {
    if (found) atomicAdd(&stats[ST_FOUND], found);
    if (smax) atomicMax(&stats[ST_NEWTON], smax);
    if (cmax) atomicMax(&stats[ST_CAND], cmax);
  }
}

// ---- sampling ------------------------------------------------------------------------------------------------------------------
// LANES lanes per point.  tab: x[ngl] | den[ngl], den_t = prod_{b != t} (x_t - x_b); loc: ref_local_lattice(ngl, DIM)
template <int DIM, int BS, int LANES>
__global__ void __launch_bounds__(256) probe_sample_kernel(int64_t n, int ngl, int nn, const int32_t* __restrict__ cell,
                                                           const double* __restrict__ xi, const int32_t* __restrict__ conn,
                                                           const int32_t* __restrict__ loc, const double* __restrict__ tab,
                                                           const double* __restrict__ u, double* __restrict__ out) {
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
  const int s = threadIdx.x & (LANES - 1);
  const int64_t k = g < n ? g : n - 1;       // spare lane groups redo the last point and write nothing
  const int e = cell[k];
  const bool hit = e >= 0;
  // lane d * ngl + t holds l_t(xi_d)
  double l1 = 0.0;
  if (hit && s < DIM * ngl) {
    const int d = s / ngl, t = s - d * ngl;
    const double x = xi[k * DIM + d];
    double num = 1.0;
    for (int b = 0; b < ngl; ++b)
      if (b != t) num *= x - tab[b];
    l1 = num / tab[ngl + t];
  }
  const int32_t* row = conn + (int64_t)(hit ? e : 0) * nn;
  double acc[BS];
#pragma unroll
  for (int c = 0; c < BS; ++c) acc[c] = 0.0;
  for (int a0 = 0; a0 < nn; a0 += LANES) {   // the same trip count in every lane: the shuffles below need the whole group
    const int a = a0 + s;
    const bool in = a < nn;
    const int aa = in ? a : 0;
    double phi = 1.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) phi *= __shfl(l1, d * ngl + loc[aa * DIM + d], LANES);
    if (in && hit) {
      const int64_t node = row[aa];
#pragma unroll
      for (int c = 0; c < BS; ++c) acc[c] = fma(phi, u[node * BS + c], acc[c]);
    }
  }
#pragma unroll
  for (int m = LANES / 2; m > 0; m >>= 1)
#pragma unroll
    for (int c = 0; c < BS; ++c) acc[c] += __shfl_xor(acc[c], m, LANES);
  if (s == 0 && g < n) {
#pragma unroll
    for (int c = 0; c < BS; ++c) out[k * BS + c] = hit ? acc[c] : __longlong_as_double(0x7ff8000000000000ll);
  }
}

template <int DIM, int BS>
int probe_sample_launch(pyn_ctx* c, const DProbe& S, const double* u, double* out) {
  const int64_t n = S.n;
  if (c->nn <= 64)
    probe_sample_kernel<DIM, BS, 16><<<(unsigned)((n * 16 + 255) / 256), 256, 0, c->stream>>>(n, c->ngl, c->nn, S.cell, S.xi, c->d_conn, c->d_probe_loc,
                                                                                             c->d_probe_tab, u, out);
  else
    probe_sample_kernel<DIM, BS, 64><<<(unsigned)((n * 64 + 255) / 256), 256, 0, c->stream>>>(n, c->ngl, c->nn, S.cell, S.xi, c->d_conn, c->d_probe_loc,
                                                                                             c->d_probe_tab, u, out);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

template <int DIM>
int probe_sample_bs(pyn_ctx* c, const DProbe& S, int bs, const double* u, double* out) {
  switch (bs) {
    case 1: return probe_sample_launch<DIM, 1>(c, S, u, out);
    case 2: return probe_sample_launch<DIM, 2>(c, S, u, out);
    case 3: return probe_sample_launch<DIM, 3>(c, S, u, out);
    case 4: return probe_sample_launch<DIM, 4>(c, S, u, out);
    case 5: return probe_sample_launch<DIM, 5>(c, S, u, out);
    case 6: return probe_sample_launch<DIM, 6>(c, S, u, out);
  }
  pyn_set_error("pyn_probe_sample: block size %d has no kernel (1 .. 6)", bs);
  return PYN_EINVAL;
}

// ---- set-up --------------------------------------------------------------------------------------------------------------------
void probe_lobatto(int n, double* out);

// the local-order table and the 1-D table of (ngl, dim): uploaded once per context and order, kept while a probe set lives
int probe_tables(pyn_ctx* c) {
  if (c->probe_tab_ngl == c->ngl && c->probe_tab_dim == c->dim && c->d_probe_loc && c->d_probe_tab) return PYN_OK;
  const int ngl = c->ngl, dim = c->dim;
  std::vector<int> loc;
  ref_local_lattice(ngl, dim, loc);
  const std::vector<int32_t> loc32(loc.begin(), loc.end());
  std::vector<double> tab((size_t)2 * ngl);
  probe_lobatto(ngl, tab.data());
  for (int t = 0; t < ngl; ++t) {
    double den = 1.0;
    for (int b = 0; b < ngl; ++b)
      if (b != t) den *= tab[t] - tab[b];
    tab[ngl + t] = den;
  }
  DevBuf<int32_t> d_loc;
  DevBuf<double> d_tab;
  PYN_TRY(dev_upload(d_loc, loc32.data(), loc32.size(), c->stream));
  PYN_TRY(dev_upload(d_tab, (const double*)tab.data(), tab.size(), c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  c->d_probe_loc = std::move(d_loc);
  c->d_probe_tab = std::move(d_tab);
  c->probe_tab_ngl = ngl;
  c->probe_tab_dim = dim;
  return PYN_OK;
}

// The ascending Gauss-Lobatto-Legendre nodes as the reference computes them (src/elements/utilities.py:63-92), operation for
// operation: Newton on all nodes together until the largest change is <= 1e-15, then the antisymmetric part.  pyn_ho::lobatto_rule
// iterates node by node and ends one unit in the last place away from it at a node of order 12, which a sample next to a mesh node
// shows as 270 eps sum |phi| |u| against a reference evaluated with the reference's nodes.
void probe_lobatto(int n, double* out) {
  std::vector<double> x((size_t)n), prev((size_t)n, 2.0), leg((size_t)n * n);
  const double step = pyn_ho::PI / (n - 1);
  for (int i = 0; i < n; ++i) x[i] = std::cos(i == n - 1 ? pyn_ho::PI : i * step);
  for (int it = 0; it < 100; ++it) {
    double change = 0.0;
    for (int i = 0; i < n; ++i) change = std::max(change, std::fabs(x[i] - prev[i]));
    if (!(change > 1e-15)) break;
    prev = x;
    for (int i = 0; i < n; ++i) {
      double* l = &leg[(size_t)i * n];
      l[0] = 1.0;
      l[1] = x[i];
      for (int j = 2; j < n; ++j) {
        volatile double a = (2 * j - 1) * x[i], b = (j - 1) * l[j - 2];   // volatile: one rounding per operation, no contraction
        volatile double ab = a * l[j - 1];
        l[j] = (ab - b) / j;
      }
      volatile double xl = x[i] * l[n - 1], den = n * l[n - 1];
      x[i] = prev[i] - (xl - l[n - 2]) / den;
    }
  }
  for (int i = 0; i < n; ++i) out[i] = 0.5 * (x[n - 1 - i] - x[i]);
}

ProbeCorners probe_corners(int dim) {
  std::vector<int> v;
  ref_local_lattice(2, dim, v);
  ProbeCorners Cn{};
  for (int c = 0; c < (1 << dim); ++c)
    for (int d = 0; d < dim; ++d)
      if (v[c * dim + d]) Cn.sbits[c] |= 1 << d;
  return Cn;
}

// path 0, if the mesh allows it: *done says whether the points were located
template <int DIM>
int probe_locate_box(pyn_ctx* c, int64_t n, const double* d_X, DProbe& S, int* d_stats, bool* done) {
  *done = false;
  const BoxLattice& L = c->box;
  if (!L.valid || !L.natural()) return PYN_OK;
  hipStream_t s = c->stream;
  ProbeBox B{};
  B.dim = DIM;
  B.m = L.ngl - 1;
  const int E[3] = {L.EX, DIM == 3 ? L.EY : L.EL, DIM == 3 ? L.EL : 1}, N[3] = {L.NX, L.ny(), L.nz()};
  int total = 0;
  for (int d = 0; d < 3; ++d) {
    B.E[d] = E[d];
    B.N[d] = N[d];
    B.off[d] = total;
    if (d < DIM) total += N[d];
  }
  // orientation: the corner at the low end of every lattice axis sits at reference position ref_local_lattice(2, dim)[a0]
  std::vector<int> ml, rl;
  mesh_local_lattice(2, DIM, ml);
  ref_local_lattice(2, DIM, rl);
  int a0 = -1;
  for (int a = 0; a < (1 << DIM); ++a) {
    bool zero = true;
    for (int d = 0; d < DIM; ++d) zero = zero && ml[a * DIM + d] == 0;
    if (zero) a0 = a;
  }
  PYN_CHECK(a0 >= 0, "pyn_probe_create: internal error, the lattice has no first corner");
  for (int d = 0; d < 3; ++d) B.flip[d] = d < DIM && rl[a0 * DIM + d] ? -1.0 : 1.0;
  DevBuf<double> d_axes;
  PYN_HIP(d_axes.alloc((size_t)total));
  int nmax = std::max(N[0], std::max(N[1], N[2]));
  probe_axes_kernel<<<(unsigned)((nmax + 255) / 256), 256, 0, s>>>(B, L.d_P, c->d_xyz, d_axes);
  probe_rect_check_kernel<<<(unsigned)((c->n_node + 255) / 256), 256, 0, s>>>(B, L.d_P, c->d_xyz, d_axes, c->n_node, d_stats);
  PYN_HIP(hipGetLastError());
  std::vector<double> axes((size_t)total);
  int bad = 0;
  PYN_HIP(hipMemcpyAsync(axes.data(), d_axes, axes.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipMemcpyAsync(&bad, d_stats + ST_BAD, sizeof(int), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  if (bad) return PYN_OK;
  for (int d = 0; d < DIM; ++d)      // the cell edges ascend strictly: the binary search and the closed form need it
    for (int e = 0; e <= E[d]; ++e) {
      const double v = axes[B.off[d] + e * B.m];
      if (!std::isfinite(v) || (e > 0 && !(v > axes[B.off[d] + (e - 1) * B.m]))) return PYN_OK;
    }
  probe_locate_box_kernel<DIM><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(B, n, d_X, d_axes, S.cell, S.xi, d_stats);
  PYN_HIP(hipGetLastError());
  PYN_HIP(hipStreamSynchronize(s));   // d_axes leaves with this frame
  S.path = 0;
  *done = true;
  return PYN_OK;
}

template <int DIM>
int probe_locate_search(pyn_ctx* c, int64_t n, const double* d_X, DProbe& S, int* d_stats) {
  hipStream_t s = c->stream;
  const int64_t ne = c->n_elem;
  const unsigned egrid = (unsigned)((ne + 255) / 256);
  // bounding box of the corners
  DevBuf<unsigned long long> d_box;
  unsigned long long box[6];
  for (int d = 0; d < 3; ++d) {
    box[d] = ~0ull;
    box[3 + d] = 0ull;
  }
  PYN_TRY(dev_upload(d_box, (const unsigned long long*)box, 6, s));
  probe_bbox_kernel<DIM><<<egrid, 256, 0, s>>>(ne, c->nn, c->d_conn, c->d_xyz, d_box);
  PYN_HIP(hipGetLastError());
  PYN_HIP(hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  ProbeBins G{};
  // about one bin per cell, the same count on every axis
  int nb = (int)std::floor(std::pow((double)ne, 1.0 / DIM) + 1e-9);
  nb = std::max(1, std::min(nb, DIM == 2 ? 4096 : 256));
  int64_t nbins = 1;
  for (int d = 0; d < 3; ++d) {
    G.nb[d] = d < DIM ? nb : 1;
    nbins *= G.nb[d];
    G.lo[d] = d < DIM ? ord_value(box[d]) : 0.0;
    G.hi[d] = d < DIM ? ord_value(box[3 + d]) : 0.0;
    PYN_CHECK(std::isfinite(G.lo[d]) && std::isfinite(G.hi[d]), "pyn_probe_create: the mesh has a corner coordinate that is not finite");
    const double ext = G.hi[d] - G.lo[d];
    G.inv[d] = ext > 0.0 ? (double)G.nb[d] / ext : 0.0;
    G.pad[d] = PROBE_PAD * ext;
  }
  // count / scan / fill
  DevBuf<int32_t> d_count, d_ptr, d_list;
  DevTmp tmp;
  PYN_HIP(d_count.alloc((size_t)nbins + 1));
  PYN_HIP(d_ptr.alloc((size_t)nbins + 1));
  PYN_HIP(hipMemsetAsync(d_count, 0, ((size_t)nbins + 1) * sizeof(int32_t), s));
  probe_bin_kernel<DIM, 0><<<egrid, 256, 0, s>>>(G, ne, c->nn, c->d_conn, c->d_xyz, d_count, nullptr, nullptr);
  PYN_HIP(hipGetLastError());
  size_t tb = 0;
  PYN_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_count.get(), d_ptr.get(), (int)(nbins + 1), s));
  PYN_HIP(tmp.alloc(std::max<size_t>(tb, 1)));
  PYN_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.get(), tb, d_count.get(), d_ptr.get(), (int)(nbins + 1), s));
  int32_t total = 0;
  PYN_HIP(hipMemcpyAsync(&total, d_ptr + nbins, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  PYN_CHECK(total >= ne, "pyn_probe_create: internal error, %d bin entries for %lld cells", (int)total, (long long)ne);
  PYN_HIP(d_list.alloc((size_t)total));
  PYN_HIP(hipMemsetAsync(d_count, 0, ((size_t)nbins + 1) * sizeof(int32_t), s));
  probe_bin_kernel<DIM, 1><<<egrid, 256, 0, s>>>(G, ne, c->nn, c->d_conn, c->d_xyz, d_count, d_ptr, d_list);
  probe_locate_kernel<DIM><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(G, probe_corners(DIM), n, d_X, c->nn, c->d_conn, c->d_xyz, d_ptr, d_list,
                                                                      S.cell, S.xi, d_stats);
  PYN_HIP(hipGetLastError());
  PYN_HIP(hipStreamSynchronize(s));   // the bins leave with this frame
  S.path = 1;
  return PYN_OK;
}

template <int DIM>
int probe_locate(pyn_ctx* c, int64_t n, const double* d_X, DProbe& S) {
  DevBuf<int> d_stats;
  PYN_HIP(d_stats.alloc(ST_COUNT));
  PYN_HIP(hipMemsetAsync(d_stats, 0, ST_COUNT * sizeof(int), c->stream));
  bool done = false;
  PYN_TRY(probe_locate_box<DIM>(c, n, d_X, S, d_stats, &done));
  if (!done) PYN_TRY(probe_locate_search<DIM>(c, n, d_X, S, d_stats));
  int st[ST_COUNT];
  PYN_HIP(hipMemcpyAsync(st, d_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  S.found = st[ST_FOUND];
  S.max_newton = st[ST_NEWTON];
  S.max_cand = S.path == 0 ? 1 : st[ST_CAND];
  return PYN_OK;
}

int probe_ready(pyn_ctx* c, const char* what, int id) {
  PYN_CHECK(c, "ctx is NULL");
  PYN_CHECK(id >= 0 && id < (int)c->probes.size() && c->probes[id].live,
            "%s: invalid probe handle %d (pyn_probe_destroy, pyn_mesh_set and pyn_mesh_box end a probe set)", what, id);
  PYN_HIP(hipSetDevice(c->device));
  return PYN_OK;
}

}  // namespace

extern "C" int pyn_probe_create(pyn_ctx* c, int64_t n, const double* X, int* probe_id) {
  PYN_CHECK(c && probe_id, "NULL argument");
  PYN_CHECK(c->n_elem > 0 && c->d_conn && c->d_xyz, "pyn_probe_create: pyn_mesh_set first");
  const int dim = c->dim, ngl = c->ngl, lim = pyn_ho_matfree_max_ngl(dim);
  PYN_CHECK(c->nn != dim + 1 && ngl >= 2, "pyn_probe_create: simplices (nn = %d in %d-D) have no probe; quadrilaterals and hexahedra only", c->nn,
            dim);
  PYN_CHECK(c->nranks == 1 && !c->detached && c->n_ghost == 0 && c->n_owned == c->n_node,
            "pyn_probe_create: point probes run on one rank (this context: %d ranks, %lld ghost nodes)", c->nranks, (long long)c->n_ghost);
  PYN_CHECK(ngl <= lim, "pyn_probe_create: ngl %d is above the limit of %d-D meshes (ngl <= %d)", ngl, dim, lim);
  PYN_CHECK(c->nn == pyn_ho::ipow(ngl, dim) && c->nc == (1 << dim), "pyn_probe_create: nn = %d is not ngl^dim = %d^%d", c->nn, ngl, dim);
  PYN_CHECK(c->n_elem < (int64_t)INT32_MAX, "pyn_probe_create: %lld cells do not fit a 32-bit cell index", (long long)c->n_elem);
  PYN_CHECK(n >= 1, "pyn_probe_create: no points (n = %lld)", (long long)n);
  PYN_CHECK(n <= PROBE_MAX_POINTS, "pyn_probe_create: %lld points exceed the limit of %lld per set", (long long)n, (long long)PROBE_MAX_POINTS);
  PYN_CHECK(X, "pyn_probe_create: X is NULL");
  for (int64_t i = 0; i < n * dim; ++i)
    PYN_CHECK(std::isfinite(X[i]), "pyn_probe_create: point %lld has a coordinate that is not finite", (long long)(i / dim));
  PYN_HIP(hipSetDevice(c->device));
  PYN_TRY(probe_tables(c));
  DProbe S;
  S.n = n;
  DevBuf<double> d_X;
  PYN_HIP(S.cell.alloc((size_t)n));
  PYN_HIP(S.xi.alloc((size_t)n * dim));
  PYN_TRY(dev_upload(d_X, X, (size_t)n * dim, c->stream));
  PYN_TRY(dim == 2 ? probe_locate<2>(c, n, d_X, S) : probe_locate<3>(c, n, d_X, S));   // ends with a synchronise: X is borrowed for the call
  S.live = true;
  c->probes.push_back(std::move(S));
  *probe_id = (int)c->probes.size() - 1;
  return PYN_OK;
}

extern "C" int pyn_probe_info(pyn_ctx* c, int probe_id, int64_t* info) {
  PYN_TRY(probe_ready(c, "pyn_probe_info", probe_id));
  PYN_CHECK(info, "NULL argument");
  const DProbe& S = c->probes[probe_id];
  info[0] = S.n;
  info[1] = S.found;
  info[2] = S.path;
  info[3] = S.max_newton;
  info[4] = S.max_cand;
  return PYN_OK;
}

extern "C" int pyn_probe_get(pyn_ctx* c, int probe_id, int32_t* cell, double* xi) {
  PYN_TRY(probe_ready(c, "pyn_probe_get", probe_id));
  const DProbe& S = c->probes[probe_id];
  if (cell) PYN_HIP(hipMemcpyAsync(cell, S.cell, (size_t)S.n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (xi) PYN_HIP(hipMemcpyAsync(xi, S.xi, (size_t)S.n * c->dim * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}

extern "C" int pyn_probe_sample(pyn_ctx* c, int probe_id, int vec_id, double* out) {
  PYN_TRY(probe_ready(c, "pyn_probe_sample", probe_id));
  PYN_CHECK(out, "NULL argument");
  PYN_TRY(pyn_check_vec(c, vec_id, "pyn_probe_sample"));
  DProbe& S = c->probes[probe_id];
  const DVec& v = c->vecs[vec_id];
  PYN_CHECK(v.bs >= 1 && v.d.size() == (size_t)c->n_node * v.bs, "pyn_probe_sample: the vector holds %lld nodes, the mesh has %lld",
            (long long)(v.d.size() / (size_t)std::max(v.bs, 1)), (long long)c->n_node);
  PYN_HIP(S.out.grow((size_t)S.n * v.bs));
  PYN_TRY(c->dim == 2 ? probe_sample_bs<2>(c, S, v.bs, v.d, S.out) : probe_sample_bs<3>(c, S, v.bs, v.d, S.out));
  PYN_HIP(hipMemcpyAsync(out, S.out, (size_t)S.n * v.bs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}

extern "C" int pyn_probe_destroy(pyn_ctx* c, int probe_id) {
  PYN_TRY(probe_ready(c, "pyn_probe_destroy", probe_id));
  PYN_HIP(hipStreamSynchronize(c->stream));   // a queued launch may still read it
  c->probes[probe_id] = DProbe();
  bool any = false;
  for (const DProbe& p : c->probes) any = any || p.live;
  if (!any) {      // the tables leave with the last set: nothing of the feature stays allocated
    c->d_probe_loc.reset();
    c->d_probe_tab.reset();
    c->probe_tab_ngl = c->probe_tab_dim = 0;
  }
  return PYN_OK;
}
