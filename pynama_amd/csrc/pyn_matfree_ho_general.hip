// Matrix-free KLE stiffness on ANY quadrilateral / hexahedral mesh of order ngl >= 4 (2-D: ngl 4..12, 3-D: ngl 4..8), one rank:
// PYN_MATFREE_KLE_GENERAL, y = K x for the K of pyn_assemble_kle.  Bent (bilinear / trilinear) cells, any node numbering, cell order,
// cell orientation and vertex valence: what the Gmsh import path (DMPlexDom(fileName=...), _lift_high_order) produces.
//
// Operator: the two-rule form of pyn_matfree_ho.hip with a POINTWISE Jacobian.  The geometry of a cell is the multilinear image of its
// 2^dim corners (the first 2^dim entries of its connectivity), as in the reference (J = HrsCoo . X at every point, spectral.py:120, 140):
//   J[r][x](xi) = sum_b dN_b / d xi_r (xi) X_b[x],  N_b = prod_d (1 +- xi_d) / 2
// in LATTICE orientation (mesh_local_lattice: local node a sits at tensor position loc[a]; 2-D carries the x ~ -r, y ~ -s flip, a
// rotation, so det J keeps its sign).  Every lane forms J at its own Lobatto node (Qd = det J Ji^T Ji of the collocated Laplacian) and,
// lanes t < (ngl - 1)^dim, again at its own Gauss point (Ji, det J of the penalty term).  Nothing of the geometry is stored: it is
// recomputed from the corners on every product.
//
// Mapping: that of ho_cell_kernel (one lane per node, HoCfg cells per workgroup, x_e and the tables in LDS, one barrier per axis), with
// the node of lane t read through the connectivity: conn[cell * NN + a_of_t[t]], a_of_t = the inverse of mesh_local_lattice.  Two passes:
//   1. hog_cell_kernel    y_e = K_e x_e -> scratch [cell][component][t]                      (imposed DOFs of x read as 0)
//   2. hog_gather_kernel  row = the sum of its contributions in the order of a node -> (cell, t) incidence list in CSR form, built on
//                         the host at set time, entries cell * NN + t ascending            (imposed rows: y = x; fused p.Ap)
// Every row is written once, no atomics, no zero fill, bit-identical from run to run; the valence of a node is whatever the mesh has.
#include <numeric>

#include "pyn_ho_tables.h"

using namespace pyn_ho;

namespace {

struct HogArgs {
  const int32_t* conn;     // [n_cells][NN]
  const double* xyz;
  const uint8_t* mask;     // [n_node][DIM] snapshot of the Dirichlet mask, null = nothing imposed
  const double* tab;       // wl Dl wr Br Gr xl xr (HoTab1D::packed)
  const int32_t* aoft;     // [NN] local node at tensor position t
  double* ye;              // [n_cells][DIM][NN] per-cell results
  int n_cells;
  double alpha_d, alpha_w;
};

// the workgroup shape of HoCfg plus what the pointwise geometry stages in LDS: the corners of every cell, the points of both rules
template <int DIM, int N>
struct HogCfg : HoCfg<DIM, N> {
  using B = HoCfg<DIM, N>;
  static constexpr int NC = 1 << DIM;
  static constexpr int CORN = NC * DIM;
  static constexpr int CELL_LDS = B::CELL_LDS + CORN;
  static constexpr int TAB = B::TAB + N + (N - 1);   // + xl, xr
  static_assert((size_t)(B::CPB * CELL_LDS + TAB) * sizeof(double) <= 65536, "static LDS");
  static_assert(CORN <= B::NN, "one lane per corner coordinate");
};

// pass 1: y_e = K_e x_e of every cell.  Lane t of a cell = tensor position t (x fastest) in the full rule and the last stage, item t of
// the intermediate stages (fewer than N^DIM items each).  The contractions are those of ho_cell_kernel.
template <int DIM, int N>
__global__ void __launch_bounds__((HogCfg<DIM, N>::BLOCK)) hog_cell_kernel(HogArgs A, const double* __restrict__ xin, const int* __restrict__ flag) {
  using C = HogCfg<DIM, N>;
  constexpr int NQ = C::NQ, NN = C::NN, NPT = C::NPT, NC = C::NC;
  __shared__ double lds[C::CPB * C::CELL_LDS + C::TAB];
  if (flag && flag[0]) return;
  double* tab = lds + C::CPB * C::CELL_LDS;
  const double* wl = tab;
  const double* Dl = wl + N;          // Dl[i * N + a] = h_a'(x_i)
  const double* wr = Dl + N * N;
  const double* Br = wr + NQ;         // Br[q * N + a] = h_a(g_q)
  const double* Gr = Br + NQ * N;     // Gr[q * N + a] = h_a'(g_q)
  const double* xl = Gr + NQ * N;     // Lobatto nodes
  const double* xr = xl + N;          // Gauss points
  for (int i = threadIdx.x; i < C::TAB; i += C::BLOCK) tab[i] = A.tab[i];
  const int slot = threadIdx.x / NN, t = threadIdx.x - slot * NN;
  double* xs = lds + (slot < C::CPB ? slot : 0) * C::CELL_LDS;   // [DIM][NN]
  double* bufA = xs + C::BUF;
  double* bufB = bufA + C::BUF;
  const double* Xc = bufB + C::BUF;   // [NC][DIM] corner coordinates, corner = lattice bits
  const int ti = t % N, tj = (t / N) % N, tk = DIM == 3 ? t / (N * N) : 0;
  const int a_t = A.aoft[t];
  const int n_groups = (A.n_cells + C::CPB - 1) / C::CPB;
  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int cell = grp * C::CPB + slot;
    const bool act = slot < C::CPB && cell < A.n_cells;
    double Qd[DIM][DIM];
    double y[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) y[p] = 0.0;
    __syncthreads();   // the tables; the previous group's buffers
    if (act) {
      const int32_t* cn = A.conn + (int64_t)cell * NN;
      // ---- this lane's node of x_e, imposed DOFs as 0
      {
        const int64_t node = cn[a_t];
#pragma unroll
        for (int q = 0; q < DIM; ++q) {
          const bool imp = A.mask && A.mask[node * DIM + q];
          xs[q * NN + t] = imp ? 0.0 : xin[node * DIM + q];
        }
      }
      // ---- the corners: lanes t < NC * DIM fetch one coordinate each
      if (t < NC * DIM) {
        const int b = t / DIM, x = t - b * DIM;
        const int tc = (N - 1) * ((b & 1) + N * (((b >> 1) & 1) + (DIM == 3 ? N * ((b >> 2) & 1) : 0)));
        const int64_t node = cn[A.aoft[tc]];
        (bufB + C::BUF)[t] = A.xyz[node * DIM + x];
      }
    }
    __syncthreads();
    if (act) {
      // ---- geometry at this lane's Lobatto node: Ji[x][r] = d(xi_r) / dx (rows = physical axes), Qd = detJ Ji^T Ji (reference axes)
      double Ji[DIM][DIM];
      const double xn[3] = {xl[ti], xl[tj], DIM == 3 ? xl[tk] : 0.0};
      const double det = hog_jac_inv<DIM>(Xc, xn, Ji);
#pragma unroll
      for (int r = 0; r < DIM; ++r)
#pragma unroll
        for (int s = 0; s < DIM; ++s) {
          double q = 0.0;
#pragma unroll
          for (int d = 0; d < DIM; ++d) q = fma(Ji[d][r], Ji[d][s], q);
          Qd[r][s] = det * q;
        }
    }
    // ---- full rule (collocated): the Laplacian of every component
#pragma unroll
    for (int p = 0; p < DIM; ++p) {
      double* fb = (p & 1) ? bufB : bufA;   // [DIM][NN]
      if (act) {
        const double* xc = xs + p * NN;
        double g[DIM];
#pragma unroll
        for (int r = 0; r < DIM; ++r) g[r] = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a) {
          g[0] = fma(Dl[ti * N + a], xc[a + N * (tj + N * tk)], g[0]);
          g[1] = fma(Dl[tj * N + a], xc[ti + N * (a + N * tk)], g[1]);
          if constexpr (DIM == 3) g[2] = fma(Dl[tk * N + a], xc[ti + N * (tj + N * a)], g[2]);
        }
        const double w = wl[ti] * wl[tj] * (DIM == 3 ? wl[tk] : 1.0);
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
          double s = 0.0;
#pragma unroll
          for (int sx = 0; sx < DIM; ++sx) s = fma(Qd[r][sx], g[sx], s);
          fb[r * NN + t] = w * s;
        }
      }
      __syncthreads();
      if (act) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a) {
          s = fma(Dl[a * N + ti], fb[a + N * (tj + N * tk)], s);
          s = fma(Dl[a * N + tj], fb[NN + ti + N * (a + N * tk)], s);
          if constexpr (DIM == 3) s = fma(Dl[a * N + tk], fb[2 * NN + ti + N * (tj + N * a)], s);
        }
        y[p] += s;
      }
    }
    __syncthreads();
    // ---- reduced rule, forward: reference gradient g[q][r] of every component at this lane's point (lanes t < NPT)
    const int qi = t % NQ, qj = (t / NQ) % NQ, qk = DIM == 3 ? t / (NQ * NQ) : 0;
    double g[DIM][DIM];
#pragma unroll
    for (int q = 0; q < DIM; ++q)
#pragma unroll
      for (int r = 0; r < DIM; ++r) g[q][r] = 0.0;
    if constexpr (DIM == 2) {
      constexpr int S1 = NQ * N;
#pragma unroll
      for (int q = 0; q < DIM; ++q) {
        if (act && t < S1) {   // (point i, node j): value and x-derivative along x
          const int i1 = t % NQ, j1 = t / NQ;
          double sb = 0.0, sg = 0.0;
#pragma unroll
          for (int a = 0; a < N; ++a) {
            const double v = xs[q * NN + a + N * j1];
            sb = fma(Br[i1 * N + a], v, sb);
            sg = fma(Gr[i1 * N + a], v, sg);
          }
          bufA[t] = sb;
          bufA[S1 + t] = sg;
        }
        __syncthreads();
        if (act && t < NPT) {
#pragma unroll
          for (int b = 0; b < N; ++b) {
            g[q][0] = fma(Br[qj * N + b], bufA[S1 + qi + NQ * b], g[q][0]);
            g[q][1] = fma(Gr[qj * N + b], bufA[qi + NQ * b], g[q][1]);
          }
        }
        __syncthreads();
      }
    } else {
      constexpr int S1 = NQ * N * N, S2 = NQ * NQ * N;
#pragma unroll
      for (int q = 0; q < DIM; ++q) {
        if (act && t < S1) {   // (point i, node j, node k)
          const int i1 = t % NQ, r1 = t / NQ;
          double sb = 0.0, sg = 0.0;
#pragma unroll
          for (int a = 0; a < N; ++a) {
            const double v = xs[q * NN + a + N * r1];
            sb = fma(Br[i1 * N + a], v, sb);
            sg = fma(Gr[i1 * N + a], v, sg);
          }
          bufA[t] = sb;
          bufA[S1 + t] = sg;
        }
        __syncthreads();
        if (act && t < S2) {   // (point i, point j, node k)
          const int i2 = t % NQ, j2 = (t / NQ) % NQ, k2 = t / (NQ * NQ);
          double bb = 0.0, gb = 0.0, bg = 0.0;
#pragma unroll
          for (int b = 0; b < N; ++b) {
            const double vb = bufA[i2 + NQ * (b + N * k2)], vg = bufA[S1 + i2 + NQ * (b + N * k2)];
            bb = fma(Br[j2 * N + b], vb, bb);
            gb = fma(Br[j2 * N + b], vg, gb);
            bg = fma(Gr[j2 * N + b], vb, bg);
          }
          bufB[t] = bb;
          bufB[S2 + t] = gb;
          bufB[2 * S2 + t] = bg;
        }
        __syncthreads();
        if (act && t < NPT) {
#pragma unroll
          for (int c = 0; c < N; ++c) {
            const int o = qi + NQ * (qj + NQ * c);
            g[q][0] = fma(Br[qk * N + c], bufB[S2 + o], g[q][0]);
            g[q][1] = fma(Br[qk * N + c], bufB[2 * S2 + o], g[q][1]);
            g[q][2] = fma(Gr[qk * N + c], bufB[o], g[q][2]);
          }
        }
        // (the next component's first stage writes bufA, whose readers are behind the barrier above; its second stage writes bufB
        // behind its own first barrier)
      }
      __syncthreads();
    }
    // ---- at the point: D[q][d] = d u_q / d x_d, W[d][p] = alpha_d tr(D) [d == p] + alpha_w (D[p][d] - D[d][p]),
    //      f[p][r] = w detJ sum_d Ji[d][r] W[d][p]
    double f[DIM][DIM];
    if (act && t < NPT) {
      double Ji[DIM][DIM];
      const double xq[3] = {xr[qi], xr[qj], DIM == 3 ? xr[qk] : 0.0};
      const double det = hog_jac_inv<DIM>(Xc, xq, Ji);
      double D[DIM][DIM], tr = 0.0;
#pragma unroll
      for (int q = 0; q < DIM; ++q)
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          double s = 0.0;
#pragma unroll
          for (int r = 0; r < DIM; ++r) s = fma(Ji[d][r], g[q][r], s);
          D[q][d] = s;
        }
#pragma unroll
      for (int q = 0; q < DIM; ++q) tr += D[q][q];
      const double wd = wr[qi] * wr[qj] * (DIM == 3 ? wr[qk] : 1.0) * det;
      const double cd = wd * A.alpha_d, cw = wd * A.alpha_w;
#pragma unroll
      for (int p = 0; p < DIM; ++p) {
        double W[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) W[d] = d == p ? cd * tr : cw * (D[p][d] - D[d][p]);
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
          double s = 0.0;
#pragma unroll
          for (int d = 0; d < DIM; ++d) s = fma(Ji[d][r], W[d], s);
          f[p][r] = s;
        }
      }
    }
    // ---- reduced rule, backward: the transpose of the forward stages, component by component
    if constexpr (DIM == 2) {
      constexpr int S1 = NQ * N;
#pragma unroll
      for (int p = 0; p < DIM; ++p) {
        if (act && t < NPT) {
          bufA[t] = f[p][0];
          bufA[NPT + t] = f[p][1];
        }
        __syncthreads();
        if (act && t < S1) {   // (point i, node b)
          const int i1 = t % NQ, b1 = t / NQ;
          double v0 = 0.0, v1 = 0.0;
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            v0 = fma(Br[j * N + b1], bufA[i1 + NQ * j], v0);
            v1 = fma(Gr[j * N + b1], bufA[NPT + i1 + NQ * j], v1);
          }
          bufB[t] = v0;
          bufB[S1 + t] = v1;
        }
        __syncthreads();
        if (act) {
          double s = 0.0;
#pragma unroll
          for (int i = 0; i < NQ; ++i) {
            s = fma(Gr[i * N + ti], bufB[i + NQ * tj], s);
            s = fma(Br[i * N + ti], bufB[S1 + i + NQ * tj], s);
          }
          y[p] += s;
        }
      }
    } else {
      constexpr int S1 = NQ * N * N, S2 = NQ * NQ * N;
#pragma unroll
      for (int p = 0; p < DIM; ++p) {
        double* X = (p & 1) ? bufB : bufA;
        double* Y = (p & 1) ? bufA : bufB;
        if (act && t < NPT) {
#pragma unroll
          for (int r = 0; r < DIM; ++r) X[r * NPT + t] = f[p][r];
        }
        __syncthreads();
        if (act && t < S2) {   // (point i, point j, node c)
          const int i2 = t % NQ, j2 = (t / NQ) % NQ, c2 = t / (NQ * NQ);
          double u0 = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
          for (int k = 0; k < NQ; ++k) {
            const int o = i2 + NQ * (j2 + NQ * k);
            u0 = fma(Br[k * N + c2], X[o], u0);
            u1 = fma(Br[k * N + c2], X[NPT + o], u1);
            u2 = fma(Gr[k * N + c2], X[2 * NPT + o], u2);
          }
          Y[t] = u0;
          Y[S2 + t] = u1;
          Y[2 * S2 + t] = u2;
        }
        __syncthreads();
        if (act && t < S1) {   // (point i, node b, node c)
          const int i1 = t % NQ, b1 = (t / NQ) % N, c1 = t / (NQ * N);
          double v0 = 0.0, v1 = 0.0;
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            const int o = i1 + NQ * (j + NQ * c1);
            v0 = fma(Br[j * N + b1], Y[o], v0);
            v1 = fma(Gr[j * N + b1], Y[S2 + o], fma(Br[j * N + b1], Y[2 * S2 + o], v1));
          }
          X[t] = v0;
          X[S1 + t] = v1;
        }
        __syncthreads();
        if (act) {
          double s = 0.0;
#pragma unroll
          for (int i = 0; i < NQ; ++i) {
            const int o = i + NQ * (tj + N * tk);
            s = fma(Gr[i * N + ti], X[o], s);
            s = fma(Br[i * N + ti], X[S1 + o], s);
          }
          y[p] += s;
        }
      }
    }
    if (act) {
#pragma unroll
      for (int p = 0; p < DIM; ++p) A.ye[((int64_t)cell * DIM + p) * NN + t] = y[p];
    }
  }
}

// pass 2: every row = the sum of its incidence entries in ascending order
template <int DIM, bool DOT>
__global__ void __launch_bounds__(256) hog_gather_kernel(const int32_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc,
                                                         const double* __restrict__ ye, const uint8_t* __restrict__ mask, int NN, int64_t n_rows,
                                                         const double* __restrict__ xin, double* __restrict__ yout, const int* __restrict__ flag,
                                                         double* __restrict__ part) {
  if (flag && flag[0]) return;
  double dot = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < n_rows; n += (int64_t)gridDim.x * 256) {
    double s[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) s[p] = 0.0;
    const int k1 = inc_ptr[n + 1];
    for (int k = inc_ptr[n]; k < k1; ++k) {
      const int e = inc[k], cell = e / NN, t = e - cell * NN;
#pragma unroll
      for (int p = 0; p < DIM; ++p) s[p] += ye[((int64_t)cell * DIM + p) * NN + t];
    }
#pragma unroll
    for (int p = 0; p < DIM; ++p) {
      const double xv = xin[n * DIM + p];
      const bool imp = mask && mask[n * DIM + p];
      const double yv = imp ? xv : s[p];
      yout[n * DIM + p] = yv;
      if (DOT) dot = fma(yv, xv, dot);
    }
  }
  if (DOT) block_partial(dot, part);
}

// det J > 0 at every Lobatto node and Gauss point of every cell?  (one lane per cell; xl / xr = the points of HoTab1D::packed)
template <int DIM>
__global__ void hog_det_kernel(HogArgs A, int N, int tab_pts, int* __restrict__ bad) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= A.n_cells) return;
  constexpr int NC = 1 << DIM;
  int NN = 1;
  for (int d = 0; d < DIM; ++d) NN *= N;
  const int32_t* cn = A.conn + (int64_t)cell * NN;
  double X[NC * DIM];
#pragma unroll
  for (int b = 0; b < NC; ++b) {
    const int tc = (N - 1) * ((b & 1) + N * (((b >> 1) & 1) + (DIM == 3 ? N * ((b >> 2) & 1) : 0)));
    const int64_t node = cn[A.aoft[tc]];
#pragma unroll
    for (int x = 0; x < DIM; ++x) X[b * DIM + x] = A.xyz[node * DIM + x];
  }
  bool ok = true;
  for (int rule = 0; rule < 2; ++rule) {
    const int n = rule ? N - 1 : N;
    const double* pts = A.tab + tab_pts + (rule ? N : 0);
    for (int k = 0; k < (DIM == 3 ? n : 1); ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
          const double xi[3] = {pts[i], pts[j], DIM == 3 ? pts[k] : 0.0};
          double Ji[DIM][DIM];
          ok = ok && hog_jac_inv<DIM>(X, xi, Ji) > 0.0;
        }
  }
  if (!ok) *bad = 1;
}

template <int DIM, int N>
int launch_hog_cells(pyn_ctx* c, const HogArgs& A, const double* x, const int* flag) {
  using C = HogCfg<DIM, N>;
  const int n_groups = (A.n_cells + C::CPB - 1) / C::CPB;
  const int grid = std::min(n_groups, 256 * 8);
  if (grid == 0) return PYN_OK;
  hog_cell_kernel<DIM, N><<<grid, C::BLOCK, 0, c->stream>>>(A, x, flag);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

int launch_hog_cells_any(pyn_ctx* c, int dim, int ngl, const HogArgs& A, const double* x, const int* flag) {
  if (dim == 2) switch (ngl) {
      case 4: return launch_hog_cells<2, 4>(c, A, x, flag);
      case 5: return launch_hog_cells<2, 5>(c, A, x, flag);
      case 6: return launch_hog_cells<2, 6>(c, A, x, flag);
      case 7: return launch_hog_cells<2, 7>(c, A, x, flag);
      case 8: return launch_hog_cells<2, 8>(c, A, x, flag);
      case 9: return launch_hog_cells<2, 9>(c, A, x, flag);
      case 10: return launch_hog_cells<2, 10>(c, A, x, flag);
      case 11: return launch_hog_cells<2, 11>(c, A, x, flag);
      case 12: return launch_hog_cells<2, 12>(c, A, x, flag);
    }
  if (dim == 3) switch (ngl) {
      case 4: return launch_hog_cells<3, 4>(c, A, x, flag);
      case 5: return launch_hog_cells<3, 5>(c, A, x, flag);
      case 6: return launch_hog_cells<3, 6>(c, A, x, flag);
      case 7: return launch_hog_cells<3, 7>(c, A, x, flag);
      case 8: return launch_hog_cells<3, 8>(c, A, x, flag);
    }
  pyn_set_error("general matrix-free KLE operator: no kernel for dim %d ngl %d", dim, ngl);
  return PYN_EINVAL;
}

HogArgs hog_args(const pyn_ctx* c) {
  HogArgs A;
  A.conn = c->d_conn;
  A.xyz = c->d_xyz;
  A.mask = c->mf_mask[PYN_MATFREE_KLE_GENERAL];
  A.tab = c->d_ho_tab;
  A.aoft = c->hog.aoft;
  A.ye = c->d_ho_ye;
  A.n_cells = (int)c->n_elem;
  A.alpha_d = c->mf_alpha_d[PYN_MATFREE_KLE_GENERAL];
  A.alpha_w = c->mf_alpha_w[PYN_MATFREE_KLE_GENERAL];
  return A;
}

constexpr const char* WHAT = "general matrix-free KLE operator";

}  // namespace

// the uploaded geometry tables (HrsCoo [point][axis][corner], reference order of points and corners) against the multilinear basis of
// the closed form, at the points of both rules (1-D points pts_full [ngl], pts_red [ngl - 1])
int pyn_hog_check_geometry_tables(pyn_ctx* c, const std::vector<double>& pts_full, const std::vector<double>& pts_red, const char* WHAT) {
  const int dim = c->dim, ngl = c->ngl, nc = c->nc;
  std::vector<int> ln;
  ref_local_lattice(ngl, dim, ln);
  double worst = 0.0;
  for (int q = 0; q < 2; ++q) {
    const int n = q ? ngl - 1 : ngl, ngp = c->quad[q].ngp;
    const std::vector<double>& pts = q ? pts_red : pts_full;
    PYN_CHECK(c->quad[q].HrsCoo, "%s (ngl %d): no geometry tables (pyn_elem_tables_set)", WHAT, ngl);
    std::vector<int> lp;
    ref_local_lattice(n, dim, lp);
    std::vector<double> hc((size_t)ngp * dim * nc);
    PYN_HIP(hipMemcpy(hc.data(), c->quad[q].HrsCoo, hc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int g = 0; g < ngp; ++g)
      for (int d = 0; d < dim; ++d)
        for (int b = 0; b < nc; ++b) {
          double v = ln[b * dim + d] > 0 ? 0.5 : -0.5;
          for (int e = 0; e < dim; ++e)
            if (e != d) v *= 0.5 * (1.0 + (ln[b * dim + e] > 0 ? 1.0 : -1.0) * pts[lp[g * dim + e]]);
          worst = std::max(worst, std::fabs(hc[((size_t)g * dim + d) * nc + b] - v));
        }
  }
  PYN_CHECK(worst <= 1e-11, "%s (ngl %d): the geometry tables are not the multilinear basis of the cell's %d corners at the points of "
                            "both rules (largest difference %.3e)", WHAT, ngl, nc, worst);
  return PYN_OK;
}

// a_of_t: the local node at tensor position i + ngl (j + ngl k), the inverse of mesh_local_lattice
void pyn_hog_aoft(int ngl, int dim, std::vector<int32_t>& aoft) {
  std::vector<int> loc;
  mesh_local_lattice(ngl, dim, loc);
  int nn = 1;
  for (int d = 0; d < dim; ++d) nn *= ngl;
  aoft.assign((size_t)nn, -1);
  for (int a = 0; a < nn; ++a) {
    int t = 0;
    for (int d = dim - 1; d >= 0; --d) t = t * ngl + loc[a * dim + d];
    aoft[t] = a;
  }
}

// det J > 0 at every point of both rules of every cell, before anything else touches the cells.  d_tab + tab_pts: the 1-D points of
// the full rule [ngl], then those of the reduced rule [ngl - 1]; `where` names the points in the message.
int pyn_hog_check_det(pyn_ctx* c, const int32_t* d_aoft, const double* d_tab, int tab_pts, const char* what, const char* where) {
  HogArgs A = hog_args(c);
  A.aoft = d_aoft;
  A.tab = d_tab;
  DevTmp flag;
  int h = 0;
  PYN_HIP(flag.alloc(sizeof(int)));
  PYN_HIP(hipMemsetAsync(flag.get(), 0, sizeof(int), c->stream));
  const int ge = (A.n_cells + 63) / 64;
  if (c->dim == 3)
    hog_det_kernel<3><<<ge, 64, 0, c->stream>>>(A, c->ngl, tab_pts, flag.as<int>());
  else
    hog_det_kernel<2><<<ge, 64, 0, c->stream>>>(A, c->ngl, tab_pts, flag.as<int>());
  PYN_HIP(hipGetLastError());
  PYN_HIP(hipMemcpyAsync(&h, flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  PYN_CHECK(!h, "%s (ngl %d): non-positive Jacobian: a cell has det J <= 0 at %s (inverted or "
                "degenerate cell, or a connectivity that does not follow the reference's local node order)", what, c->ngl, where);
  return PYN_OK;
}

// node -> (cell, t) incidence list: a counting sort over the connectivity conn [n_elem][nn] in ascending cell * nn + t
// (ptr [n_node + 1], inc [n_elem * nn]); returns the index of the first connectivity entry out of range, -1 when there is none
int64_t pyn_hog_incidence_host(const int32_t* conn, int64_t n_elem, int nn, int64_t n_node, const int32_t* aoft, std::vector<int32_t>& ptr,
                               std::vector<int32_t>& inc) {
  const int64_t n_ent = n_elem * nn;
  ptr.assign((size_t)n_node + 1, 0);
  inc.assign((size_t)n_ent, 0);
  for (int64_t i = 0; i < n_ent; ++i) {
    if (conn[i] < 0 || conn[i] >= n_node) return i;
    ++ptr[conn[i] + 1];
  }
  std::partial_sum(ptr.begin(), ptr.end(), ptr.begin());
  std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
  for (int64_t e = 0; e < n_elem; ++e)
    for (int t = 0; t < nn; ++t) inc[fill[conn[e * nn + aoft[t]]]++] = (int32_t)(e * nn + t);
  return -1;
}

// ... of the context's mesh, on the device
int pyn_hog_incidence(pyn_ctx* c, const std::vector<int32_t>& aoft, const char* what, DevBuf<int32_t>& d_inc_ptr, DevBuf<int32_t>& d_inc) {
  const int nn = c->nn;
  const int64_t n_node = c->n_node, n_ent = c->n_elem * nn;
  std::vector<int32_t> conn((size_t)n_ent), ptr, inc;
  PYN_HIP(hipMemcpy(conn.data(), c->d_conn, (size_t)n_ent * sizeof(int32_t), hipMemcpyDeviceToHost));
  const int64_t bad = pyn_hog_incidence_host(conn.data(), c->n_elem, nn, n_node, aoft.data(), ptr, inc);
  PYN_CHECK(bad < 0, "%s: conn[%lld] = %d out of range", what, (long long)bad, conn[bad]);
  PYN_HIP(d_inc_ptr.alloc((size_t)n_node + 1));
  PYN_HIP(d_inc.alloc(std::max<size_t>(1, (size_t)n_ent)));
  PYN_HIP(hipMemcpy(d_inc_ptr, ptr.data(), ((size_t)n_node + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  PYN_HIP(hipMemcpy(d_inc, inc.data(), (size_t)n_ent * sizeof(int32_t), hipMemcpyHostToDevice));
  return PYN_OK;
}

// pyn_matfree_set(PYN_MATFREE_KLE_GENERAL): the refusals, the tables, a_of_t, the sign of det J everywhere, the incidence list
int pyn_hog_set(pyn_ctx* c) {
  const int dim = c->dim, ngl = c->ngl, lim = pyn_ho_matfree_max_ngl(dim), nn = c->nn;
  int nn_want = 1;
  for (int d = 0; d < dim; ++d) nn_want *= ngl;
  PYN_CHECK((dim == 2 || dim == 3) && ngl >= 4 && nn == nn_want && c->nc == (1 << dim),
            "%s: needs a quadrilateral / hexahedral mesh of order ngl 4..%d (2-D) / 4..%d (3-D)", WHAT, PYN_HO_MAX_NGL_2D, PYN_HO_MAX_NGL_3D);
  PYN_CHECK(ngl <= lim, "%s: ngl %d is above the limit of %d-D meshes (ngl <= %d; 2-D: %d, 3-D: %d)", WHAT, ngl, dim, lim, PYN_HO_MAX_NGL_2D,
            PYN_HO_MAX_NGL_3D);
  PYN_CHECK(c->nranks == 1 && !c->detached && c->n_ghost == 0 && c->n_owned == c->n_node,
            "%s: runs on one rank (this context: %d ranks, %lld ghost nodes)", WHAT, c->nranks, (long long)c->n_ghost);
  PYN_CHECK(c->n_elem * (int64_t)nn < ((int64_t)1 << 31), "%s: %lld cells of %d nodes: the incidence list needs n_elem * nn < 2^31", WHAT,
            (long long)c->n_elem, nn);
  PYN_HIP(hipSetDevice(c->device));
  const HoTab1D T(ngl);
  PYN_TRY(pyn_ho_check_rules(c, T, WHAT));
  PYN_TRY(pyn_hog_check_geometry_tables(c, T.xl, T.xr, WHAT));
  PYN_TRY(pyn_ho_tab_upload(c, T));
  c->hog = HogState();
  c->mf_set[PYN_MATFREE_KLE_GENERAL] = false;
  std::vector<int32_t> aoft;
  pyn_hog_aoft(ngl, dim, aoft);
  DevBuf<int32_t> d_aoft, d_inc_ptr, d_inc;   // committed together at the end: a refused set leaves no lists behind
  PYN_HIP(d_aoft.alloc((size_t)nn));
  PYN_HIP(hipMemcpy(d_aoft, aoft.data(), (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice));
  const int tab_pts = (int)(T.packed().size() - T.xl.size() - T.xr.size());
  PYN_TRY(pyn_hog_check_det(c, d_aoft, c->d_ho_tab, tab_pts, WHAT, "a Lobatto node or a Gauss point"));
  PYN_TRY(pyn_hog_incidence(c, aoft, WHAT, d_inc_ptr, d_inc));
  c->hog.aoft = std::move(d_aoft);
  c->hog.inc_ptr = std::move(d_inc_ptr);
  c->hog.inc = std::move(d_inc);
  return PYN_OK;
}

// pass 2 of both general operators: every row = the sum of its incidence entries in ascending order, under `mask`.  dot: fused p.Ap
// partials into c->d_part (one per workgroup, *grid_out of them).
int pyn_hog_gather(pyn_ctx* c, const int32_t* inc_ptr, const int32_t* inc, const double* ye, const uint8_t* mask, const double* x, double* y,
                   bool dot, int* grid_out) {
  const int* flag = dot ? c->d_flag : nullptr;
  const int64_t rows = c->n_node;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, PYN_MAX_PARTIALS));
  if (grid_out) *grid_out = grid;
  double* part = dot ? c->d_part : nullptr;
  if (c->dim == 3) {
    if (dot)
      hog_gather_kernel<3, true><<<grid, 256, 0, c->stream>>>(inc_ptr, inc, ye, mask, c->nn, rows, x, y, flag, part);
    else
      hog_gather_kernel<3, false><<<grid, 256, 0, c->stream>>>(inc_ptr, inc, ye, mask, c->nn, rows, x, y, flag, part);
  } else {
    if (dot)
      hog_gather_kernel<2, true><<<grid, 256, 0, c->stream>>>(inc_ptr, inc, ye, mask, c->nn, rows, x, y, flag, part);
    else
      hog_gather_kernel<2, false><<<grid, 256, 0, c->stream>>>(inc_ptr, inc, ye, mask, c->nn, rows, x, y, flag, part);
  }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

// y = K x under the mask snapshot of pyn_matfree_set.  dot: fused p.Ap partials into c->d_part (one per workgroup of the gather pass,
// *grid_out of them).
int pyn_hog_spmv(pyn_ctx* c, const double* x, double* y, bool dot, int* grid_out) {
  PYN_CHECK(c->mf_set[PYN_MATFREE_KLE_GENERAL] && c->d_ho_tab && c->d_ho_ye && c->hog.aoft && c->hog.inc_ptr && c->hog.inc,
            "%s: pyn_matfree_set first", WHAT);
  const HogArgs A = hog_args(c);
  PYN_TRY(launch_hog_cells_any(c, c->dim, c->ngl, A, x, dot ? c->d_flag : nullptr));
  return pyn_hog_gather(c, c->hog.inc_ptr, c->hog.inc, A.ye, A.mask, x, y, dot, grid_out);
}
