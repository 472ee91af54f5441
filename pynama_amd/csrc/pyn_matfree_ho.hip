// Matrix-free KLE stiffness on structured box lattices of affine cells at orders ngl >= 4 (2-D: ngl 4..12, 3-D: ngl 4..8):
// y = K x for the K of pyn_assemble_kle, recomputed from the corner coordinates and 1-D tables on every product.
//
// Operator (the two-rule form of the header of pyn_matfree_ho3.hip at general order):
//   full rule = Lobatto(ngl) ON THE NODES (spectral.py:41-42): the vector Laplacian, component by component, collocated --
//               reference gradient g_r = sum_a h_a'(x_i) x[.., a, ..] along axis r, f = w detJ (Ji^T Ji) g, y += the transpose
//   reduced rule = Gauss(ngl - 1): alpha_d (div u)(div v) + alpha_w curl u . curl v in the per-point form
//               D = grad u (physical), W = alpha_d tr(D) I + alpha_w (D - D^T), test side sum_dp Dv[d][p] W[d][p];
//               values and derivatives at the points by interpolation along one axis at a time
// The cells are affine, so J is one matrix per cell, taken from the cell's edges along the LATTICE axes (J[r] = E_r / 2): the element
// space and both rules are symmetric under a flip of a reference axis, so the lattice orientation gives the reference's operator
// (2-D meshes carry the x ~ -r, y ~ -s flip of SURVEY.md A.2).  The 1-D tables (Lobatto nodes / weights, the derivative matrix at
// the nodes, values and derivatives at the Gauss(ngl - 1) points) are recomputed on the host for the mesh's order
// (pyn_ho_tables_1d) and checked against the uploaded tensor tables in ho_matfree_set.
//
// Mapping: one lane per node of a cell (2-D and low 3-D orders: several cells per workgroup), x_e and the tables in LDS, every
// contraction along one axis with a barrier between the axes.  Two passes:
//   1. ho_cell_kernel    y_e = K_e x_e for every local cell -> scratch [cell][component][node]   (imposed DOFs of x read as 0)
//   2. ho_gather_kernel  owned row = the sum of its <= 2^dim cell contributions in a fixed order  (imposed rows: y = x; fused p.Ap)
// Every owned row is written once, no atomics, no zero fill, bit-identical from run to run.  Cost of the second pass: one write and
// one read of (ngl / (ngl - 1))^dim vectors.
// Dirichlet: a SNAPSHOT of the per-DOF mask taken by pyn_matfree_set.  Rank slabs: x carries the ghost tail; planes (3-D) / x-lines
// (2-D) are numbered through BoxLattice::P; every cell of the local mesh touches an owned plane, so all of them are computed.
#include "pyn_ho_tables.h"

using namespace pyn_ho;

namespace {

struct HoMfArgs {
  const double* xyz;
  const int32_t* P;        // [npl] first node id of every plane (3-D) / x-line (2-D)
  const uint8_t* mask;     // [n_node][DIM] snapshot of the Dirichlet mask, null = nothing imposed
  const double* tab;       // wl Dl wr Br Gr (HoTab1D::packed)
  double* ye;              // [n_cells][DIM][N^DIM] per-cell results
  int NX, NY, npl, p_own0, n_own;
  int EX, EY, EL;          // cells along x, y (3-D; 1 in 2-D), the slow axis
  int n_cells;
  double alpha_d, alpha_w;
};

// pass 1: y_e = K_e x_e of every local cell.  Lane t of a cell = node t (x fastest) in the full rule and the last stage, item t of the
// intermediate stages (fewer than N^DIM items each).
template <int DIM, int N>
__global__ void __launch_bounds__((HoCfg<DIM, N>::BLOCK)) ho_cell_kernel(HoMfArgs A, const double* __restrict__ xin, const int* __restrict__ flag) {
  using C = HoCfg<DIM, N>;
  constexpr int NQ = C::NQ, NN = C::NN, NPT = C::NPT;
  __shared__ double lds[C::CPB * C::CELL_LDS + C::TAB];
  if (flag && flag[0]) return;
  double* tab = lds + C::CPB * C::CELL_LDS;
  const double* wl = tab;
  const double* Dl = wl + N;          // Dl[i * N + a] = h_a'(x_i)
  const double* wr = Dl + N * N;
  const double* Br = wr + NQ;         // Br[q * N + a] = h_a(g_q)
  const double* Gr = Br + NQ * N;     // Gr[q * N + a] = h_a'(g_q)
  for (int i = threadIdx.x; i < C::TAB; i += C::BLOCK) tab[i] = A.tab[i];
  const int slot = threadIdx.x / NN, t = threadIdx.x - slot * NN;
  double* xs = lds + (slot < C::CPB ? slot : 0) * C::CELL_LDS;   // [DIM][NN]
  double* bufA = xs + C::BUF;
  double* bufB = bufA + C::BUF;
  const int ti = t % N, tj = (t / N) % N, tk = DIM == 3 ? t / (N * N) : 0;
  const int n_groups = (A.n_cells + C::CPB - 1) / C::CPB;
  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int cell = grp * C::CPB + slot;
    const bool act = slot < C::CPB && cell < A.n_cells;
    double Ji[DIM][DIM], Qd[DIM][DIM], det = 0.0;
    double y[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) y[p] = 0.0;
    __syncthreads();   // the tables; the previous group's buffers
    if (act) {
      const int cx = cell % A.EX, cy = DIM == 3 ? (cell / A.EX) % A.EY : 0, cz = cell / (A.EX * A.EY);
      const int m = N - 1;
      // ---- this lane's node of x_e, imposed DOFs as 0
      {
        const int pl = DIM == 3 ? m * cz + tk : m * cz + tj;
        const int64_t node = (int64_t)A.P[pl] + (DIM == 3 ? (int64_t)(m * cy + tj) * A.NX : 0) + m * cx + ti;
#pragma unroll
        for (int q = 0; q < DIM; ++q) {
          const bool imp = A.mask && A.mask[node * DIM + q];
          xs[q * NN + t] = imp ? 0.0 : xin[node * DIM + q];
        }
      }
      // ---- geometry of the affine cell: J[r][x] = dx / d(xi_r) = E_r[x] / 2, E_r = the cell's edge along lattice axis r
      double J[DIM][DIM];
      {
        const int64_t n0 = (int64_t)A.P[m * cz] + (DIM == 3 ? (int64_t)(m * cy) * A.NX : 0) + m * cx;
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
          const int64_t nr = r == DIM - 1 ? (int64_t)A.P[m * cz + m] + (n0 - A.P[m * cz]) : n0 + (r == 0 ? m : (int64_t)m * A.NX);
#pragma unroll
          for (int x = 0; x < DIM; ++x) J[r][x] = 0.5 * (A.xyz[nr * DIM + x] - A.xyz[n0 * DIM + x]);
        }
      }
      if constexpr (DIM == 2) {
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        const double rr = 1.0 / det;
        Ji[0][0] = J[1][1] * rr;
        Ji[0][1] = -J[0][1] * rr;
        Ji[1][0] = -J[1][0] * rr;
        Ji[1][1] = J[0][0] * rr;
      } else {
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        const double rr = 1.0 / det;
        Ji[0][0] = c00 * rr;
        Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * rr;
        Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * rr;
        Ji[1][0] = c01 * rr;
        Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * rr;
        Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * rr;
        Ji[2][0] = c02 * rr;
        Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * rr;
        Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * rr;
      }
      // Ji[x][r] = d(xi_r) / dx: rows = physical axes.  Qd = detJ Ji^T Ji (reference axes)
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
    __syncthreads();
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

// pass 2: every owned row = the sum of its cells' contributions (x, then y, then the slow axis; the lower cell first)
template <int DIM, bool DOT>
__global__ void __launch_bounds__(256) ho_gather_kernel(HoMfArgs A, int N, const double* __restrict__ xin, double* __restrict__ yout,
                                                        const int* __restrict__ flag, double* __restrict__ part) {
  if (flag && flag[0]) return;
  const int m = N - 1;
  const int PS = DIM == 3 ? A.NX * A.NY : A.NX;
  const int NN = DIM == 3 ? N * N * N : N * N;
  const int64_t n_rows = (int64_t)A.n_own * PS;
  double dot = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < n_rows; n += (int64_t)gridDim.x * 256) {
    const int pr = (int)(n / PS), in = (int)(n - (int64_t)pr * PS);
    int co[3] = {DIM == 3 ? in % A.NX : in, DIM == 3 ? in / A.NX : A.p_own0 + pr, DIM == 3 ? A.p_own0 + pr : 0};
    const int E[3] = {A.EX, DIM == 3 ? A.EY : A.EL, DIM == 3 ? A.EL : 1};
    int nc[3] = {1, 1, 1}, cc[3][2] = {{0, 0}, {0, 0}, {0, 0}}, cl[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const int c0 = co[d] / m, l0 = co[d] - c0 * m;
      const bool lo = l0 == 0 && c0 > 0, hi = c0 < E[d];   // a cell below / at this coordinate (one of them always)
      cc[d][0] = lo ? c0 - 1 : c0;
      cl[d][0] = lo ? m : l0;
      cc[d][1] = c0;
      cl[d][1] = l0;
      nc[d] = lo && hi ? 2 : 1;
    }
    double s[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) s[p] = 0.0;
    // (fixed trip counts, so that the small index arrays stay in registers)
#pragma unroll
    for (int kz = 0; kz < (DIM == 3 ? 2 : 1); ++kz)
#pragma unroll
      for (int ky = 0; ky < 2; ++ky)
#pragma unroll
        for (int kx = 0; kx < 2; ++kx) {
          if (kx >= nc[0] || ky >= nc[1] || kz >= nc[2]) continue;
          const int64_t cell = cc[0][kx] + (int64_t)A.EX * (cc[1][ky] + (DIM == 3 ? (int64_t)A.EY * cc[2][kz] : 0));
          const int t = cl[0][kx] + N * (cl[1][ky] + (DIM == 3 ? N * cl[2][kz] : 0));
#pragma unroll
          for (int p = 0; p < DIM; ++p) s[p] += A.ye[(cell * DIM + p) * NN + t];
        }
#pragma unroll
    for (int p = 0; p < DIM; ++p) {
      const double xv = xin[n * DIM + p];
      const bool imp = A.mask && A.mask[n * DIM + p];
      const double yv = imp ? xv : s[p];
      yout[n * DIM + p] = yv;
      if (DOT) dot = fma(yv, xv, dot);
    }
  }
  if (DOT) block_partial(dot, part);
}

// every cell a parallelogram / parallelepiped with positive volume?  (corner coordinates only, tolerance of ho3_geom_kernel)
template <int DIM>
__global__ void ho_affine_kernel(HoMfArgs A, int m, int* __restrict__ not_affine) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= A.n_cells) return;
  const int cx = cell % A.EX, cy = DIM == 3 ? (cell / A.EX) % A.EY : 0, cz = cell / (A.EX * A.EY);
  constexpr int NC = 1 << DIM;
  double X[NC][DIM];
#pragma unroll
  for (int b = 0; b < NC; ++b) {
    const int bx = b & 1, by = DIM == 3 ? (b >> 1) & 1 : 0, bz = DIM == 3 ? (b >> 2) & 1 : (b >> 1) & 1;
    const int64_t node = (int64_t)A.P[m * (cz + bz)] + (DIM == 3 ? (int64_t)(m * (cy + by)) * A.NX : 0) + m * (cx + bx);
#pragma unroll
    for (int x = 0; x < DIM; ++x) X[b][x] = A.xyz[node * DIM + x];
  }
  double na = 0.0, h2 = 0.0;
#pragma unroll
  for (int b = 0; b < NC; ++b)
#pragma unroll
    for (int x = 0; x < DIM; ++x) {
      double pr = X[0][x];
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        if ((b >> d) & 1) pr += X[1 << d][x] - X[0][x];
      const double df = X[b][x] - pr;
      na = fma(df, df, na);
      if (b == NC - 1) h2 = fma(X[b][x] - X[0][x], X[b][x] - X[0][x], h2);
    }
  double det;
  if constexpr (DIM == 2) {
    det = (X[1][0] - X[0][0]) * (X[2][1] - X[0][1]) - (X[1][1] - X[0][1]) * (X[2][0] - X[0][0]);
  } else {
    double e[3][3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int x = 0; x < 3; ++x) e[d][x] = X[1 << d][x] - X[0][x];
    det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) + e[0][1] * (e[1][2] * e[2][0] - e[1][0] * e[2][2]) +
          e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
  }
  if (!(na <= 1e-25 * h2) || !(det > 0.0)) *not_affine = 1;
}

template <int DIM, int N>
int launch_ho_cells(pyn_ctx* c, const HoMfArgs& A, const double* x, const int* flag) {
  using C = HoCfg<DIM, N>;
  const int n_groups = (A.n_cells + C::CPB - 1) / C::CPB;
  const int grid = std::min(n_groups, 256 * 8);
  if (grid == 0) return PYN_OK;
  ho_cell_kernel<DIM, N><<<grid, C::BLOCK, 0, c->stream>>>(A, x, flag);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

int launch_ho_cells_any(pyn_ctx* c, int dim, int ngl, const HoMfArgs& A, const double* x, const int* flag) {
  if (dim == 2) switch (ngl) {
      case 4: return launch_ho_cells<2, 4>(c, A, x, flag);
      case 5: return launch_ho_cells<2, 5>(c, A, x, flag);
      case 6: return launch_ho_cells<2, 6>(c, A, x, flag);
      case 7: return launch_ho_cells<2, 7>(c, A, x, flag);
      case 8: return launch_ho_cells<2, 8>(c, A, x, flag);
      case 9: return launch_ho_cells<2, 9>(c, A, x, flag);
      case 10: return launch_ho_cells<2, 10>(c, A, x, flag);
      case 11: return launch_ho_cells<2, 11>(c, A, x, flag);
      case 12: return launch_ho_cells<2, 12>(c, A, x, flag);
    }
  if (dim == 3) switch (ngl) {
      case 4: return launch_ho_cells<3, 4>(c, A, x, flag);
      case 5: return launch_ho_cells<3, 5>(c, A, x, flag);
      case 6: return launch_ho_cells<3, 6>(c, A, x, flag);
      case 7: return launch_ho_cells<3, 7>(c, A, x, flag);
      case 8: return launch_ho_cells<3, 8>(c, A, x, flag);
    }
  pyn_set_error("matrix-free KLE operator: no kernel for dim %d ngl %d", dim, ngl);
  return PYN_EINVAL;
}

HoMfArgs ho_args(const pyn_ctx* c) {
  const BoxLattice& L = c->box;
  HoMfArgs A;
  A.xyz = c->d_xyz;
  A.P = L.d_P;
  A.mask = c->mf_mask[PYN_MATFREE_KLE];
  A.tab = c->d_ho_tab;
  A.ye = c->d_ho_ye;
  A.NX = L.NX;
  A.NY = L.NY;
  A.npl = L.npl;
  A.p_own0 = L.p_own0;
  A.n_own = L.n_own;
  A.EX = L.EX;
  A.EY = L.EY;
  A.EL = L.EL;
  A.n_cells = (int)c->n_elem;
  A.alpha_d = c->mf_alpha_d[PYN_MATFREE_KLE];
  A.alpha_w = c->mf_alpha_w[PYN_MATFREE_KLE];
  return A;
}

}  // namespace

extern "C" int pyn_ho_matfree_max_ngl(int dim) { return dim == 2 ? PYN_HO_MAX_NGL_2D : dim == 3 ? PYN_HO_MAX_NGL_3D : 0; }

extern "C" int pyn_ho_tables_1d(int ngl, double* xl, double* wl, double* Dl, double* xr, double* wr, double* Br, double* Gr) {
  PYN_CHECK(ngl >= 2 && ngl <= 32, "pyn_ho_tables_1d: ngl %d out of range (2..32)", ngl);
  const HoTab1D T(ngl);
  auto put = [](double* dst, const std::vector<double>& v) {
    if (dst) std::copy(v.begin(), v.end(), dst);
  };
  put(xl, T.xl);
  put(wl, T.wl);
  put(Dl, T.Dl);
  put(xr, T.xr);
  put(wr, T.wr);
  put(Br, T.Br);
  put(Gr, T.Gr);
  return PYN_OK;
}

extern "C" int pyn_ho_local_lattice(int ngl, int dim, int32_t* loc) {
  PYN_CHECK(loc && ngl >= 2 && ngl <= 32 && (dim == 2 || dim == 3), "pyn_ho_local_lattice: bad argument");
  std::vector<int> l;
  mesh_local_lattice(ngl, dim, l);
  std::copy(l.begin(), l.end(), loc);
  return PYN_OK;
}

extern "C" int pyn_mesh_ho_lattice(pyn_ctx* c, int* ngl, int* nx, int* ny, int* nz) {
  PYN_CHECK(c && c->n_elem > 0, "pyn_mesh_set first");
  const BoxLattice& L = c->box;
  if (ngl) *ngl = c->ho_valid ? L.ngl : 0;
  if (nx) *nx = c->ho_valid ? L.NX : 0;
  if (ny) *ny = c->ho_valid ? L.ny() : 0;
  if (nz) *nz = c->ho_valid ? L.nz() : 0;
  return PYN_OK;
}

// The ngl >= 4 view of c->box: the orders the kernels are instantiated for.  pyn_mesh_topology keeps reporting kind 0 for these meshes:
// only the matrix-free operator uses the view.
void pyn_ho_view(pyn_ctx* c) {
  const BoxLattice& B = c->box;
  c->ho_valid = B.valid && B.ngl >= 4 && B.ngl <= pyn_ho_matfree_max_ngl(B.dim) && B.plane() <= INT32_MAX / 4 && B.n_own >= 1 &&
                c->n_elem < INT32_MAX && !getenv("PYNAMA_NO_HO_LATTICE");
}

int pyn_ho_check_rules(pyn_ctx* c, const HoTab1D& T, const char* what) {
  const int dim = c->dim, ngl = c->ngl, nn = c->nn, nq = ngl - 1;
  int npt = 1;
  for (int d = 0; d < dim; ++d) npt *= nq;
  PYN_CHECK(c->quad[0].ngp == nn && c->quad[1].ngp == npt && c->quad[1].H && c->quad[1].w,
            "%s (ngl %d): needs the tables of the Lobatto(%d) full rule and the Gauss(%d) reduced rule "
            "(pyn_elem_tables_set)", what, ngl, ngl, nq);
  // the uploaded reduced rule (reference order of points and nodes) against the tensor products of the 1-D tables
  std::vector<double> w((size_t)npt), H((size_t)npt * nn);
  PYN_HIP(hipMemcpy(w.data(), c->quad[1].w, w.size() * sizeof(double), hipMemcpyDeviceToHost));
  PYN_HIP(hipMemcpy(H.data(), c->quad[1].H, H.size() * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<int> ln, lp;
  ref_local_lattice(ngl, dim, ln);
  ref_local_lattice(nq, dim, lp);
  double worst = 0.0;
  for (int g = 0; g < npt; ++g) {
    double wt = 1.0;
    for (int d = 0; d < dim; ++d) wt *= T.wr[lp[g * dim + d]];
    worst = std::max(worst, std::fabs(w[g] - wt));
    for (int a = 0; a < nn; ++a) {
      double hv = 1.0;
      for (int d = 0; d < dim; ++d) hv *= T.Br[(size_t)lp[g * dim + d] * ngl + ln[a * dim + d]];
      worst = std::max(worst, std::fabs(H[(size_t)g * nn + a] - hv));
    }
  }
  PYN_CHECK(worst <= 1e-11, "%s (ngl %d): the element tables are not those of the Gauss(%d) reduced rule on the "
                            "Lobatto(%d) nodes (largest difference %.3e)", what, ngl, nq, ngl, worst);
  return PYN_OK;
}

int pyn_ho_tab_upload(pyn_ctx* c, const HoTab1D& T) {
  const std::vector<double> packed = T.packed();
  DevBuf<double> tab;
  PYN_HIP(tab.alloc(packed.size()));
  PYN_HIP(hipMemcpy(tab, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice));
  if (!c->d_ho_ye) PYN_HIP(c->d_ho_ye.alloc((size_t)c->n_elem * c->nn * c->dim));
  c->d_ho_tab = std::move(tab);   // the one commit: a failure above leaves the tables of the last set
  return PYN_OK;
}

// pyn_matfree_set on a mesh of order ngl >= 4: the refusals, the 1-D tables of the order (checked against the uploaded reduced-rule
// tables), the per-cell scratch
static int ho_matfree_set(pyn_ctx* c, int op) {
  const int dim = c->dim, ngl = c->ngl, lim = pyn_ho_matfree_max_ngl(dim);
  PYN_CHECK(ngl >= 4, "matrix-free operator: not a mesh of order ngl >= 4");
  if (op == PYN_MATFREE_KLE_GENERAL) return pyn_hog_set(c);
  PYN_CHECK(op == PYN_MATFREE_KLE, "matrix-free operator %d: meshes of order ngl >= 4 have the matrix-free KLE operator only "
                                   "(PYN_MATFREE_KLE)", op);
  PYN_CHECK(ngl <= lim, "matrix-free KLE operator: ngl %d is above the limit of %d-D meshes (ngl <= %d; 2-D: %d, 3-D: %d)", ngl, dim, lim,
            PYN_HO_MAX_NGL_2D, PYN_HO_MAX_NGL_3D);
  PYN_CHECK(c->ho_valid, "matrix-free KLE operator (ngl %d): the connectivity is not that of a structured box lattice numbered "
                        "lexicographically (imported / renumbered meshes have no matrix-free form)", ngl);
  PYN_CHECK(c->quad[0].ngp == c->nn, "matrix-free KLE operator (ngl %d): needs the tables of the Lobatto(%d) full rule and the Gauss(%d) "
                                     "reduced rule (pyn_elem_tables_set)", ngl, ngl, ngl - 1);
  PYN_HIP(hipSetDevice(c->device));
  HoMfArgs A = ho_args(c);
  {
    DevTmp flag;
    int h = 0;
    PYN_HIP(flag.alloc(sizeof(int)));
    PYN_HIP(hipMemsetAsync(flag.get(), 0, sizeof(int), c->stream));
    const int ge = (A.n_cells + 255) / 256;
    if (dim == 3)
      ho_affine_kernel<3><<<ge, 256, 0, c->stream>>>(A, ngl - 1, flag.as<int>());
    else
      ho_affine_kernel<2><<<ge, 256, 0, c->stream>>>(A, ngl - 1, flag.as<int>());
    PYN_HIP(hipGetLastError());
    PYN_HIP(hipMemcpyAsync(&h, flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PYN_HIP(hipStreamSynchronize(c->stream));
    PYN_CHECK(!h, "matrix-free KLE operator (ngl %d): needs affine cells (parallelograms / parallelepipeds); this mesh has a cell "
                  "that is not affine", ngl);
  }
  const HoTab1D T(ngl);
  PYN_TRY(pyn_ho_check_rules(c, T, "matrix-free KLE operator"));
  return pyn_ho_tab_upload(c, T);
}

// y = K x under the mask snapshot of pyn_matfree_set; x carries the ghost tail.  dot: fused p.Ap partials into c->d_part (one per
// workgroup of the gather pass, *grid_out of them).
static int ho_matfree_spmv(pyn_ctx* c, int op, const double* x, double* y, bool dot, int* grid_out) {
  if (op == PYN_MATFREE_KLE_GENERAL) return pyn_hog_spmv(c, x, y, dot, grid_out);
  PYN_CHECK(c->ho_valid, "matrix-free operator: not a structured mesh of order ngl >= 4");
  PYN_CHECK(op == PYN_MATFREE_KLE && c->mf_set[PYN_MATFREE_KLE] && c->d_ho_tab && c->d_ho_ye, "matrix-free KLE operator: pyn_matfree_set first");
  const BoxLattice& L = c->box;
  const HoMfArgs A = ho_args(c);
  const int* flag = dot ? c->d_flag : nullptr;
  PYN_TRY(launch_ho_cells_any(c, L.dim, L.ngl, A, x, flag));
  const int64_t rows = L.n_own * L.plane();
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, PYN_MAX_PARTIALS));
  if (grid_out) *grid_out = grid;
  if (L.dim == 3) {
    if (dot)
      ho_gather_kernel<3, true><<<grid, 256, 0, c->stream>>>(A, L.ngl, x, y, flag, c->d_part);
    else
      ho_gather_kernel<3, false><<<grid, 256, 0, c->stream>>>(A, L.ngl, x, y, flag, nullptr);
  } else {
    if (dot)
      ho_gather_kernel<2, true><<<grid, 256, 0, c->stream>>>(A, L.ngl, x, y, flag, c->d_part);
    else
      ho_gather_kernel<2, false><<<grid, 256, 0, c->stream>>>(A, L.ngl, x, y, flag, nullptr);
  }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

// every mesh of order ngl >= 4 is answered here: ho_matfree_set accepts it or says why not
static bool ho_matfree_mesh(const pyn_ctx* c) { return c->ngl >= 4; }
static int ho_matfree_bs(const pyn_ctx* c, int op) { return op == PYN_MATFREE_KLE || op == PYN_MATFREE_KLE_GENERAL ? c->dim : 1; }

const MfBackend* pyn_mf_ho() {
  static const MfBackend b = {ho_matfree_mesh, ho_matfree_set, ho_matfree_bs, ho_matfree_spmv, nullptr};
  return &b;
}
