// Matrix-free KLE stiffness on second-order structured meshes (ngl 3: 9-node quadrilaterals, 27-node hexahedra) whose cells are all
// parallelograms / parallelepipeds: y = K x for the K of pyn_assemble_kle (pyn_assemble_ho3.hip), recomputed from the node
// coordinates and the element tables on every product instead of streamed from HBM.
//
// Operator (the two-rule form of the header of pyn_assemble_ho3.hip, applied to x):
//   full rule (Gauss 3^dim):    the vector Laplacian, component by component: detJ sum_rs Q_rs Tf_rs,  Q = Ji^T Ji
//   reduced rule (Gauss 2^dim): alpha_d (div u)(div v) + alpha_w curl u . curl v, in the per-point form of lat_affine_apply_kle:
//                               D = grad u (physical), W = alpha_d tr(D) I + alpha_w (D - D^T), test side sum_dp Dv[d][p] W[d][p]
// On an affine cell J^-1 is constant, so both are sum factorisations with 1-D point bases: the 1-D factors of pyn_ho3_tables
// (M = sum w h h, D = sum w h' h, S = sum w h' h' per rule) are split on the host as M = B^T B, D = G^T B, S = G^T G with
// B, G [points][3 nodes] (ho3_matfree_set; the square roots of the weights sit in B and G).  Any such split gives the same
// operator because the point-wise map is the same at every point of an affine cell.  A cell's product runs one z-point slice at
// a time (3-D): 3x3 / 2x3 contractions along one axis at a time, never a dense 27 x 27 block.
//
// Write path as the Q1 shell (MfTile, pyn_assemble_lattice.hip): a workgroup owns TX x TY x TZ node rows (even sizes, tiles start at
// even lattice positions, i.e. on cell boundaries), loads the node box of x that its (TX/2+1)(TY/2+1)(TZ/2+1) cells read into LDS
// (imposed DOFs as 0), lets one lane per cell form y_e = K_e x_e, adds the rows the tile owns with ds_add_f64 and writes every owned
// row once (imposed rows: y = x).  No HBM atomics, no zero fill; the cells on tile borders are computed by both tiles
// ((E+1)/E per axis with E = T/2 cells per tile).
// Dirichlet: a SNAPSHOT of the per-DOF mask taken by pyn_matfree_set, read as "imposed columns eliminated, imposed rows identity" --
// K after Mat.setIndices2One (src/matrices/mat_generator.py:113-118).
// Rank slabs: x carries the ghost tail; planes (3-D) / x-lines (2-D) are numbered through BoxLattice::P as in the assembly.
#include <algorithm>
#include <cmath>

#include "pyn_lattice.h"

namespace {

struct Ho3MfArgs {
  const double* xyz;
  const int32_t* P;        // [npl] first node id of every plane (3-D) / x-line (2-D)
  const uint8_t* mask;     // [n_node][DIM] snapshot of the Dirichlet mask, null = nothing imposed
  int NX, NY, npl, p_own0, n_own;
  int EX, EY, EL;          // cells along x, y (3-D), the slow axis
  int ntx, nty, zb;        // tiles along x, y; first plane of the first tile layer (even)
  double alpha_d, alpha_w;
  Ho3MfBasis b;
};

// slow axis "z" in both dimensions: 2-D tiles are TX x TZ (x-lines along z), TY unused
template <int DIM, int TX, int TY, int TZ>
struct Ho3MfTile {
  static_assert(TX % 2 == 0 && TZ % 2 == 0 && (DIM == 2 || TY % 2 == 0), "tiles start and end on cell boundaries");
  static constexpr int RY = DIM == 3 ? TY : 1;
  static constexpr int BX = TX + 3, BY = DIM == 3 ? TY + 3 : 1, BZ = TZ + 3, NB = BX * BY * BZ;   // node box
  static constexpr int NR = TX * RY * TZ;                                                            // owned rows
  static constexpr int CX = TX / 2 + 1, CY = DIM == 3 ? TY / 2 + 1 : 1, CZ = TZ / 2 + 1, NC = CX * CY * CZ;   // cells
  static constexpr size_t BYTES = (size_t)(NB + NR) * DIM * sizeof(double) + ((NB + 7) & ~7);
  // LDS strides of the in-plane axes (i: x, j: y in 3-D / the slow axis in 2-D) and of the out-of-plane axis (3-D: z)
  static constexpr int SI = DIM, SJ = BX * DIM, SK = BX * BY * DIM;
};

// One slice of the forward map of one component: xc -> reference gradient at the NQ x NQ points of slice k (3-D: z-point k; 2-D: the
// whole cell).  g[r][jq * NQ + iq]: derivative along reference axis r.
template <int DIM, int NQ, int SI, int SJ, int SK>
__device__ __forceinline__ void ho3_fwd_slice(const double* __restrict__ xc, int k, const double (&B)[NQ][3], const double (&G)[NQ][3],
                                              double (&g)[DIM][NQ * NQ]) {
  double xb[3][3], xg[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if constexpr (DIM == 3) {
        double sb = 0.0, sg = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double v = xc[c * SK + j * SJ + i * SI];
          sb = fma(B[k][c], v, sb);
          sg = fma(G[k][c], v, sg);
        }
        xb[j][i] = sb;
        xg[j][i] = sg;
      } else {
        xb[j][i] = xc[j * SJ + i * SI];
      }
    }
  double tb[NQ][3], tg[NQ][3], tz[NQ][3];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double sb = 0.0, sg = 0.0, sz = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        sb = fma(B[q][j], xb[j][i], sb);
        sg = fma(G[q][j], xb[j][i], sg);
        if constexpr (DIM == 3) sz = fma(B[q][j], xg[j][i], sz);
      }
      tb[q][i] = sb;
      tg[q][i] = sg;
      tz[q][i] = sz;
    }
#pragma unroll
  for (int jq = 0; jq < NQ; ++jq)
#pragma unroll
    for (int iq = 0; iq < NQ; ++iq) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        s0 = fma(G[iq][i], tb[jq][i], s0);
        s1 = fma(B[iq][i], tg[jq][i], s1);
        if constexpr (DIM == 3) s2 = fma(B[iq][i], tz[jq][i], s2);
      }
      g[0][jq * NQ + iq] = s0;
      g[1][jq * NQ + iq] = s1;
      if constexpr (DIM == 3) g[2][jq * NQ + iq] = s2;
    }
}

// transpose of ho3_fwd_slice: ye[c * 9 + j * 3 + i] (3-D) / ye[j * 3 + i] (2-D) += sum_r (reference gradient r)^T f[r]
template <int DIM, int NQ>
__device__ __forceinline__ void ho3_bwd_slice(const double (&f)[DIM][NQ * NQ], int k, const double (&B)[NQ][3], const double (&G)[NQ][3],
                                              double* ye) {
  double u0[NQ][3], u1[NQ][3], u2[NQ][3];
#pragma unroll
  for (int jq = 0; jq < NQ; ++jq)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int iq = 0; iq < NQ; ++iq) {
        s0 = fma(G[iq][i], f[0][jq * NQ + iq], s0);
        s1 = fma(B[iq][i], f[1][jq * NQ + iq], s1);
        if constexpr (DIM == 3) s2 = fma(B[iq][i], f[2][jq * NQ + iq], s2);
      }
      u0[jq][i] = s0;
      u1[jq][i] = s1;
      u2[jq][i] = s2;
    }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double hb = 0.0, hg = 0.0;
#pragma unroll
      for (int jq = 0; jq < NQ; ++jq) {
        hb = fma(B[jq][j], u0[jq][i], fma(G[jq][j], u1[jq][i], hb));
        if constexpr (DIM == 3) hg = fma(B[jq][j], u2[jq][i], hg);
      }
      if constexpr (DIM == 3) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ye[c * 9 + j * 3 + i] = fma(B[k][c], hb, fma(G[k][c], hg, ye[c * 9 + j * 3 + i]));
      } else {
        ye[j * 3 + i] += hb;
      }
    }
}

template <int DIM, int TX, int TY, int TZ, bool DG, bool DOT>
__global__ void __launch_bounds__(256) ho3_matfree_kle_kernel(Ho3MfArgs A, const double* __restrict__ xin, double* __restrict__ yout,
                                                              const int* __restrict__ flag, double* __restrict__ part, int n_tiles) {
  using MT = Ho3MfTile<DIM, TX, TY, TZ>;
  constexpr int NS = DIM == 3 ? 3 : 1, NSR = DIM == 3 ? 2 : 1;   // slices of the full / reduced rule
  constexpr int NN = DIM == 3 ? 27 : 9, NP = DIM == 3 ? 3 : 1;   // nodes per cell; curl components
  extern __shared__ __align__(16) double lds[];
  __shared__ double smd[4];
  if (flag && flag[0]) return;
  double* xs = lds;                                                             // [NB][DIM] node box of x, imposed DOFs as 0
  double* acc = xs + MT::NB * DIM;                                              // [NR][DIM]
  unsigned char* nbc = reinterpret_cast<unsigned char*>(acc + MT::NR * DIM);    // [NB] bit q: DOF q imposed
  const int tid = threadIdx.x;
  const int NX = A.NX, NY = A.NY;
  double dot = 0.0;
  for (int tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
    const int bt = xcd_contiguous_tile(tb, n_tiles);
    const int bx = bt % A.ntx, by = DIM == 3 ? (bt / A.ntx) % A.nty : 0, bz = bt / (A.ntx * A.nty);
    const int x0 = bx * TX, y0 = by * TY, z0 = A.zb + bz * TZ;
    for (int i = tid; i < MT::NB; i += 256) {
      const int qx = i % MT::BX, qy = (i / MT::BX) % MT::BY, qz = i / (MT::BX * MT::BY);
      const int x = x0 - 2 + qx, y = DIM == 3 ? y0 - 2 + qy : 0, pl = z0 - 2 + qz;
      double v[DIM];
      unsigned char f = 0;
#pragma unroll
      for (int q = 0; q < DIM; ++q) v[q] = 0.0;
      if (x >= 0 && x < NX && y >= 0 && (DIM == 2 || y < NY) && pl >= 0 && pl < A.npl) {
        const int64_t node = (int64_t)A.P[pl] + (DIM == 3 ? (int64_t)y * NX : 0) + x;
#pragma unroll
        for (int q = 0; q < DIM; ++q) {
          const int fq = A.mask ? (A.mask[node * DIM + q] ? 1 : 0) : 0;
          f |= fq << q;
          v[q] = fq ? 0.0 : xin[node * DIM + q];
        }
      }
#pragma unroll
      for (int q = 0; q < DIM; ++q) xs[i * DIM + q] = v[q];
      nbc[i] = f;
    }
    for (int i = tid; i < MT::NR * DIM; i += 256) acc[i] = 0.0;
    __syncthreads();
    for (int t = tid; t < MT::NC; t += 256) {
      const int lx = t % MT::CX, ly = (t / MT::CX) % MT::CY, lz = t / (MT::CX * MT::CY);
      const int cx = x0 / 2 - 1 + lx, cy = DIM == 3 ? y0 / 2 - 1 + ly : 0, cz = z0 / 2 - 1 + lz;
      if (cx < 0 || cx >= A.EX || cy < 0 || (DIM == 3 && cy >= A.EY) || cz < 0 || cz >= A.EL) continue;
      // ---- geometry of the affine cell: J[r][x] = dx / dr = sum_d C[r][d] E_d[x], E_d = the cell's edge along lattice axis d
      double J[DIM][DIM];
      {
        const int64_t n0 = (int64_t)A.P[2 * cz] + (DIM == 3 ? (int64_t)(2 * cy) * NX : 0) + 2 * cx;
        double X0[DIM], E[DIM][DIM];
#pragma unroll
        for (int x = 0; x < DIM; ++x) X0[x] = A.xyz[n0 * DIM + x];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          const int64_t nd = d == DIM - 1 ? (int64_t)A.P[2 * cz + 2] + (n0 - A.P[2 * cz]) : n0 + (d == 0 ? 2 : 2 * (int64_t)NX);
#pragma unroll
          for (int x = 0; x < DIM; ++x) E[d][x] = A.xyz[nd * DIM + x] - X0[x];
        }
#pragma unroll
        for (int r = 0; r < DIM; ++r)
#pragma unroll
          for (int x = 0; x < DIM; ++x) {
            double sacc = 0.0;
            if (!DG || r == x) {
#pragma unroll
              for (int d = 0; d < DIM; ++d) sacc = fma(A.b.C[r][d], E[d][x], sacc);
            }
            J[r][x] = sacc;
          }
      }
      double Ji[DIM][DIM], det;
      if constexpr (DG) {
        det = 1.0;
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
          det *= J[r][r];
#pragma unroll
          for (int x = 0; x < DIM; ++x) Ji[x][r] = x == r ? 1.0 / J[r][r] : 0.0;
        }
      } else if constexpr (DIM == 2) {
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
      // Ji as used above is (J^-1) with rows = physical axes: J[r][x] = dx / dr, so (J^-1)[x][r] = dr / dx -- the layout of ho3_geom_kernel
      double Qd[DIM][DIM];   // detJ (Ji^T Ji)[r][s]
#pragma unroll
      for (int r = 0; r < DIM; ++r)
#pragma unroll
        for (int s = 0; s < DIM; ++s) {
          double q = 0.0;
#pragma unroll
          for (int d = 0; d < DIM; ++d)
            if (!DG || (d == r && d == s)) q = fma(Ji[d][r], Ji[d][s], q);
          Qd[r][s] = det * q;
        }
      const double* xc0 = xs + ((2 * lz * MT::BY + (DIM == 3 ? 2 * ly : 0)) * MT::BX + 2 * lx) * DIM;
      // rows of the cell that the tile owns += ye (component p)
      auto add_rows = [&](int p, const double (&ye)[NN]) {
#pragma unroll
        for (int a = 0; a < NN; ++a) {
          const int i = a % 3, j = (a / 3) % 3, c = a / 9;   // 2-D: j = the slow axis, c = 0
          const int rx = 2 * lx + i - 2;
          const int ry = DIM == 3 ? 2 * ly + j - 2 : 0;
          const int rz = DIM == 3 ? 2 * lz + c - 2 : 2 * lz + j - 2;
          if (rx < 0 || rx >= TX || ry < 0 || ry >= MT::RY || rz < 0 || rz >= TZ) continue;
          atomicAdd(&acc[((rz * MT::RY + ry) * TX + rx) * DIM + p], ye[a]);
        }
      };
      // ---- full rule: the Laplacian of every component, f_r = detJ sum_s Q_rs g_s at each point (rolled loops: register pressure)
#pragma nounroll
      for (int p = 0; p < DIM; ++p) {
        double ye[NN];
#pragma unroll
        for (int a = 0; a < NN; ++a) ye[a] = 0.0;
#pragma nounroll
        for (int k = 0; k < NS; ++k) {
          double g[DIM][9];
          ho3_fwd_slice<DIM, 3, MT::SI, MT::SJ, MT::SK>(xc0 + p, k, A.b.Bf, A.b.Gf, g);
          double f[DIM][9];
#pragma unroll
          for (int pt = 0; pt < 9; ++pt)
#pragma unroll
            for (int r = 0; r < DIM; ++r) {
              double sacc = 0.0;
#pragma unroll
              for (int sx = 0; sx < DIM; ++sx)
                if (!DG || sx == r) sacc = fma(Qd[r][sx], g[sx][pt], sacc);
              f[r][pt] = sacc;
            }
          ho3_bwd_slice<DIM, 3>(f, k, A.b.Bf, A.b.Gf, ye);
        }
        add_rows(p, ye);
      }
      // ---- reduced rule, pass 1: det alpha_d div u and det alpha_w (D[d][e] - D[e][d]), d < e, at every point
      constexpr int NQR = 4;   // points per slice (2 x 2)
      double tr[NSR][NQR], om[NSR][NP][NQR];
#pragma unroll
      for (int k = 0; k < NSR; ++k)
#pragma unroll
        for (int pt = 0; pt < NQR; ++pt) {
          tr[k][pt] = 0.0;
#pragma unroll
          for (int e = 0; e < NP; ++e) om[k][e][pt] = 0.0;
        }
#pragma unroll
      for (int q = 0; q < DIM; ++q)
#pragma unroll
        for (int k = 0; k < NSR; ++k) {
          double g[DIM][NQR];
          ho3_fwd_slice<DIM, 2, MT::SI, MT::SJ, MT::SK>(xc0 + q, k, A.b.Br, A.b.Gr, g);
#pragma unroll
          for (int pt = 0; pt < NQR; ++pt) {
            double D[DIM];   // physical gradient of component q
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
              double sacc = 0.0;
#pragma unroll
              for (int r = 0; r < DIM; ++r)
                if (!DG || r == d) sacc = fma(Ji[d][r], g[r][pt], sacc);
              D[d] = sacc;
            }
            tr[k][pt] += D[q];
            // curl pairs (d, e), d < e: 2-D (0,1); 3-D (0,1), (0,2), (1,2)
#pragma unroll
            for (int d = 0, e0 = 0; d < DIM; ++d)
#pragma unroll
              for (int e = d + 1; e < DIM; ++e, ++e0) {
                if (q == e) om[k][e0][pt] += D[d];
                if (q == d) om[k][e0][pt] -= D[e];
              }
          }
        }
      const double cd = det * A.alpha_d, cw = det * A.alpha_w;
#pragma unroll
      for (int k = 0; k < NSR; ++k)
#pragma unroll
        for (int pt = 0; pt < NQR; ++pt) {
          tr[k][pt] *= cd;
#pragma unroll
          for (int e = 0; e < NP; ++e) om[k][e][pt] *= cw;
        }
      // ---- reduced rule, pass 2: test side of component p, f_r = sum_d Ji[d][r] W[d][p]
#pragma unroll
      for (int p = 0; p < DIM; ++p) {
        double ye[NN];
#pragma unroll
        for (int a = 0; a < NN; ++a) ye[a] = 0.0;
#pragma unroll
        for (int k = 0; k < NSR; ++k) {
          double f[DIM][NQR];
#pragma unroll
          for (int pt = 0; pt < NQR; ++pt) {
            double W[DIM];   // W[d][p]
#pragma unroll
            for (int d = 0; d < DIM; ++d) W[d] = 0.0;
#pragma unroll
            for (int d = 0, e0 = 0; d < DIM; ++d)
#pragma unroll
              for (int e = d + 1; e < DIM; ++e, ++e0) {
                if (p == e) W[d] = om[k][e0][pt];
                if (p == d) W[e] = -om[k][e0][pt];
              }
            W[p] = tr[k][pt];
#pragma unroll
            for (int r = 0; r < DIM; ++r) {
              double sacc = 0.0;
#pragma unroll
              for (int d = 0; d < DIM; ++d)
                if (!DG || d == r) sacc = fma(Ji[d][r], W[d], sacc);
              f[r][pt] = sacc;
            }
          }
          ho3_bwd_slice<DIM, 2>(f, k, A.b.Br, A.b.Gr, ye);
        }
        add_rows(p, ye);
      }
    }
    __syncthreads();
    for (int s = tid; s < MT::NR * DIM; s += 256) {
      const int r = s / DIM, q = s - r * DIM;
      const int rx = r % TX, ry = (r / TX) % MT::RY, rz = r / (TX * MT::RY);
      const int x = x0 + rx, y = y0 + ry, pl = z0 + rz;
      if (x >= NX || (DIM == 3 && y >= NY) || pl < A.p_own0 || pl >= A.p_own0 + A.n_own) continue;
      const int64_t node = (int64_t)A.P[pl] + (DIM == 3 ? (int64_t)y * NX : 0) + x;
      const int bi = ((rz + 2) * MT::BY + (DIM == 3 ? ry + 2 : 0)) * MT::BX + rx + 2;
      const bool imp = (nbc[bi] >> q) & 1;
      const double xv = imp ? xin[node * DIM + q] : xs[bi * DIM + q];
      const double yv = imp ? xv : acc[s];
      yout[node * DIM + q] = yv;
      if (DOT) dot = fma(yv, xv, dot);
    }
    __syncthreads();
  }
  if (DOT) {
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if ((tid & 63) == 0) smd[tid >> 6] = dot;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = smd[0] + smd[1] + smd[2] + smd[3];
  }
}

template <int DIM, int TX, int TY, int TZ, bool DG, bool DOT>
int launch_ho3_matfree(pyn_ctx* c, Ho3MfArgs& A, const double* x, double* y, int* grid_out) {
  using MT = Ho3MfTile<DIM, TX, TY, TZ>;
  const BoxLattice& L = c->box;
  A.ntx = (L.NX + TX - 1) / TX;
  A.nty = DIM == 3 ? (L.NY + TY - 1) / TY : 1;
  A.zb = L.p_own0 & ~1;
  const int ntz = (L.p_own0 + L.n_own - A.zb + TZ - 1) / TZ;
  const int64_t nt = (int64_t)A.ntx * A.nty * ntz;
  PYN_CHECK(nt < INT32_MAX, "matrix-free operator: %lld tiles", (long long)nt);
  const int n_tiles = (int)nt;
  const int grid = std::min(n_tiles, PYN_MAX_PARTIALS);   // a multiple of 8 whenever it is smaller than n_tiles: the XCD mapping survives
  if (grid_out) *grid_out = grid;
  if (grid == 0) return PYN_OK;
  if (MT::BYTES > 65536)
    PYN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ho3_matfree_kle_kernel<DIM, TX, TY, TZ, DG, DOT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)MT::BYTES));
  ho3_matfree_kle_kernel<DIM, TX, TY, TZ, DG, DOT><<<grid, 256, MT::BYTES, c->stream>>>(A, x, y, DOT ? c->d_flag : nullptr,
                                                                                      DOT ? c->d_part : nullptr, n_tiles);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

// tile shapes: 3-D 10 x 10 x 10 rows (6^3 = 216 cells per 256 lanes, 1.73x cell redundancy, 79 KB of LDS: two workgroups per CU);
// 2-D 30 x 30 rows (16^2 = 256 cells, 1.14x, 32 KB)
template <int DIM, bool DG, bool DOT>
int launch_ho3_matfree_dim(pyn_ctx* c, Ho3MfArgs& A, const double* x, double* y, int* grid_out) {
  if constexpr (DIM == 3)
    return launch_ho3_matfree<3, 10, 10, 10, DG, DOT>(c, A, x, y, grid_out);
  else
    return launch_ho3_matfree<2, 30, 1, 30, DG, DOT>(c, A, x, y, grid_out);
}

// symmetric 3 x 3 eigen-decomposition by cyclic Jacobi rotations: M = V diag(lam) V^T
void sym3_eig(const double (&M)[3][3], double (&lam)[3], double (&V)[3][3]) {
  double a[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      a[i][j] = M[i][j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 50; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double th = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < 3; ++k) {   // a = R^T a R
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = cs * akp - sn * akq;
          a[k][q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = cs * apk - sn * aqk;
          a[q][k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
  }
  for (int i = 0; i < 3; ++i) lam[i] = a[i][i];
}

// the 1-D factors M, D, S (row-major [3][3], M[i][j] = sum w h_i h_j, D[i][j] = sum w h'_i h_j) as M = B^T B, D = G^T B, S = G^T G with
// NQ rows = the rank of M; false when they are not those of one rule with NQ points
template <int NQ>
bool split_rule(const double* M, const double* D, const double* S, double (&B)[NQ][3], double (&G)[NQ][3]) {
  double m[3][3], lam[3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[i][j] = 0.5 * (M[i * 3 + j] + M[j * 3 + i]);
  sym3_eig(m, lam, V);
  int ord[3] = {0, 1, 2};   // descending eigenvalues
  std::sort(ord, ord + 3, [&](int u, int v) { return lam[u] > lam[v]; });
  if (!(lam[ord[NQ - 1]] > 1e-8 * lam[ord[0]])) return false;
  if (NQ < 3 && !(std::fabs(lam[ord[NQ]]) <= 1e-12 * lam[ord[0]])) return false;
  for (int k = 0; k < NQ; ++k) {
    const double l = lam[ord[k]], sl = std::sqrt(l);
    for (int i = 0; i < 3; ++i) {
      B[k][i] = sl * V[i][ord[k]];
      double s = 0.0;
      for (int j = 0; j < 3; ++j) s += D[i * 3 + j] * V[j][ord[k]];
      G[k][i] = s / sl;
    }
  }
  double worst = 0.0, scale = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double bb = 0.0, gb = 0.0, gg = 0.0;
      for (int k = 0; k < NQ; ++k) {
        bb += B[k][i] * B[k][j];
        gb += G[k][i] * B[k][j];
        gg += G[k][i] * G[k][j];
      }
      worst = std::max(worst, std::max(std::fabs(bb - M[i * 3 + j]), std::max(std::fabs(gb - D[i * 3 + j]), std::fabs(gg - S[i * 3 + j]))));
      scale = std::max(scale, std::max(std::fabs(M[i * 3 + j]), std::max(std::fabs(D[i * 3 + j]), std::fabs(S[i * 3 + j]))));
    }
  return worst <= 1e-13 * scale;
}

}  // namespace

// pyn_matfree_set(PYN_MATFREE_KLE) on a second-order lattice: every cell affine, tables that are tensor products of one full (Gauss 3)
// and one reduced (Gauss 2) rule; fills c->mf_ho3
static bool ho3_matfree_mesh(const pyn_ctx* c) { return c->ho3.valid && c->box.ngl == 3; }

static int ho3_matfree_set(pyn_ctx* c, int op) {
  PYN_CHECK(ho3_matfree_mesh(c), "matrix-free operator: not a second-order structured mesh");
  PYN_CHECK(op == PYN_MATFREE_KLE, "matrix-free operator %d: second-order (ngl 3) meshes have the matrix-free KLE operator only "
                                   "(PYN_MATFREE_KLE)", op);
  PYN_CHECK(c->ho3_tabs_nn == c->nn && c->ho3_tabs_ok[0] && c->ho3_tabs_ok[1] && c->ho3_tens_ok && c->quad[0].ngp > 0,
            "matrix-free KLE operator (ngl 3): needs the full- and reduced-rule tables of the tensor-product element (pyn_elem_tables_set)");
  bool affine = false, diag = false;
  Ho3MfBasis b;
  double hc[3][8] = {};
  PYN_TRY(pyn_ho3_cell_facts(c, &affine, &diag, hc));
  const int dim = c->dim;
  for (int r = 0; r < 3; ++r)
    for (int d = 0; d < 3; ++d) {
      b.C[r][d] = 0.0;
      if (r < dim && d < dim)
        for (int cb = 0; cb < (1 << dim); ++cb)
          if ((cb >> d) & 1) b.C[r][d] += hc[r][cb];
    }
  PYN_CHECK(affine, "matrix-free KLE operator (ngl 3): needs affine cells (parallelograms / parallelepipeds); this mesh has a cell "
                    "that is not affine");
  const double* t = c->ho3_t1d_host.data();   // [8][3][3]: Mf Df Sf Mr Dr Sr Mn Dn
  PYN_CHECK(c->ho3_t1d_host.size() >= 54 && split_rule<3>(t, t + 9, t + 18, b.Bf, b.Gf) && split_rule<2>(t + 27, t + 36, t + 45, b.Br, b.Gr),
            "matrix-free KLE operator (ngl 3): the element tables are not those of a 3-point full and a 2-point reduced rule");
  b.diag = diag && !getenv("PYNAMA_HO3_NO_DIAG");
  c->mf_ho3 = b;
  return PYN_OK;
}

// y = K x, K = the KLE stiffness of pyn_assemble_kle on a second-order lattice under the mask snapshot of pyn_matfree_set; x carries
// the ghost tail.  dot: fused p.Ap partials into c->d_part (one per workgroup, *grid_out of them).
static int ho3_matfree_spmv(pyn_ctx* c, int op, const double* x, double* y, bool dot, int* grid_out) {
  PYN_CHECK(ho3_matfree_mesh(c), "matrix-free operator: not a second-order structured mesh");
  PYN_CHECK(op == PYN_MATFREE_KLE && c->mf_set[PYN_MATFREE_KLE], "matrix-free KLE operator: pyn_matfree_set first");
  const BoxLattice& L = c->box;
  Ho3MfArgs A;
  A.xyz = c->d_xyz;
  A.P = L.d_P;
  A.mask = c->mf_mask[PYN_MATFREE_KLE];
  A.NX = L.NX;
  A.NY = L.dim == 3 ? L.NY : 0;
  A.npl = L.npl;
  A.p_own0 = L.p_own0;
  A.n_own = L.n_own;
  A.EX = L.EX;
  A.EY = L.EY;
  A.EL = (L.npl - 1) / 2;
  A.ntx = A.nty = A.zb = 0;
  A.alpha_d = c->mf_alpha_d[PYN_MATFREE_KLE];
  A.alpha_w = c->mf_alpha_w[PYN_MATFREE_KLE];
  A.b = c->mf_ho3;
  const bool dg = c->mf_ho3.diag != 0;
  if (L.dim == 3) {
    if (dg) return dot ? launch_ho3_matfree_dim<3, true, true>(c, A, x, y, grid_out) : launch_ho3_matfree_dim<3, true, false>(c, A, x, y, grid_out);
    return dot ? launch_ho3_matfree_dim<3, false, true>(c, A, x, y, grid_out) : launch_ho3_matfree_dim<3, false, false>(c, A, x, y, grid_out);
  }
  if (dg) return dot ? launch_ho3_matfree_dim<2, true, true>(c, A, x, y, grid_out) : launch_ho3_matfree_dim<2, true, false>(c, A, x, y, grid_out);
  return dot ? launch_ho3_matfree_dim<2, false, true>(c, A, x, y, grid_out) : launch_ho3_matfree_dim<2, false, false>(c, A, x, y, grid_out);
}

// 2 or 3 DOFs per node
static int ho3_matfree_bs(const pyn_ctx* c, int op) { return op == PYN_MATFREE_KLE ? c->dim : 1; }

const MfBackend* pyn_mf_ho3() {
  static const MfBackend b = {ho3_matfree_mesh, ho3_matfree_set, ho3_matfree_bs, ho3_matfree_spmv, nullptr};
  return &b;
}
