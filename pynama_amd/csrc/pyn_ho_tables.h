// What the matrix-free KLE kernels with a lane per node / point share (pyn_matfree_ho.hip: box lattices of affine cells at ngl >= 4;
// pyn_matfree_ho_general.hip: any quadrilateral / hexahedral mesh at ngl >= 4; pyn_matfree_ho3_general.hip: any such mesh at ngl 3): the
// 1-D rules and tables of an order, the workgroup shape of the cell pass, the table upload, the Jacobian of a multilinear cell at a point.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "pyn_internal.h"

namespace pyn_ho {

constexpr double PI = 3.14159265358979323846;

// P_n(x) and P_{n-1}(x)
inline void legendre(int n, double x, double& pn, double& pm) {
  double p0 = 1.0, p1 = x;
  if (n == 0) {
    pn = 1.0;
    pm = 0.0;
    return;
  }
  for (int j = 2; j <= n; ++j) {
    const double p2 = ((2 * j - 1) * x * p1 - (j - 1) * p0) / j;
    p0 = p1;
    p1 = p2;
  }
  pn = p1;
  pm = p0;
}

// Gauss-Lobatto-Legendre rule with n points, ascending (Newton on (1 - x^2) P'_{n-1}, src/elements/utilities.py:63-92)
inline void lobatto_rule(int n, double* x, double* w) {
  std::vector<double> t(n), wt(n);
  for (int i = 0; i < n; ++i) {
    double v = std::cos(PI * i / (n - 1)), prev = 2.0;
    for (int it = 0; it < 100 && std::fabs(v - prev) > 1e-16; ++it) {
      prev = v;
      double pn, pm;
      legendre(n - 1, v, pn, pm);
      v = prev - (v * pn - pm) / (n * pn);
    }
    double pn, pm;
    legendre(n - 1, v, pn, pm);
    t[i] = v;
    wt[i] = 2.0 / ((n - 1) * (double)n * pn * pn);
  }
  for (int i = 0; i < n; ++i) {   // t descends from 1 to -1
    x[i] = 0.5 * (t[n - 1 - i] - t[i]);
    w[i] = 0.5 * (wt[n - 1 - i] + wt[i]);
  }
}

// Gauss-Legendre rule with n points, ascending (Newton on P_n)
inline void gauss_rule(int n, double* x, double* w) {
  std::vector<double> t(n), wt(n);
  for (int i = 0; i < n; ++i) {
    double v = std::cos(PI * (i + 0.75) / (n + 0.5)), prev = 2.0, dp = 0.0;
    for (int it = 0; it < 100 && std::fabs(v - prev) > 1e-16; ++it) {
      prev = v;
      double pn, pm;
      legendre(n, v, pn, pm);
      dp = n * (v * pn - pm) / (v * v - 1.0);
      v = prev - pn / dp;
    }
    double pn, pm;
    legendre(n, v, pn, pm);
    dp = n * (v * pn - pm) / (v * v - 1.0);
    t[i] = v;
    wt[i] = 2.0 / ((1.0 - v * v) * dp * dp);
  }
  for (int i = 0; i < n; ++i) {
    x[i] = 0.5 * (t[n - 1 - i] - t[i]);
    w[i] = 0.5 * (wt[n - 1 - i] + wt[i]);
  }
}

// Lagrange cardinal functions of `nodes` and their first derivatives at `pts`: h, dh [npts][n] (src/elements/element.py:17-49)
inline void lagrange_1d(int n, const double* nodes, int npts, const double* pts, double* h, double* dh) {
  for (int a = 0; a < n; ++a) {
    double den = 1.0;
    for (int b = 0; b < n; ++b)
      if (b != a) den *= nodes[a] - nodes[b];
    for (int ip = 0; ip < npts; ++ip) {
      const double x = pts[ip];
      double num = 1.0, acc = 0.0;
      for (int b = 0; b < n; ++b)
        if (b != a) num *= x - nodes[b];
      for (int skip = 0; skip < n; ++skip) {
        if (skip == a) continue;
        double pr = 1.0;
        for (int b = 0; b < n; ++b)
          if (b != a && b != skip) pr *= x - nodes[b];
        acc += pr;
      }
      h[ip * n + a] = num / den;
      dh[ip * n + a] = acc / den;
    }
  }
}

// the 1-D tables of one order, in the layout the kernels read: wl[n] Dl[n][n] wr[n-1] Br[n-1][n] Gr[n-1][n], then the points
// xl[n] xr[n-1] (HoCfg::TAB counts the tables without the points: only the general kernels stage those too)
struct HoTab1D {
  std::vector<double> xl, wl, Dl, xr, wr, Br, Gr;
  explicit HoTab1D(int n) : xl(n), wl(n), Dl((size_t)n * n), xr(n - 1), wr(n - 1), Br((size_t)(n - 1) * n), Gr((size_t)(n - 1) * n) {
    std::vector<double> hl((size_t)n * n);
    lobatto_rule(n, xl.data(), wl.data());
    gauss_rule(n - 1, xr.data(), wr.data());
    lagrange_1d(n, xl.data(), n, xl.data(), hl.data(), Dl.data());
    lagrange_1d(n, xl.data(), n - 1, xr.data(), Br.data(), Gr.data());
  }
  std::vector<double> packed() const {
    std::vector<double> t;
    for (const auto* v : {&wl, &Dl, &wr, &Br, &Gr, &xl, &xr}) t.insert(t.end(), v->begin(), v->end());
    return t;
  }
};

constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

template <int DIM, int N>
struct HoCfg {
  static constexpr int NQ = N - 1, NN = ipow(N, DIM), NPT = ipow(NQ, DIM);
  static constexpr int CPB = NN >= 256 ? 1 : 256 / NN;              // cells per workgroup
  static constexpr int BLOCK = (CPB * NN + 63) / 64 * 64;
  static constexpr int BUF = DIM * NN;                              // one stage buffer (doubles); x_e takes one more
  static constexpr int CELL_LDS = 3 * BUF;
  static constexpr int TAB = N + N * N + NQ + 2 * NQ * N;
  static_assert((size_t)(CPB * CELL_LDS + TAB) * sizeof(double) <= 65536, "static LDS");
  static_assert(BLOCK <= 1024, "workgroup size");
};

// J[r][x] at the point xi of the cell with corners Xc[b][x], b = lattice bits (x the lowest); returns det J and Ji[x][r] = d xi_r / d x
template <int DIM, class XP>
__device__ __forceinline__ double hog_jac_inv(XP Xc, const double* xi, double (*Ji)[DIM]) {
  double fm[DIM], fp[DIM], J[DIM][DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    fm[d] = 0.5 * (1.0 - xi[d]);
    fp[d] = 0.5 * (1.0 + xi[d]);
  }
#pragma unroll
  for (int r = 0; r < DIM; ++r)
#pragma unroll
    for (int x = 0; x < DIM; ++x) J[r][x] = 0.0;
#pragma unroll
  for (int b = 0; b < (1 << DIM); ++b)
#pragma unroll
    for (int r = 0; r < DIM; ++r) {
      double dn = ((b >> r) & 1) ? 0.5 : -0.5;
#pragma unroll
      for (int e = 0; e < DIM; ++e)
        if (e != r) dn *= ((b >> e) & 1) ? fp[e] : fm[e];
#pragma unroll
      for (int x = 0; x < DIM; ++x) J[r][x] = fma(dn, Xc[b * DIM + x], J[r][x]);
    }
  double det;
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
  return det;
}

}  // namespace pyn_ho

// what pyn_matfree_set does for both operators of these orders (pyn_matfree_ho.hip): the uploaded rules against the tensor products of
// the 1-D tables (`what` names the operator in the message); c->d_ho_tab = HoTab1D::packed and the per-cell scratch c->d_ho_ye
int pyn_ho_check_rules(pyn_ctx* c, const pyn_ho::HoTab1D& T, const char* what);
int pyn_ho_tab_upload(pyn_ctx* c, const pyn_ho::HoTab1D& T);
// the general operator (pyn_matfree_ho_general.hip), reached through the backend of pyn_matfree_ho.hip
int pyn_hog_set(pyn_ctx* c);
int pyn_hog_spmv(pyn_ctx* c, const double* x, double* y, bool dot, int* grid_out);
// what the two general operators share (pyn_matfree_ho_general.hip; `what` names the operator in the messages): a_of_t, the geometry
// tables against the multilinear corner basis at the 1-D points of both rules, the device check of det J > 0 at the points
// d_tab[tab_pts ...] (full rule [ngl], reduced rule [ngl - 1]), the node -> (cell, t) incidence list, the gather pass
void pyn_hog_aoft(int ngl, int dim, std::vector<int32_t>& aoft);
int pyn_hog_check_geometry_tables(pyn_ctx* c, const std::vector<double>& pts_full, const std::vector<double>& pts_red, const char* what);
int pyn_hog_check_det(pyn_ctx* c, const int32_t* d_aoft, const double* d_tab, int tab_pts, const char* what, const char* where);
int64_t pyn_hog_incidence_host(const int32_t* conn, int64_t n_elem, int nn, int64_t n_node, const int32_t* aoft, std::vector<int32_t>& ptr,
                               std::vector<int32_t>& inc);
int pyn_hog_incidence(pyn_ctx* c, const std::vector<int32_t>& aoft, const char* what, DevBuf<int32_t>& d_inc_ptr, DevBuf<int32_t>& d_inc);
int pyn_hog_gather(pyn_ctx* c, const int32_t* inc_ptr, const int32_t* inc, const double* ye, const uint8_t* mask, const double* x, double* y,
                   bool dot, int* grid_out);
