// Matrix-free KLE stiffness on ANY quadrilateral (9-node) / hexahedral (27-node) mesh of order ngl 3, one rank:
// PYN_MATFREE_KLE_NGL3_GENERAL, y = K x for the K of pyn_assemble_kle.  Bent (bilinear / trilinear) cells, any node numbering, cell
// order, orientation-preserving cell orientation and vertex valence: second-order lattices with a cell that is not affine (which
// PYN_MATFREE_KLE refuses) and what the Gmsh import path produces at the reference's own order.
//
// Operator: the two-rule form of the header of pyn_matfree_ho3.hip with a POINTWISE Jacobian.  At ngl <= 3 the full rule of the reference
// is Gauss(3)^dim, not the collocated Lobatto rule of the orders ngl >= 4 (spectral.py:41-42), so BOTH rules interpolate:
//   full rule, Gauss(3)^dim:    the Laplacian of every component p: reference gradient g_r at the 3^dim points by sum factorisation with
//                               the 1-D point bases Bf[q][a] = h_a(g_q), Gf[q][a] = h_a'(g_q) on the Lobatto(3) nodes,
//                               f = w detJ (Ji^T Ji) g, back through the transposed bases
//   reduced rule, Gauss(2)^dim: D = grad u (physical), W = alpha_d tr(D) I + alpha_w (D - D^T), test side sum_dp Dv[d][p] W[d][p],
//                               with Br, Gr at the 2^dim points (the reduced stage of hog_cell_kernel at N = 3)
// The geometry of a cell is the multilinear image of its 2^dim corners (the first 2^dim entries of its connectivity) in LATTICE
// orientation (hog_jac_inv: 2-D carries the x ~ -r, y ~ -s flip, a rotation, so det J keeps its sign), formed at every point of both rules
// on every product.  Nothing of the geometry is stored.
//
// Mapping: lane <-> tensor position t <-> full-rule point t (both count 3^dim), HoCfg<DIM, 3>::CPB cells per 256-lane workgroup (2-D: 28
// cells, 252 lanes; 3-D: 9 cells, 243 lanes), the node of lane t read through conn[cell * NN + a_of_t[t]].  x_e, the point values f of both
// rules, the corners and the tables sit in LDS (3-D: 420 doubles per cell).  The sum factorisation runs IN THE LANE (x-contraction per node
// line, then the two other axes): at three nodes per axis the work repeated between the lanes of a cell costs less than the barrier per
// contracted axis that a factorisation shared through LDS needs -- four barriers per group of cells instead of about fifty.
//   1. h3g_cell_kernel    y_e = K_e x_e -> scratch [cell][component][t]                      (imposed DOFs of x read as 0)
//   2. hog_gather_kernel  row = the sum of its node -> (cell, t) incidence entries in ascending order (pyn_matfree_ho_general.hip)
//                                                                                           (imposed rows: y = x; fused p.Ap)
// Every row is written once, no atomics, no zero fill, bit-identical from run to run; the valence of a node is whatever the mesh has.
// Dirichlet: a SNAPSHOT of the per-DOF mask taken by pyn_matfree_set.
#include "pyn_ho_tables.h"

using namespace pyn_ho;

namespace {

constexpr const char* WHAT = "general ngl 3 matrix-free KLE operator";
constexpr int OP = PYN_MATFREE_KLE_NGL3_GENERAL;

struct H3gArgs {
  const int32_t* conn;     // [n_cells][NN]
  const double* xyz;
  const uint8_t* mask;     // [n_node][DIM] snapshot of the Dirichlet mask, null = nothing imposed
  const double* tab;       // H3gTab::packed
  const int32_t* aoft;     // [NN] local node at tensor position t
  double* ye;              // [n_cells][DIM][NN] per-cell results
  int n_cells;
  double alpha_d, alpha_w;
};

// the 1-D tables: Gauss(3) full rule and Gauss(2) reduced rule on the Lobatto(3) nodes.  packed: wf[3] Bf[3][3] Gf[3][3] wr[2] Br[2][3]
// Gr[2][3] xf[3] xr[2]; the points last, full rule first, as hog_det_kernel reads them
struct H3gTab {
  std::vector<double> xl, xf, wf, Bf, Gf, xr, wr, Br, Gr;
  static constexpr int WF = 0, BF = 3, GF = 12, WR = 21, BR = 23, GR = 29, XF = 35, XR = 38, SIZE = 40;
  H3gTab() : xl(3), xf(3), wf(3), Bf(9), Gf(9), xr(2), wr(2), Br(6), Gr(6) {
    std::vector<double> wl(3);
    lobatto_rule(3, xl.data(), wl.data());
    gauss_rule(3, xf.data(), wf.data());
    gauss_rule(2, xr.data(), wr.data());
    lagrange_1d(3, xl.data(), 3, xf.data(), Bf.data(), Gf.data());
    lagrange_1d(3, xl.data(), 2, xr.data(), Br.data(), Gr.data());
  }
  std::vector<double> packed() const {
    std::vector<double> t;
    for (const auto* v : {&wf, &Bf, &Gf, &wr, &Br, &Gr, &xf, &xr}) t.insert(t.end(), v->begin(), v->end());
    return t;
  }
};

template <int DIM>
struct H3gCfg : HoCfg<DIM, 3> {
  using B = HoCfg<DIM, 3>;
  static constexpr int NC = 1 << DIM;
  static constexpr int CORN = NC * DIM;
  static constexpr int XS = DIM * B::NN;              // x_e [DIM][NN]
  static constexpr int FF = DIM * DIM * B::NN;        // full rule: f [p][r][point]
  static constexpr int FR = DIM * DIM * B::NPT;       // reduced rule: g [q][r][point], then f [p][r][point] in its place
  static constexpr int CELL_LDS = XS + FF + FR + CORN;
  static constexpr int TAB = H3gTab::SIZE;
  static_assert((size_t)(B::CPB * CELL_LDS + TAB) * sizeof(double) <= 65536, "static LDS");
  static_assert(CORN <= B::NN && DIM * B::NPT <= B::NN, "one lane per corner coordinate / per (component, reduced point)");
  static_assert(B::BLOCK == 256, "the kernel is launched with 256 lanes");
};

// Reference gradient g[r] of one component at the point (qi, qj, qk) of an NQ^DIM rule with the 1-D bases B, G [NQ][3] from its nodal
// values v[NN] (LDS): sum factorisation IN THE LANE -- the x-contraction per node line, then the products of the two other axes.  With
// three nodes per axis the redundant work between the lanes of a cell is cheaper than a barrier per axis.
template <int DIM>
__device__ __forceinline__ void h3g_grad_at(const double* v, const double* B, const double* G, int qi, int qj, int qk, double (&g)[DIM]) {
  constexpr int N = 3;
  double bx[N], gx[N];
#pragma unroll
  for (int a = 0; a < N; ++a) {
    bx[a] = B[qi * N + a];
    gx[a] = G[qi * N + a];
  }
#pragma unroll
  for (int r = 0; r < DIM; ++r) g[r] = 0.0;
#pragma unroll
  for (int c = 0; c < (DIM == 3 ? N : 1); ++c) {
    const double bz = DIM == 3 ? B[qk * N + c] : 1.0, gz = DIM == 3 ? G[qk * N + c] : 0.0;
#pragma unroll
    for (int b = 0; b < N; ++b) {
      const double by = B[qj * N + b], gy = G[qj * N + b];
      const double* ln = v + N * (b + N * c);
      const double sb = fma(bx[2], ln[2], fma(bx[1], ln[1], bx[0] * ln[0]));
      const double sg = fma(gx[2], ln[2], fma(gx[1], ln[1], gx[0] * ln[0]));
      g[0] = fma(by * bz, sg, g[0]);
      g[1] = fma(gy * bz, sb, g[1]);
      if constexpr (DIM == 3) g[2] = fma(by * gz, sb, g[2]);
    }
  }
}

// The transpose at node (ti, tj, tk): sum over the NQ^DIM points of f[r][point] (LDS, [DIM][NPT]) against the test-side bases
template <int DIM, int NQ>
__device__ __forceinline__ double h3g_test_at(const double* f, const double* B, const double* G, int ti, int tj, int tk) {
  constexpr int N = 3, NPT = ipow(NQ, DIM);
  double bx[NQ], gx[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    bx[i] = B[i * N + ti];
    gx[i] = G[i * N + ti];
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < (DIM == 3 ? NQ : 1); ++k) {
    const double bz = DIM == 3 ? B[k * N + tk] : 1.0, gz = DIM == 3 ? G[k * N + tk] : 0.0;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const double by = B[j * N + tj], gy = G[j * N + tj];
      const double* ln = f + NQ * (j + NQ * k);
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        s0 = fma(gx[i], ln[i], s0);
        s1 = fma(bx[i], ln[NPT + i], s1);
        if constexpr (DIM == 3) s2 = fma(bx[i], ln[2 * NPT + i], s2);
      }
      s = fma(by * bz, s0, s);
      s = fma(gy * bz, s1, s);
      if constexpr (DIM == 3) s = fma(by * gz, s2, s);
    }
  }
  return s;
}

// pass 1: y_e = K_e x_e of every cell.  Lane t of a cell = tensor position t (x fastest) = point t of the full rule; lanes
// t < DIM * NPR also take (component t / NPR, reduced point t % NPR) of the reduced rule's forward map, lanes t < NPR its points.
// Four barriers per group of cells: x_e and the corners are in LDS | f of the full rule and g of the reduced rule are | f of the
// reduced rule is | (the next group) everything has been read.
template <int DIM>
__global__ void __launch_bounds__(256) h3g_cell_kernel(H3gArgs A, const double* __restrict__ xin, const int* __restrict__ flag) {
  using C = H3gCfg<DIM>;
  using T = H3gTab;
  constexpr int N = 3, NN = C::NN, NC = C::NC, NPR = C::NPT;   // NPR: points of the reduced rule
  __shared__ double lds[C::CPB * C::CELL_LDS + C::TAB];
  if (flag && flag[0]) return;
  double* tab = lds + C::CPB * C::CELL_LDS;
  const double *wf = tab + T::WF, *Bf = tab + T::BF, *Gf = tab + T::GF, *wr = tab + T::WR, *Br = tab + T::BR, *Gr = tab + T::GR;
  const double *xf = tab + T::XF, *xr = tab + T::XR;
  for (int i = threadIdx.x; i < C::TAB; i += 256) tab[i] = A.tab[i];
  const int slot = threadIdx.x / NN, t = threadIdx.x - slot * NN;
  double* xs = lds + (slot < C::CPB ? slot : 0) * C::CELL_LDS;   // [DIM][NN]
  double* ff = xs + C::XS;      // [DIM][DIM][NN]
  double* fr = ff + C::FF;      // [DIM][DIM][NPR]
  double* Xc = fr + C::FR;      // [NC][DIM] corner coordinates, corner = lattice bits
  const int ti = t % N, tj = (t / N) % N, tk = DIM == 3 ? t / (N * N) : 0;
  const int a_t = A.aoft[t];
  const int n_groups = (A.n_cells + C::CPB - 1) / C::CPB;
  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int cell = grp * C::CPB + slot;
    const bool act = slot < C::CPB && cell < A.n_cells;
    __syncthreads();   // the tables; the previous group's buffers
    if (act) {
      const int32_t* cn = A.conn + (int64_t)cell * NN;
      {   // this lane's node of x_e, imposed DOFs as 0
        const int64_t node = cn[a_t];
#pragma unroll
        for (int q = 0; q < DIM; ++q) {
          const bool imp = A.mask && A.mask[node * DIM + q];
          xs[q * NN + t] = imp ? 0.0 : xin[node * DIM + q];
        }
      }
      if (t < NC * DIM) {   // the corners: one coordinate per lane
        const int b = t / DIM, x = t - b * DIM;
        const int tc = (N - 1) * ((b & 1) + N * (((b >> 1) & 1) + (DIM == 3 ? N * ((b >> 2) & 1) : 0)));
        const int64_t node = cn[A.aoft[tc]];
        Xc[t] = A.xyz[node * DIM + x];
      }
    }
    __syncthreads();
    if (act) {
      // ---- full rule, forward: Qd = w detJ Ji^T Ji at this lane's Gauss(3) point (Ji[x][r] = d(xi_r) / dx, rows = physical axes),
      //      f[p][r] = sum_s Qd[r][s] g_p[s]
      double Qd[DIM][DIM], Ji[DIM][DIM];
      const double xq[3] = {xf[ti], xf[tj], DIM == 3 ? xf[tk] : 0.0};
      const double wd = hog_jac_inv<DIM>(Xc, xq, Ji) * wf[ti] * wf[tj] * (DIM == 3 ? wf[tk] : 1.0);
#pragma unroll
      for (int r = 0; r < DIM; ++r)
#pragma unroll
        for (int s = 0; s < DIM; ++s) {
          double q = 0.0;
#pragma unroll
          for (int d = 0; d < DIM; ++d) q = fma(Ji[d][r], Ji[d][s], q);
          Qd[r][s] = wd * q;
        }
#pragma unroll
      for (int p = 0; p < DIM; ++p) {
        double g[DIM];
        h3g_grad_at<DIM>(xs + p * NN, Bf, Gf, ti, tj, tk, g);
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
          double s = 0.0;
#pragma unroll
          for (int sx = 0; sx < DIM; ++sx) s = fma(Qd[r][sx], g[sx], s);
          ff[(p * DIM + r) * NN + t] = s;
        }
      }
      // ---- reduced rule, forward: reference gradient of component t / NPR at the Gauss(2) point t % NPR
      if (t < DIM * NPR) {
        const int q = t / NPR, pt = t - q * NPR;
        double g[DIM];
        h3g_grad_at<DIM>(xs + q * NN, Br, Gr, pt % 2, (pt / 2) % 2, DIM == 3 ? pt / 4 : 0, g);
#pragma unroll
        for (int r = 0; r < DIM; ++r) fr[(q * DIM + r) * NPR + pt] = g[r];
      }
    }
    __syncthreads();
    // ---- at the reduced point (lanes t < NPR): D[q][d] = d u_q / d x_d, W[d][p] = alpha_d tr(D) [d == p] + alpha_w (D[p][d] - D[d][p]),
    //      f[p][r] = w detJ sum_d Ji[d][r] W[d][p], written over this point's g (no other lane reads that column)
    if (act && t < NPR) {
      const int qi = t % 2, qj = (t / 2) % 2, qk = DIM == 3 ? t / 4 : 0;
      double g[DIM][DIM], Ji[DIM][DIM];
#pragma unroll
      for (int q = 0; q < DIM; ++q)
#pragma unroll
        for (int r = 0; r < DIM; ++r) g[q][r] = fr[(q * DIM + r) * NPR + t];
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
          fr[(p * DIM + r) * NPR + t] = s;
        }
      }
    }
    // ---- full rule, backward
    double y[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) y[p] = act ? h3g_test_at<DIM, 3>(ff + p * DIM * NN, Bf, Gf, ti, tj, tk) : 0.0;
    __syncthreads();
    // ---- reduced rule, backward
    if (act) {
#pragma unroll
      for (int p = 0; p < DIM; ++p) {
        y[p] += h3g_test_at<DIM, 2>(fr + p * DIM * NPR, Br, Gr, ti, tj, tk);
        A.ye[((int64_t)cell * DIM + p) * NN + t] = y[p];
      }
    }
  }
}

template <int DIM>
int launch_h3g_cells(pyn_ctx* c, const H3gArgs& A, const double* x, const int* flag) {
  using C = H3gCfg<DIM>;
  const int n_groups = (A.n_cells + C::CPB - 1) / C::CPB;
  const int grid = std::min(n_groups, 256 * 8);
  if (grid == 0) return PYN_OK;
  h3g_cell_kernel<DIM><<<grid, 256, 0, c->stream>>>(A, x, flag);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

H3gArgs h3g_args(const pyn_ctx* c) {
  H3gArgs A;
  A.conn = c->d_conn;
  A.xyz = c->d_xyz;
  A.mask = c->mf_mask[OP];
  A.tab = c->h3g.tab;
  A.aoft = c->h3g.aoft;
  A.ye = c->h3g.ye;
  A.n_cells = (int)c->n_elem;
  A.alpha_d = c->mf_alpha_d[OP];
  A.alpha_w = c->mf_alpha_w[OP];
  return A;
}

// the uploaded rules (reference order of points and nodes) against the tensor products of the 1-D tables: the Gauss(3) full rule and the
// Gauss(2) reduced rule on the Lobatto(3) nodes
int h3g_check_rules(pyn_ctx* c, const H3gTab& T) {
  const int dim = c->dim, nn = c->nn;
  std::vector<int> ln;
  ref_local_lattice(3, dim, ln);
  double worst = 0.0;
  for (int q = 0; q < 2; ++q) {
    const int n = q ? 2 : 3;
    int npt = 1;
    for (int d = 0; d < dim; ++d) npt *= n;
    PYN_CHECK(c->quad[q].ngp == npt && c->quad[q].H && c->quad[q].w,
              "%s: needs the tables of the Gauss(3) full rule and the Gauss(2) reduced rule (pyn_elem_tables_set)", WHAT);
    const std::vector<double>&w1 = q ? T.wr : T.wf, &B1 = q ? T.Br : T.Bf;
    std::vector<double> w((size_t)npt), H((size_t)npt * nn);
    PYN_HIP(hipMemcpy(w.data(), c->quad[q].w, w.size() * sizeof(double), hipMemcpyDeviceToHost));
    PYN_HIP(hipMemcpy(H.data(), c->quad[q].H, H.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> lp;
    ref_local_lattice(n, dim, lp);
    for (int g = 0; g < npt; ++g) {
      double wt = 1.0;
      for (int d = 0; d < dim; ++d) wt *= w1[lp[g * dim + d]];
      worst = std::max(worst, std::fabs(w[g] - wt));
      for (int a = 0; a < nn; ++a) {
        double hv = 1.0;
        for (int d = 0; d < dim; ++d) hv *= B1[(size_t)lp[g * dim + d] * 3 + ln[a * dim + d]];
        worst = std::max(worst, std::fabs(H[(size_t)g * nn + a] - hv));
      }
    }
  }
  PYN_CHECK(worst <= 1e-11, "%s: the element tables are not those of the Gauss(3) full rule and the Gauss(2) reduced rule on the "
                            "Lobatto(3) nodes (largest difference %.3e)", WHAT, worst);
  return PYN_OK;
}

// pyn_matfree_set(PYN_MATFREE_KLE_NGL3_GENERAL): the refusals, the tables, a_of_t, the sign of det J everywhere, the incidence list
int h3g_set(pyn_ctx* c, int op) {
  PYN_CHECK(op == OP, "%s: serves PYN_MATFREE_KLE_NGL3_GENERAL only (operator %d asked for)", WHAT, op);
  const int dim = c->dim, nn = c->nn;
  PYN_CHECK(c->n_elem > 0 && (dim == 2 || dim == 3) && c->ngl == 3 && nn == (dim == 2 ? 9 : 27) && c->nc == (1 << dim),
            "%s: serves quadrilateral (9-node) / hexahedral (27-node) meshes of order ngl 3; this mesh has ngl %d and %d nodes per cell "
            "(orders ngl >= 4: PYN_MATFREE_KLE_GENERAL)", WHAT, c->ngl, nn);
  PYN_CHECK(c->nranks == 1 && !c->detached && c->n_ghost == 0 && c->n_owned == c->n_node,
            "%s: runs on one rank (this context: %d ranks, %lld ghost nodes)", WHAT, c->nranks, (long long)c->n_ghost);
  PYN_CHECK(c->n_elem * (int64_t)nn < ((int64_t)1 << 31), "%s: %lld cells of %d nodes: the incidence list needs n_elem * nn < 2^31", WHAT,
            (long long)c->n_elem, nn);
  PYN_HIP(hipSetDevice(c->device));
  const H3gTab T;
  PYN_TRY(h3g_check_rules(c, T));
  PYN_TRY(pyn_hog_check_geometry_tables(c, T.xf, T.xr, WHAT));
  c->h3g = H3gState();
  c->mf_set[OP] = false;
  // built here, committed together at the end: a refused set leaves nothing behind
  DevBuf<double> d_tab, d_ye;
  DevBuf<int32_t> d_aoft, d_inc_ptr, d_inc;
  const std::vector<double> packed = T.packed();
  PYN_HIP(d_tab.alloc(packed.size()));
  PYN_HIP(hipMemcpy(d_tab, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice));
  std::vector<int32_t> aoft;
  pyn_hog_aoft(3, dim, aoft);
  PYN_HIP(d_aoft.alloc((size_t)nn));
  PYN_HIP(hipMemcpy(d_aoft, aoft.data(), (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice));
  PYN_TRY(pyn_hog_check_det(c, d_aoft, d_tab, H3gTab::XF, WHAT, "a point of the Gauss(3) or of the Gauss(2) rule"));
  PYN_TRY(pyn_hog_incidence(c, aoft, WHAT, d_inc_ptr, d_inc));
  PYN_HIP(d_ye.alloc((size_t)c->n_elem * nn * dim));
  c->h3g.tab = std::move(d_tab);
  c->h3g.ye = std::move(d_ye);
  c->h3g.aoft = std::move(d_aoft);
  c->h3g.inc_ptr = std::move(d_inc_ptr);
  c->h3g.inc = std::move(d_inc);
  return PYN_OK;
}

// y = K x under the mask snapshot of pyn_matfree_set.  dot: fused p.Ap partials into c->d_part (one per workgroup of the gather pass,
// *grid_out of them).
int h3g_spmv(pyn_ctx* c, int op, const double* x, double* y, bool dot, int* grid_out) {
  PYN_CHECK(op == OP && c->mf_set[OP] && c->h3g.tab && c->h3g.ye && c->h3g.aoft && c->h3g.inc_ptr && c->h3g.inc,
            "%s: pyn_matfree_set first", WHAT);
  const H3gArgs A = h3g_args(c);
  const int* flag = dot ? c->d_flag : nullptr;
  if (c->dim == 3)
    PYN_TRY(launch_h3g_cells<3>(c, A, x, flag));
  else
    PYN_TRY(launch_h3g_cells<2>(c, A, x, flag));
  return pyn_hog_gather(c, c->h3g.inc_ptr, c->h3g.inc, A.ye, A.mask, x, y, dot, grid_out);
}

bool h3g_mesh(const pyn_ctx*) { return false; }   // never chosen by the mesh: the operator id selects this backend
int h3g_bs(const pyn_ctx* c, int) { return c->dim; }

}  // namespace

const MfBackend* pyn_mf_h3g() {
  static const MfBackend b = {h3g_mesh, h3g_set, h3g_bs, h3g_spmv, nullptr};
  return &b;
}
