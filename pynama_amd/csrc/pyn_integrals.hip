// Mesh integrals: the moments of a nodal field over any quadrilateral / hexahedral mesh of order 2 <= ngl <= pyn_ho_matfree_max_ngl(dim),
// one rank: volume, int u_c, int u_c^2 and, on request, int |grad u_c|^2, int (div u)^2, int (curl u)_k^2 of u = a or u = a - b.
//
// Scheme: the field of a cell is its own tensor Lagrange interpolant on the Lobatto(ngl) nodes; the geometry is the multilinear image
// of the cell's 2^dim corners (the first 2^dim entries of its connectivity row), J formed at every quadrature point (hog_jac_inv), in
// the LATTICE orientation of the general matrix-free shells (a_of_t, the inverse of mesh_local_lattice: a rotation of the reference
// axes, which no integral sees).  Two rules:
//   PYN_RULE_NODAL  the Lobatto(ngl) nodes themselves (collocation: the reference's lumped weights).  One lane per node, the value is
//                   the nodal value, the reference gradient comes from the collocation derivative table.
//   PYN_RULE_GAUSS  Gauss-Legendre with ngl + 1 points per axis: u^2 det J has degree <= 2 ngl per axis, so volume, value and square
//                   are exact on every multilinear cell, the gradient moments on affine cells.  One lane per point; values and
//                   reference derivatives by sum factorisation along one axis at a time through LDS.
//
// Mapping: a cell owns LP lanes, LP = the points of the rule rounded up to a power of two (<= 64) or to whole waves, so that a cell is
// an aligned piece of a wave or a run of whole waves wherever it sits; CPB cells per workgroup.  The components of the vector are
// walked one after the other (the block size is a run-time loop: the library carries one kernel per (dim, ngl, grad, rule), 72 in
// all), each through the same LDS stages.
//
// Reduction, no floating-point atomics:
//   cell    every quantity is summed over the cell's lanes by a fixed tree (cell_tree: two shuffles across the halves of a wave, then
//           DPP row moves inside 16 lanes, which cost no LDS traffic), then over its waves in ascending order: a function of the
//           cell alone
//   chunk   CHUNK = 16 CPB consecutive cells are accumulated in cell order by one workgroup: part[quantity][chunk]
//   mesh    a one-workgroup kernel sums the chunk partials: lane t takes chunks t, t + 256, ... in order, then a fixed LDS tree
// The result is a function of the mesh, the vectors and these constants; the grid (capped by PYNAMA_INTEGRATE_MAX_GRID, read at
// every call) only says which workgroup computes which chunk.
#include <climits>
#include <cstdlib>

#include "pyn_ho_tables.h"

using namespace pyn_ho;

namespace {

constexpr int INT_NQTY = 24;          // stride of a row of quantities: 1 + 3 * 6 + 1 + 3 = 23 at most
constexpr int INT_GROUPS = 16;        // groups of CPB cells per chunk
constexpr int INT_NO_BAD = 0x7f7f7f7f;

constexpr int pow2_ceil(int n) { return n <= 1 ? 1 : 2 * pow2_ceil((n + 1) / 2); }

template <int DIM, int N, int RULE>
struct IntCfg {
  static constexpr bool GAUSS = RULE == PYN_RULE_GAUSS;
  static constexpr int NQ = GAUSS ? N + 1 : N;                           // points per axis
  static constexpr int NN = ipow(N, DIM), NPT = ipow(NQ, DIM);
  static constexpr int LP = NPT <= 64 ? pow2_ceil(NPT) : (NPT + 63) / 64 * 64;   // lanes of a cell
  static constexpr int CPB = LP >= 256 ? 1 : 256 / LP;                   // cells per workgroup
  static constexpr int BLOCK = CPB * LP;
  static constexpr int WPC = LP <= 64 ? 1 : LP / 64;                     // waves of a cell
  static constexpr int CHUNK = INT_GROUPS * CPB;                         // cells per partial
  static constexpr int S1 = GAUSS ? NQ * ipow(N, DIM - 1) : 0;           // items of the first stage
  static constexpr int S2 = GAUSS && DIM == 3 ? NQ * NQ * N : 0;         // ... of the second (3-D)
  static constexpr int NC = 1 << DIM, CORN = NC * DIM;
  static constexpr int CELL_LDS = NN + 2 * S1 + 3 * S2 + CORN + WPC * INT_NQTY;
  static constexpr int TAB = 2 * NQ + 2 * NQ * N;                        // w[NQ] x[NQ] B[NQ][N] G[NQ][N]
  static_assert((size_t)(CPB * CELL_LDS + TAB) * sizeof(double) <= 65536, "static LDS");
  static_assert(BLOCK <= 1024 && BLOCK >= INT_NQTY && BLOCK % 64 == 0, "workgroup size");
  static_assert(S1 <= LP && S2 <= LP && NN <= LP, "one lane per item of every stage");
};

struct IntArgs {
  const int32_t* conn;     // [n_cells][NN]
  const double* xyz;
  const double* tab;       // w x B G of the rule (IntCfg::TAB)
  const int32_t* aoft;     // [NN] local node at tensor position t
  const double* a;
  const double* b;         // null: u = a
  double* part;            // [quantity][n_chunks]
  int* bad;                // lowest cell with det J <= 0 at a point
  int n_cells, bs;
};

// a double moved between the lanes of a row of 16 by a DPP control word (row_mirror 0x140, row_half_mirror 0x141, quad_perm): two
// vector moves, no LDS traffic; every lane is active wherever this is called
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// sum over the lanes of a cell in one wave, a fixed tree: across the halves of 32 and 16 lanes by shuffles, then inside a row of 16
// lanes i + (15 - i), i + (7 - i), i + (3 - i), i + (i ^ 1).  Every lane of the cell's aligned piece of the wave ends with the sum;
// lanes 0 of the cell's waves hold their wave's share (one wave: the cell's sum)
template <int LP>
__device__ __forceinline__ double cell_tree(double v) {
  constexpr int W = LP < 64 ? LP : 64;
  static_assert(W >= 4, "a cell has at least 2^2 points");
  if constexpr (W >= 64) v += __shfl_xor(v, 32, 64);
  if constexpr (W >= 32) v += __shfl_xor(v, 16, 64);
  if constexpr (W >= 16) v += dpp_f64<0x140>(v);
  if constexpr (W >= 8) v += dpp_f64<0x141>(v);
  v += dpp_f64<0x1B>(v);
  v += dpp_f64<0xB1>(v);
  return v;
}

template <int DIM, int N, int GRAD, int RULE>
__global__ void __launch_bounds__((IntCfg<DIM, N, RULE>::BLOCK)) integrate_kernel(IntArgs A) {
  using C = IntCfg<DIM, N, RULE>;
  constexpr int NQ = C::NQ, NN = C::NN, NPT = C::NPT, LP = C::LP, S1 = C::S1, S2 = C::S2;
  constexpr int WL = LP < 64 ? LP : 64;   // lanes of a cell in one wave
  __shared__ double lds[C::CPB * C::CELL_LDS + C::TAB];
  double* tab = lds + C::CPB * C::CELL_LDS;
  const double* wq = tab;
  const double* xq = wq + NQ;
  const double* Bq = xq + NQ;             // Bq[q * N + a] = h_a(x_q)
  const double* Gq = Bq + NQ * N;         // Gq[q * N + a] = h_a'(x_q)
  for (int i = threadIdx.x; i < C::TAB; i += C::BLOCK) tab[i] = A.tab[i];
  const int slot = threadIdx.x / LP, t = threadIdx.x - slot * LP;
  double* xs = lds + slot * C::CELL_LDS;  // [NN] one component of u_e, tensor order
  double* bufA = xs + NN;
  double* bufB = bufA + 2 * S1;
  double* Xc = bufB + 3 * S2;             // [NC][DIM] corner coordinates, corner = lattice bits
  double* cq = Xc + C::CORN;              // [WPC][INT_NQTY] the cell's sums, per wave
  (void)bufA;
  (void)bufB;
  const int qi = t % NQ, qj = (t / NQ) % NQ, qk = DIM == 3 ? t / (NQ * NQ) : 0;
  const int a_t = t < NN ? A.aoft[t] : 0;
  const int bs = A.bs;
  const bool vecq = GRAD && bs == DIM;    // div and curl
  const int nq = 1 + (GRAD ? 3 : 2) * bs + (vecq ? 1 + (DIM == 3 ? 3 : 1) : 0);
  const int n_chunks = (A.n_cells + C::CHUNK - 1) / C::CHUNK;
  const bool head = (t & (WL - 1)) == 0;  // lane 0 of each of the cell's waves
  double* cqw = cq + (t >> 6) * INT_NQTY;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    double acc = 0.0;                     // thread q < nq: quantity q over the chunk's cells, in cell order
    for (int g = 0; g < INT_GROUPS; ++g) {
      const int base = chunk * C::CHUNK + g * C::CPB;
      if (base >= A.n_cells) break;
      const int cell = base + slot;
      const bool act = cell < A.n_cells;
      const bool pt = act && t < NPT;
      __syncthreads();   // the tables; the previous group's sums and buffers
      int64_t node = 0;
      if (act) {
        const int32_t* cn = A.conn + (int64_t)cell * NN;
        if (t < NN) node = cn[a_t];
        for (int i = t; i < C::CORN; i += LP) {
          const int b = i / DIM, x = i - b * DIM;
          const int tc = (N - 1) * ((b & 1) + N * (((b >> 1) & 1) + (DIM == 3 ? N * ((b >> 2) & 1) : 0)));
          Xc[i] = A.xyz[(int64_t)cn[A.aoft[tc]] * DIM + x];
        }
      }
      __syncthreads();
      // ---- geometry at this lane's point: Ji[x][r] = d xi_r / d x, wd = w det J
      double Ji[DIM][DIM], wd = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d)
#pragma unroll
        for (int r = 0; r < DIM; ++r) Ji[d][r] = 0.0;
      if (pt) {
        const double xi[3] = {xq[qi], xq[qj], DIM == 3 ? xq[qk] : 0.0};
        const double det = hog_jac_inv<DIM>((const double*)Xc, xi, Ji);
        if (!(det > 0.0)) atomicMin(A.bad, cell);
        wd = wq[qi] * wq[qj] * (DIM == 3 ? wq[qk] : 1.0) * det;
      }
      {
        const double s = cell_tree<LP>(wd);
        if (head) cqw[0] = s;
      }
      double dv = 0.0, cw[3] = {0.0, 0.0, 0.0};
      for (int c = 0; c < bs; ++c) {
        if (act && t < NN) {
          double v = A.a[node * bs + c];
          if (A.b) v = v - A.b[node * bs + c];   // the difference first, one rounding
          xs[t] = v;
        }
        __syncthreads();
        double val = 0.0, gr[DIM];
#pragma unroll
        for (int r = 0; r < DIM; ++r) gr[r] = 0.0;
        if constexpr (!C::GAUSS) {
          if (pt) {
            val = xs[t];
            if constexpr (GRAD) {
#pragma unroll
              for (int a = 0; a < N; ++a) {
                gr[0] = fma(Gq[qi * N + a], xs[a + N * (qj + N * qk)], gr[0]);
                gr[1] = fma(Gq[qj * N + a], xs[qi + N * (a + N * qk)], gr[1]);
                if constexpr (DIM == 3) gr[2] = fma(Gq[qk * N + a], xs[qi + N * (qj + N * a)], gr[2]);
              }
            }
          }
          __syncthreads();   // the next component overwrites xs
        } else if constexpr (DIM == 2) {
          if (act && t < S1) {   // (point i, node j)
            const int i1 = t % NQ, j1 = t / NQ;
            double sb = 0.0, sg = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) {
              const double v = xs[a + N * j1];
              sb = fma(Bq[i1 * N + a], v, sb);
              if constexpr (GRAD) sg = fma(Gq[i1 * N + a], v, sg);
            }
            bufA[t] = sb;
            if constexpr (GRAD) bufA[S1 + t] = sg;
          }
          __syncthreads();
          if (pt) {
#pragma unroll
            for (int b = 0; b < N; ++b) {
              val = fma(Bq[qj * N + b], bufA[qi + NQ * b], val);
              if constexpr (GRAD) {
                gr[0] = fma(Bq[qj * N + b], bufA[S1 + qi + NQ * b], gr[0]);
                gr[1] = fma(Gq[qj * N + b], bufA[qi + NQ * b], gr[1]);
              }
            }
          }
        } else {
          if (act && t < S1) {   // (point i, node j, node k)
            const int i1 = t % NQ, r1 = t / NQ;
            double sb = 0.0, sg = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) {
              const double v = xs[a + N * r1];
              sb = fma(Bq[i1 * N + a], v, sb);
              if constexpr (GRAD) sg = fma(Gq[i1 * N + a], v, sg);
            }
            bufA[t] = sb;
            if constexpr (GRAD) bufA[S1 + t] = sg;
          }
          __syncthreads();
          if (act && t < S2) {   // (point i, point j, node k)
            const int i2 = t % NQ, j2 = (t / NQ) % NQ, k2 = t / (NQ * NQ);
            double bb = 0.0, gb = 0.0, bg = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) {
              const double vb = bufA[i2 + NQ * (b + N * k2)];
              bb = fma(Bq[j2 * N + b], vb, bb);
              if constexpr (GRAD) {
                gb = fma(Bq[j2 * N + b], bufA[S1 + i2 + NQ * (b + N * k2)], gb);
                bg = fma(Gq[j2 * N + b], vb, bg);
              }
            }
            bufB[t] = bb;
            if constexpr (GRAD) {
              bufB[S2 + t] = gb;
              bufB[2 * S2 + t] = bg;
            }
          }
          __syncthreads();
          if (pt) {
#pragma unroll
            for (int k = 0; k < N; ++k) {
              const int o = qi + NQ * (qj + NQ * k);
              val = fma(Bq[qk * N + k], bufB[o], val);
              if constexpr (GRAD) {
                gr[0] = fma(Bq[qk * N + k], bufB[S2 + o], gr[0]);
                gr[1] = fma(Bq[qk * N + k], bufB[2 * S2 + o], gr[1]);
                gr[2] = fma(Gq[qk * N + k], bufB[o], gr[2]);
              }
            }
          }
        }
        // ---- this component's moments (lanes without a point carry wd = 0 and zeros)
        const double wv = wd * val;
        double s = cell_tree<LP>(wv);
        if (head) cqw[1 + c] = s;
        s = cell_tree<LP>(wv * val);
        if (head) cqw[1 + bs + c] = s;
        if constexpr (GRAD) {
          double D[DIM], g2 = 0.0;   // D[d] = d u_c / d x_d
#pragma unroll
          for (int d = 0; d < DIM; ++d) {
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < DIM; ++r) q = fma(Ji[d][r], gr[r], q);
            D[d] = q;
            g2 = fma(q, q, g2);
          }
          s = cell_tree<LP>(wd * g2);
          if (head) cqw[1 + 2 * bs + c] = s;
          if (vecq) {   // div u = sum_c D_c[c]; curl u in the order and sign of the reference's curl rows
            if constexpr (DIM == 2) {
              if (c == 0) {
                dv += D[0];
                cw[0] -= D[1];
              } else {
                dv += D[1];
                cw[0] += D[0];
              }
            } else {
              if (c == 0) {
                dv += D[0];
                cw[1] += D[2];
                cw[2] -= D[1];
              } else if (c == 1) {
                dv += D[1];
                cw[0] -= D[2];
                cw[2] += D[0];
              } else {
                dv += D[2];
                cw[0] += D[1];
                cw[1] -= D[0];
              }
            }
          }
        }
      }
      if constexpr (GRAD) {
        if (vecq) {
          double s = cell_tree<LP>(wd * dv * dv);
          if (head) cqw[1 + 3 * bs] = s;
#pragma unroll
          for (int k = 0; k < (DIM == 3 ? 3 : 1); ++k) {
            s = cell_tree<LP>(wd * cw[k] * cw[k]);
            if (head) cqw[2 + 3 * bs + k] = s;
          }
        }
      }
      __syncthreads();
      if ((int)threadIdx.x < nq) {   // the group's cells in order, each the sum of its waves in order
        for (int sl = 0; sl < C::CPB && base + sl < A.n_cells; ++sl) {
          const double* q = lds + sl * C::CELL_LDS + (C::CELL_LDS - C::WPC * INT_NQTY) + threadIdx.x;
          double cs = q[0];
#pragma unroll
          for (int w = 1; w < C::WPC; ++w) cs += q[w * INT_NQTY];
          acc += cs;
        }
      }
    }
    if ((int)threadIdx.x < nq) A.part[(int64_t)threadIdx.x * n_chunks + chunk] = acc;
  }
}

// the chunk partials of every quantity: lane t sums chunks t, t + 256, ... in order, then a fixed tree
__global__ void __launch_bounds__(256) integrate_sum_kernel(const double* __restrict__ part, int n_chunks, int nq, double* __restrict__ out) {
  __shared__ double sm[256];
  for (int q = 0; q < nq; ++q) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += 256) s += part[(int64_t)q * n_chunks + i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[q] = sm[0];
    __syncthreads();
  }
}

template <int DIM, int N, int GRAD, int RULE>
int integrate_launch(pyn_ctx* c, IntArgs& A, int nq) {
  using C = IntCfg<DIM, N, RULE>;
  const int n_chunks = (A.n_cells + C::CHUNK - 1) / C::CHUNK;
  PYN_HIP(c->d_int_part.grow((size_t)n_chunks * INT_NQTY));
  A.part = c->d_int_part;
  int grid = std::min(n_chunks, 2048);
  if (const char* e = getenv("PYNAMA_INTEGRATE_MAX_GRID")) {
    const int cap = atoi(e);
    if (cap > 0) grid = std::min(grid, cap);
  }
  integrate_kernel<DIM, N, GRAD, RULE><<<grid, C::BLOCK, 0, c->stream>>>(A);
  PYN_HIP(hipGetLastError());
  integrate_sum_kernel<<<1, 256, 0, c->stream>>>(A.part, n_chunks, nq, c->d_int_out);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

template <int DIM, int N>
int integrate_variant(pyn_ctx* c, IntArgs& A, int nq, int grad, int rule) {
  if (rule == PYN_RULE_GAUSS)
    return grad ? integrate_launch<DIM, N, 1, PYN_RULE_GAUSS>(c, A, nq) : integrate_launch<DIM, N, 0, PYN_RULE_GAUSS>(c, A, nq);
  return grad ? integrate_launch<DIM, N, 1, PYN_RULE_NODAL>(c, A, nq) : integrate_launch<DIM, N, 0, PYN_RULE_NODAL>(c, A, nq);
}

int integrate_any(pyn_ctx* c, IntArgs& A, int nq, int grad, int rule) {
  if (c->dim == 2) switch (c->ngl) {
      case 2: return integrate_variant<2, 2>(c, A, nq, grad, rule);
      case 3: return integrate_variant<2, 3>(c, A, nq, grad, rule);
      case 4: return integrate_variant<2, 4>(c, A, nq, grad, rule);
      case 5: return integrate_variant<2, 5>(c, A, nq, grad, rule);
      case 6: return integrate_variant<2, 6>(c, A, nq, grad, rule);
      case 7: return integrate_variant<2, 7>(c, A, nq, grad, rule);
      case 8: return integrate_variant<2, 8>(c, A, nq, grad, rule);
      case 9: return integrate_variant<2, 9>(c, A, nq, grad, rule);
      case 10: return integrate_variant<2, 10>(c, A, nq, grad, rule);
      case 11: return integrate_variant<2, 11>(c, A, nq, grad, rule);
      case 12: return integrate_variant<2, 12>(c, A, nq, grad, rule);
    }
  if (c->dim == 3) switch (c->ngl) {
      case 2: return integrate_variant<3, 2>(c, A, nq, grad, rule);
      case 3: return integrate_variant<3, 3>(c, A, nq, grad, rule);
      case 4: return integrate_variant<3, 4>(c, A, nq, grad, rule);
      case 5: return integrate_variant<3, 5>(c, A, nq, grad, rule);
      case 6: return integrate_variant<3, 6>(c, A, nq, grad, rule);
      case 7: return integrate_variant<3, 7>(c, A, nq, grad, rule);
      case 8: return integrate_variant<3, 8>(c, A, nq, grad, rule);
    }
  pyn_set_error("pyn_integrate: no kernel for dim %d ngl %d", c->dim, c->ngl);
  return PYN_EINVAL;
}

// w x B G of both rules and a_of_t for the context's order and dimension: uploaded on first use, kept until the mesh changes
int integrate_tables(pyn_ctx* c) {
  if (c->int_tab_ngl == c->ngl && c->int_tab_dim == c->dim && c->d_int_tab[0] && c->d_int_tab[1] && c->d_int_aoft && c->d_int_out && c->d_int_bad)
    return PYN_OK;
  const int n = c->ngl;
  std::vector<double> xl((size_t)n), wl((size_t)n);
  lobatto_rule(n, xl.data(), wl.data());
  DevBuf<double> d_tab[2], d_out;
  DevBuf<int32_t> d_aoft;
  DevBuf<int> d_bad;
  for (int rule = 0; rule < 2; ++rule) {
    const int nqp = rule == PYN_RULE_GAUSS ? n + 1 : n;
    std::vector<double> t((size_t)2 * nqp + 2 * nqp * n);
    double* w = t.data();
    double* x = w + nqp;
    if (rule == PYN_RULE_GAUSS) {
      gauss_rule(nqp, x, w);
    } else {
      std::copy(xl.begin(), xl.end(), x);
      std::copy(wl.begin(), wl.end(), w);
    }
    lagrange_1d(n, xl.data(), nqp, x, x + nqp, x + nqp + (size_t)nqp * n);
    PYN_TRY(dev_upload(d_tab[rule], (const double*)t.data(), t.size(), c->stream));
  }
  std::vector<int32_t> aoft;
  pyn_hog_aoft(n, c->dim, aoft);
  PYN_TRY(dev_upload(d_aoft, (const int32_t*)aoft.data(), aoft.size(), c->stream));
  PYN_HIP(d_out.alloc(INT_NQTY));
  PYN_HIP(d_bad.alloc(1));
  PYN_HIP(hipStreamSynchronize(c->stream));   // the host tables leave with this frame
  c->d_int_tab[0] = std::move(d_tab[0]);
  c->d_int_tab[1] = std::move(d_tab[1]);
  c->d_int_aoft = std::move(d_aoft);
  c->d_int_out = std::move(d_out);
  c->d_int_bad = std::move(d_bad);
  c->int_tab_ngl = n;
  c->int_tab_dim = c->dim;
  return PYN_OK;
}

}  // namespace

extern "C" int pyn_integrate_len(int dim, int bs, int with_grad) {
  if ((dim != 2 && dim != 3) || bs < 1 || bs > 6) return 0;
  return 1 + (with_grad ? 3 : 2) * bs + (with_grad && bs == dim ? 1 + (dim == 3 ? 3 : 1) : 0);
}

extern "C" int pyn_integrate(pyn_ctx* c, int rule, int with_grad, int vec_a, int vec_b, double* out, int* n_out) {
  PYN_CHECK(c && out && n_out, "NULL argument");
  PYN_CHECK(c->n_elem > 0 && c->d_conn && c->d_xyz, "pyn_integrate: pyn_mesh_set first");
  const int dim = c->dim, ngl = c->ngl, lim = pyn_ho_matfree_max_ngl(dim);
  PYN_CHECK(rule == PYN_RULE_NODAL || rule == PYN_RULE_GAUSS, "pyn_integrate: unknown rule %d (PYN_RULE_NODAL 0, PYN_RULE_GAUSS 1)", rule);
  PYN_CHECK(c->nn != dim + 1 && ngl >= 2, "pyn_integrate: simplices (nn = %d in %d-D) have no mesh integrals; quadrilaterals and hexahedra only",
            c->nn, dim);
  PYN_CHECK(c->nranks == 1 && !c->detached && c->n_ghost == 0 && c->n_owned == c->n_node,
            "pyn_integrate: mesh integrals run on one rank (this context: %d ranks, %lld ghost nodes)", c->nranks, (long long)c->n_ghost);
  PYN_CHECK(ngl <= lim, "pyn_integrate: ngl %d is above the limit of %d-D meshes (ngl <= %d)", ngl, dim, lim);
  PYN_CHECK((dim == 2 || dim == 3) && c->nn == ipow(ngl, dim) && c->nc == (1 << dim), "pyn_integrate: nn = %d is not ngl^dim = %d^%d", c->nn, ngl,
            dim);
  PYN_CHECK(c->n_elem < (int64_t)INT_NO_BAD, "pyn_integrate: %lld cells do not fit a 32-bit cell index", (long long)c->n_elem);
  PYN_TRY(pyn_check_vec(c, vec_a, "pyn_integrate a"));
  const DVec& va = c->vecs[vec_a];
  PYN_CHECK(va.bs >= 1 && va.bs <= 6, "pyn_integrate: block size %d has no kernel (1 .. 6)", va.bs);
  PYN_CHECK(va.d.size() == (size_t)c->n_node * va.bs, "pyn_integrate: the vector holds %lld nodes, the mesh has %lld",
            (long long)(va.d.size() / (size_t)va.bs), (long long)c->n_node);
  const double* db = nullptr;
  if (vec_b >= 0) {
    PYN_TRY(pyn_check_vec(c, vec_b, "pyn_integrate b"));
    const DVec& vb = c->vecs[vec_b];
    PYN_CHECK(vb.bs == va.bs, "pyn_integrate: vec_b has block size %d, vec_a has %d", vb.bs, va.bs);
    PYN_CHECK(vb.d.size() == va.d.size(), "pyn_integrate: vec_b holds %lld nodes, the mesh has %lld", (long long)(vb.d.size() / (size_t)vb.bs),
              (long long)c->n_node);
    db = vb.d;
  }
  PYN_HIP(hipSetDevice(c->device));
  PYN_TRY(integrate_tables(c));
  const int grad = with_grad ? 1 : 0, nq = pyn_integrate_len(dim, va.bs, grad);
  IntArgs A;
  A.conn = c->d_conn;
  A.xyz = c->d_xyz;
  A.tab = c->d_int_tab[rule];
  A.aoft = c->d_int_aoft;
  A.a = va.d;
  A.b = db;
  A.part = nullptr;
  A.bad = c->d_int_bad;
  A.n_cells = (int)c->n_elem;
  A.bs = va.bs;
  PYN_HIP(hipMemsetAsync(c->d_int_bad, 0x7f, sizeof(int), c->stream));
  PYN_HIP(hipEventRecord(c->ev0, c->stream));
  PYN_TRY(integrate_any(c, A, nq, grad, rule));
  PYN_HIP(hipEventRecord(c->ev1, c->stream));
  double res[INT_NQTY];
  int bad = INT_NO_BAD;
  PYN_HIP(hipMemcpyAsync(res, c->d_int_out, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipMemcpyAsync(&bad, c->d_int_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  float ms = 0;
  PYN_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->timers[PYN_T_INTEGRATE] = ms;
  PYN_CHECK(bad == INT_NO_BAD, "pyn_integrate: non-positive Jacobian: cell %d has det J <= 0 at a point of the %s rule (inverted or degenerate "
                               "cell, or a connectivity that does not follow the reference's local node order)", bad,
            rule == PYN_RULE_GAUSS ? "Gauss" : "nodal");
  for (int i = 0; i < nq; ++i) out[i] = res[i];
  *n_out = nq;
  return PYN_OK;
}
