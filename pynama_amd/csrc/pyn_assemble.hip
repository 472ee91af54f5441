// Numeric phase (HOT LOOP 1): per-element quadrature + global scatter with Dirichlet elimination.
//
// Reference: Spectral.getElemKLEMatrices (src/elements/spectral.py:89-157) called per cell by
// FreeSlip.buildKLEMats (src/cases/base_problem.py:499-552), then Mat.setIndices2One
// (src/matrices/mat_generator.py:113-118).
//
// Closed forms used by the kernels (derived from the B-matrix products of spectral.py:124-156;
// G = J^-1 Hrs are physical gradients at a point, c = w detJ, eps = Levi-Civita):
//   K [(a,p),(b,q)] = d_pq sum_full c G_a.G_b
//                   + sum_red c ( alpha_d G_pa G_qb + alpha_w ( d_pq G_a.G_b - G_qa G_pb ) )
//   Rw[(a,p),(b,k)] = sum_full c H_a curlsel(p,k;G_b) + sum_red alpha_w c curlsel(k,p;G_a)^T H_b
//   Rd[(a,p), b   ] = -sum_full c H_a G_pb + sum_red alpha_d c G_pa H_b
// where curlsel encodes (curl w)_p = eps_pmk d_m w_k (3D) and (d_y w, -d_x w) (2D).
#include <cstring>

#include "pyn_internal.h"

namespace {

struct AsmArgs {
  // mesh
  const int32_t* conn;
  const double* xyz;
  int64_t n_elem, n_owned;
  int dim, nn, nc;
  // tables: 0 = full, 1 = reduced, 2 = nodal
  int ngp[3];
  const double* w[3];
  const double* H[3];
  const double* Hrs[3];
  const double* HrsCoo[3];
  // graph
  const int32_t* rowptr;
  const int32_t* colidx;
  // bc
  const uint8_t* bcmask;  // may be null
  // form
  int form;
  double alpha_d, alpha_w;
  // outputs (scatter mode) -- null when skipped
  double *K, *Krhs, *Rw, *Rd;
  // no-slip / free-slip split (NoSlipFreeSlip.buildKLEMats, base_problem.py:329-454): DOF classes in
  // bcmask are 0 free, 1 tangential at a no-slip wall (free in the FS solve), 2 imposed in both solves
  double *Kfs, *Krhsfs, *Rwfs, *Rdfs;
  // compact imposed-column targets (pyn_rhs.hip): first block of every owned node row in Krhs / Krhsfs, -1 = row not stored; null = the
  // matrix has the graph's full pattern
  const int32_t *rcrow, *rcrow_fs;
  // element subset (elements with an imposed node: the ones that feed an imposed-column matrix); null = all elements
  const int32_t* esel;
  // dense mode
  const double* corners;  // single element
  double *out0, *out1, *out2;
  // first-order operator form: M[(a,p),(b,q)] = sum_g c_g H_g[a] sum_t [row_t=p, col_t=q] coef_t G_g[der_t][b]
  int op_rule, op_br, op_bc, op_nterms;
  const int32_t* op_terms;  // [nterms][3] = (row comp, col comp, derivative axis)
  const double* op_coef;    // [nterms]
  // scratch for high order
  double* gscratch;
  int64_t gscratch_stride;  // doubles per block
  int ho_chunk;             // > 0: high-order KLE path, Gauss points staged through LDS `ho_chunk` at a time
};

__device__ inline int find_slot(const int32_t* __restrict__ colidx, int lo, int len, int col) {
  // lower_bound over a sorted row; the column is guaranteed to be present
  int l = 0, h = len;
  while (l < h) {
    int m = (l + h) >> 1;
    if (colidx[lo + m] < col)
      l = m + 1;
    else
      h = m;
  }
  return l;
}

__device__ inline double inv_det(const double* J, double* Ji, int dim) {
  if (dim == 2) {
    double det = J[0] * J[3] - J[1] * J[2];
    double r = 1.0 / det;
    Ji[0] = J[3] * r;
    Ji[1] = -J[1] * r;
    Ji[2] = -J[2] * r;
    Ji[3] = J[0] * r;
    return det;
  }
  double c00 = J[4] * J[8] - J[5] * J[7];
  double c01 = J[5] * J[6] - J[3] * J[8];
  double c02 = J[3] * J[7] - J[4] * J[6];
  double det = J[0] * c00 + J[1] * c01 + J[2] * c02;
  double r = 1.0 / det;
  Ji[0] = c00 * r;
  Ji[1] = (J[2] * J[7] - J[1] * J[8]) * r;
  Ji[2] = (J[1] * J[5] - J[2] * J[4]) * r;
  Ji[3] = c01 * r;
  Ji[4] = (J[0] * J[8] - J[2] * J[6]) * r;
  Ji[5] = (J[2] * J[3] - J[0] * J[5]) * r;
  Ji[6] = c02 * r;
  Ji[7] = (J[1] * J[6] - J[0] * J[7]) * r;
  Ji[8] = (J[0] * J[4] - J[1] * J[3]) * r;
  return det;
}

// (curl w)_p = sum_{m,k} cs(p,m,k) d_m w_k ; returns the sign and the derivative index m for (p,k), 0 if none
__device__ inline int curl_term(int dim, int p, int k, int* m) {
  if (dim == 2) {  // w scalar (k = 0): (curl w)_x = d_y w, (curl w)_y = -d_x w
    *m = 1 - p;
    return p == 0 ? 1 : -1;
  }
  if (p == k) return 0;
  *m = 3 - p - k;
  // eps_{p m k}
  return ((m[0] - p + 3) % 3 == 1) ? 1 : -1;
}

// Generic element kernel: one workgroup per element (grid-stride).  All per-point data
// (J^-1, c, G) live in `pt` -- LDS when it fits (PT_LDS), per-block global scratch otherwise.
// v[m] for a runtime m without dynamic register-array indexing (which would put the array in scratch memory)
__device__ __forceinline__ double pick3(const double (&v)[3], int m) { return m == 0 ? v[0] : (m == 1 ? v[1] : v[2]); }

// G_a . G_b over the first `dim` axes, and one reduced-rule point's term of entry (p, q) of a node pair's K block,
// alpha_d G_pa G_qb + alpha_w (d_pq G_a.G_b - G_qa G_pb), with every rounding spelled out.  The per-pair and the staged KLE paths
// both sum their K entries through these two functions and fma(c, term, acc), so that they round alike: with the same sums written
// as plain expressions and fused as the compiler saw fit at each site, the two paths differed in the last bit of a few per cent of
// the diagonal-component entries of a one-cell mesh (tests/test_gpu_generic_forms.py keeps them bit-identical).
__device__ __forceinline__ double gdot(const double (&ga)[3], const double (&gb)[3], int dim) {
  double s = ga[0] * gb[0];
  if (dim > 1) s = fma(ga[1], gb[1], s);
  if (dim > 2) s = fma(ga[2], gb[2], s);
  return s;
}
__device__ __forceinline__ double kle_pen(double ad, double aw, double gap, double gbq, double gaq, double gbp, double s, bool diag) {
  const double pen = fma(ad * gap, gbq, -(aw * gaq * gbp));
  return diag ? fma(aw, s, pen) : pen;
}

template <int BLOCK, bool PT_LDS, bool DENSE>
__global__ void __launch_bounds__(BLOCK) assemble_generic_kernel(AsmArgs A) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int dim = A.dim, nn = A.nn, nc = A.nc;
  const int dd = dim * dim;
  // which rules this form integrates on
  const bool oper = A.form == PYN_FORM_OPERATOR;
  const int qa = oper ? A.op_rule : (A.form == PYN_FORM_MASS_NODAL) ? 2 : 0;  // primary rule
  const bool kle = A.form == PYN_FORM_KLE;
  const int nga = A.ngp[qa];
  const int ngb = kle ? A.ngp[1] : 0;  // reduced rule only for KLE
  const int ngt = nga + ngb;

  double* Xs = reinterpret_cast<double*>(smem_raw);  // [nc*dim]
  int32_t* ids = reinterpret_cast<int32_t*>(Xs + nc * dim);  // [nn] (padded to even)
  double* pt_lds = reinterpret_cast<double*>(ids + ((nn + 1) & ~1));
  const int pt_stride = dd + 1 + dim * nn;  // per point: Jinv[dd], c, G[dim][nn]
  double* pt = PT_LDS ? pt_lds : (A.gscratch + (int64_t)blockIdx.x * A.gscratch_stride);

  const int tid = threadIdx.x;
  const int dw = dim == 2 ? 1 : 3;
  const int64_t e_end = DENSE ? 1 : A.n_elem;

  for (int64_t eq = blockIdx.x; eq < e_end; eq += gridDim.x) {
    const int64_t e = (!DENSE && A.esel) ? A.esel[eq] : eq;
    __syncthreads();
    // ---- gather corners + connectivity
    for (int t = tid; t < nn; t += BLOCK) ids[t] = DENSE ? t : A.conn[e * nn + t];
    for (int t = tid; t < nc * dim; t += BLOCK) {
      if (DENSE) {
        Xs[t] = A.corners[t];
      } else {
        int cn = t / dim, x = t - cn * dim;
        Xs[t] = A.xyz[(int64_t)A.conn[e * nn + cn] * dim + x];
      }
    }
    __syncthreads();
    // ---- geometry at every point: J = HrsCoo.X (spectral.py:120,140), inverse, c = w detJ (:122,142)
    for (int g = tid; g < ngt; g += BLOCK) {
      const int q = g < nga ? qa : 1;
      const int gl = g < nga ? g : g - nga;
      const double* hc = A.HrsCoo[q] + (int64_t)gl * dim * nc;
      double J[9], Ji[9];
      for (int d = 0; d < dim; ++d)
        for (int x = 0; x < dim; ++x) {
          double s = 0.0;
          for (int cn = 0; cn < nc; ++cn) s += hc[d * nc + cn] * Xs[cn * dim + x];
          J[d * dim + x] = s;
        }
      double det = inv_det(J, Ji, dim);
      double* P = pt + (int64_t)g * pt_stride;
      for (int i = 0; i < dd; ++i) P[i] = Ji[i];
      P[dd] = A.w[q][gl] * det;
    }
    __syncthreads();
    // ---- physical gradients G = J^-1 Hrs (spectral.py:121,141)
    for (int t = tid; t < ngt * dim * nn; t += BLOCK) {
      int g = t / (dim * nn);
      int r = t - g * dim * nn;
      int d = r / nn, a = r - d * nn;
      const int q = g < nga ? qa : 1;
      const int gl = g < nga ? g : g - nga;
      const double* hrs = A.Hrs[q] + (int64_t)gl * dim * nn;
      double* P = pt + (int64_t)g * pt_stride;
      double s = 0.0;
      for (int x = 0; x < dim; ++x) s += P[d * dim + x] * hrs[x * nn + a];
      P[dd + 1 + d * nn + a] = s;
    }
    __syncthreads();

    // ---- entries.  ab (node pair) is the fast index so that a thread keeps the same pair
    //      across components when nn*nn is a multiple of BLOCK (Q1 hex: 64 pairs = 64 lanes).
    const int npair = nn * nn;
    int last_ab = -1, slot = 0, r_lo = 0, r_len = 0, r_cr = 0, r_crfs = 0;   // r_cr / r_crfs: row start inside Krhs / Krhsfs
    auto locate = [&](int ab, int a, int b) {
      if (ab != last_ab) {
        last_ab = ab;
        int row = ids[a];
        if (row < A.n_owned) {
          r_lo = A.rowptr[row];
          r_len = A.rowptr[row + 1] - r_lo;
          slot = find_slot(A.colidx, r_lo, r_len, ids[b]);
          r_cr = A.rcrow ? A.rcrow[row] : r_lo;
          r_crfs = A.rcrow_fs ? A.rcrow_fs[row] : r_lo;
        } else {
          r_len = -1;
        }
      }
    };

    if (!PT_LDS && !DENSE && A.ho_chunk > 0) {
      // ---- high-order KLE elements: the point data (pt) sits in global scratch and an entry-per-lane loop re-reads
      //      it nn^2 times.  Here the points go through LDS `CH` at a time and every lane owns a 2x2 micro-block of
      //      node pairs whose 3x3 blocks accumulate in registers: 17 LDS reads per point serve 4 pairs.  Entries are
      //      summed in the order g = 0, 1, ... as everywhere else (bit-identical to the per-entry formulation).
      const int CH = A.ho_chunk;
      const int CS = (dim * nn + nn + 1 + 1) & ~1;                 // per point: G[dim][nn], H row [nn], c
      double* chunk = reinterpret_cast<double*>(ids + ((nn + 1) & ~1));
      const int nb2 = (nn + 1) / 2, n_mb = nb2 * nb2;
      int sgv[3][3], mv[3][3], sg2v[3][3], m2v[3][3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          sgv[p][k] = sg2v[p][k] = 0;
          mv[p][k] = m2v[p][k] = 0;
          if (p < dim && k < dw) {
            int m = 0;
            sgv[p][k] = curl_term(dim, p, k, &m);
            mv[p][k] = m;
            int m2 = 0;
            if (dim == 2) {
              m2 = 1 - p;
              sg2v[p][k] = p == 0 ? -1 : 1;
            } else {
              sg2v[p][k] = curl_term(3, k, p, &m2);
            }
            m2v[p][k] = m2;
          }
        }
      const bool want_k = A.K || A.Krhs, want_r = A.Rw || A.Rd;
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !want_k : !want_r) continue;
        for (int mb0 = 0; mb0 < n_mb; mb0 += BLOCK) {
          const int mb = mb0 + tid;
          const bool active = mb < n_mb;
          const int bi = active ? mb / nb2 : 0, bj = active ? mb - bi * nb2 : 0;
          const int an[2] = {2 * bi, min(2 * bi + 1, nn - 1)}, bn[2] = {2 * bj, min(2 * bj + 1, nn - 1)};
          const bool av[2] = {active, active && 2 * bi + 1 < nn}, bv[2] = {active, active && 2 * bj + 1 < nn};
          double acc[4][3][3], accd[4][3];
#pragma unroll
          for (int pr = 0; pr < 4; ++pr)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
              accd[pr][p] = 0.0;
#pragma unroll
              for (int q = 0; q < 3; ++q) acc[pr][p][q] = 0.0;
            }
          for (int g0 = 0; g0 < ngt; g0 += CH) {
            const int ng = min(CH, ngt - g0);
            __syncthreads();
            for (int t = tid; t < ng * CS; t += BLOCK) {
              const int gg = t / CS, idx = t - gg * CS, g = g0 + gg;
              const double* P = pt + (int64_t)g * pt_stride;
              double val = 0.0;
              if (idx < dim * nn)
                val = P[dd + 1 + idx];
              else if (idx < dim * nn + nn)
                val = g < nga ? A.H[0][(int64_t)g * nn + (idx - dim * nn)] : A.H[1][(int64_t)(g - nga) * nn + (idx - dim * nn)];
              else if (idx == dim * nn + nn)
                val = P[dd];
              chunk[t] = val;
            }
            __syncthreads();
            if (!active) continue;
            for (int gg = 0; gg < ng; ++gg) {
              const double* Cg = chunk + gg * CS;
              const bool full = g0 + gg < nga;
              const double cg = Cg[dim * nn + nn];
              double ga[2][3], gb[2][3], ha[2], hb[2];
#pragma unroll
              for (int u = 0; u < 2; ++u) {
                ha[u] = Cg[dim * nn + an[u]];
                hb[u] = Cg[dim * nn + bn[u]];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                  ga[u][d] = d < dim ? Cg[d * nn + an[u]] : 0.0;
                  gb[u][d] = d < dim ? Cg[d * nn + bn[u]] : 0.0;
                }
              }
#pragma unroll
              for (int ua = 0; ua < 2; ++ua)
#pragma unroll
                for (int ub = 0; ub < 2; ++ub) {
                  const int pr = ua * 2 + ub;
                  if (pass == 0) {
                    const double sdot = gdot(ga[ua], gb[ub], dim);
                    if (full) {
#pragma unroll
                      for (int p = 0; p < 3; ++p)
                        if (p < dim) acc[pr][p][p] = fma(cg, sdot, acc[pr][p][p]);
                    } else {
#pragma unroll
                      for (int p = 0; p < 3; ++p)
#pragma unroll
                        for (int q = 0; q < 3; ++q)
                          if (p < dim && q < dim)
                            acc[pr][p][q] = fma(cg, kle_pen(A.alpha_d, A.alpha_w, ga[ua][p], gb[ub][q], ga[ua][q], gb[ub][p], sdot, p == q),
                                                acc[pr][p][q]);
                    }
                  } else if (full) {
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                      if (p < dim) accd[pr][p] -= cg * ha[ua] * gb[ub][p];
#pragma unroll
                      for (int k = 0; k < 3; ++k)
                        if (sgv[p][k] != 0) acc[pr][p][k] += cg * ha[ua] * (double)sgv[p][k] * pick3(gb[ub], mv[p][k]);
                    }
                  } else {
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                      if (p < dim) accd[pr][p] += cg * A.alpha_d * ga[ua][p] * hb[ub];
#pragma unroll
                      for (int k = 0; k < 3; ++k)
                        if (sgv[p][k] != 0) acc[pr][p][k] += cg * A.alpha_w * (double)sg2v[p][k] * pick3(ga[ua], m2v[p][k]) * hb[ub];
                    }
                  }
                }
            }
          }
          // ---- scatter the micro-block (same routing as the per-pair path)
#pragma unroll
          for (int ua = 0; ua < 2; ++ua)
#pragma unroll
            for (int ub = 0; ub < 2; ++ub) {
              if (!av[ua] || !bv[ub]) continue;
              const int pr = ua * 2 + ub, a = an[ua], b = bn[ub];
              const int row = ids[a];
              if (row >= A.n_owned) continue;
              const int lo = A.rowptr[row], len = A.rowptr[row + 1] - lo;
              const int sl = find_slot(A.colidx, lo, len, ids[b]);
#pragma unroll
              for (int p = 0; p < 3; ++p) {
                if (p >= dim) continue;
                const int64_t rd = (int64_t)row * dim + p;
                const int ci = A.bcmask ? A.bcmask[rd] : 0;
                if (pass == 0) {
#pragma unroll
                  for (int q = 0; q < 3; ++q) {
                    if (q >= dim) continue;
                    const int cj = A.bcmask ? A.bcmask[(int64_t)ids[b] * dim + q] : 0;
                    const int64_t off = ((int64_t)lo * dim + (int64_t)p * len + sl) * dim + q;
                    const double vv = acc[pr][p][q];
                    if (ci == 0) {
                      if (cj == 0) {
                        if (A.K) atomicAdd(&A.K[off], vv);
                      } else if (A.Krhs) {
                        const int cr = A.rcrow ? A.rcrow[row] : lo;
                        if (cr >= 0) atomicAdd(&A.Krhs[((int64_t)cr * dim + (int64_t)p * len + sl) * dim + q], -vv);
                      }
                    }
                  }
                } else {
                  if (A.Rw) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                      if (k >= dw) continue;
                      const double vv = acc[pr][p][k];
                      if (vv != 0.0 && ci == 0) atomicAdd(&A.Rw[((int64_t)lo * dim + (int64_t)p * len + sl) * dw + k], vv);
                    }
                  }
                  if (A.Rd && ci == 0) atomicAdd(&A.Rd[(int64_t)lo * dim + (int64_t)p * len + sl], accd[pr][p]);
                }
              }
            }
        }
      }
      continue;
    }

    if (oper) {
      const int br = A.op_br, bc = A.op_bc;
      for (int t = tid; t < npair * br * bc; t += BLOCK) {
        int pq = t / npair, ab = t - pq * npair;
        int a = ab / nn, b = ab - a * nn;
        int p = pq / bc, q = pq - p * bc;
        double v = 0.0;
        for (int g = 0; g < nga; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          const double ha = A.H[qa][(int64_t)g * nn + a];
          if (ha == 0.0) continue;  // nodal rules: H is the identity
          double sterm = 0.0;
          for (int k = 0; k < A.op_nterms; ++k)
            if (A.op_terms[3 * k] == p && A.op_terms[3 * k + 1] == q)
              sterm += A.op_coef[k] * P[dd + 1 + A.op_terms[3 * k + 2] * nn + b];
          v += P[dd] * ha * sterm;
        }
        if (DENSE) {
          A.out0[(int64_t)(a * br + p) * (bc * nn) + b * bc + q] = v;
        } else {
          locate(ab, a, b);
          if (r_len < 0) continue;
          int64_t off = ((int64_t)r_lo * br + (int64_t)p * r_len + slot) * bc + q;
          if (v != 0.0) atomicAdd(&A.K[off], v);
        }
      }
      continue;
    }
    if (!kle) {
      // scalar forms: A_ab = sum c G_a.G_b (Laplace) or sum c H_a H_b (mass)
      for (int ab = tid; ab < npair; ab += BLOCK) {
        int a = ab / nn, b = ab - a * nn;
        double v = 0.0;
        for (int g = 0; g < nga; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          double cg = P[dd];
          if (A.form == PYN_FORM_LAPLACE) {
            double s = 0.0;
            for (int d = 0; d < dim; ++d) s += P[dd + 1 + d * nn + a] * P[dd + 1 + d * nn + b];
            v += cg * s;
          } else {
            const double* Hq = A.H[qa] + (int64_t)g * nn;
            v += cg * Hq[a] * Hq[b];
          }
        }
        if (DENSE) {
          A.out0[ab] = v;
        } else {
          locate(ab, a, b);
          if (r_len < 0) continue;
          int ra = ids[a], cb = ids[b];
          bool mr = A.bcmask && A.bcmask[ra], mc = A.bcmask && A.bcmask[cb];
          if (mr) continue;
          int64_t off = (int64_t)r_lo + slot;
          if (mc) {
            if (A.Krhs && r_cr >= 0) atomicAdd(&A.Krhs[(int64_t)r_cr + slot], -v);
          } else if (A.K) {
            atomicAdd(&A.K[off], v);
          }
        }
      }
      continue;
    }

    // ---- KLE blocks.  One lane per NODE PAIR (a, b) computing all components of its block: the point data
    //      (c, G[.][a], G[.][b], H) is read once per pair instead of once per entry, which is what bounds the
    //      high-order elements whose point data lives in global scratch.  Every entry is still summed in the
    //      order g = 0, 1, ... of the per-entry formulation (bit-identical results).
    // ---- K (dim x dim blocks); component loops have the static bound 3 with `< dim` guards so that the
    //      accumulators stay in registers
    if (DENSE ? (A.out0 != nullptr) : (A.K != nullptr || A.Krhs != nullptr || A.Kfs != nullptr || A.Krhsfs != nullptr)) {
      for (int ab = tid; ab < npair; ab += BLOCK) {
        const int a = ab / nn, b = ab - a * nn;
        double vfull = 0.0;
        for (int g = 0; g < nga; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          const double* G = P + dd + 1;
          double ga[3] = {0.0, 0.0, 0.0}, gb[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int d = 0; d < 3; ++d)
            if (d < dim) {
              ga[d] = G[d * nn + a];
              gb[d] = G[d * nn + b];
            }
          vfull = fma(P[dd], gdot(ga, gb, dim), vfull);
        }
        double v[3][3];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int q = 0; q < 3; ++q) v[p][q] = p == q ? vfull : 0.0;
        for (int g = nga; g < ngt; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          const double* G = P + dd + 1;
          double ga[3] = {0.0, 0.0, 0.0}, gb[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int d = 0; d < 3; ++d)
            if (d < dim) {
              ga[d] = G[d * nn + a];
              gb[d] = G[d * nn + b];
            }
          const double s = gdot(ga, gb, dim);
          const double cg = P[dd];
#pragma unroll
          for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q)
              if (p < dim && q < dim) v[p][q] = fma(cg, kle_pen(A.alpha_d, A.alpha_w, ga[p], gb[q], ga[q], gb[p], s, p == q), v[p][q]);
        }
        if (!DENSE) {
          locate(ab, a, b);
          if (r_len < 0) continue;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int q = 0; q < 3; ++q)
            if (p < dim && q < dim) {
              const double vv = v[p][q];
              if (DENSE) {
                A.out0[(int64_t)(a * dim + p) * (dim * nn) + b * dim + q] = vv;
              } else {
                int64_t rd = (int64_t)ids[a] * dim + p, cd = (int64_t)ids[b] * dim + q;
                const int ci = A.bcmask ? A.bcmask[rd] : 0, cj = A.bcmask ? A.bcmask[cd] : 0;
                int64_t off = ((int64_t)r_lo * dim + (int64_t)p * r_len + slot) * dim + q;
                if (ci == 0) {                                   // base_problem.py:426-427 / 388-390
                  if (cj == 0) {
                    if (A.K) atomicAdd(&A.K[off], vv);
                  } else if (A.Krhs && r_cr >= 0) {
                    atomicAdd(&A.Krhs[((int64_t)r_cr * dim + (int64_t)p * r_len + slot) * dim + q], -vv);
                  }
                }
                if (A.Kfs && ((ci == 1 && cj <= 1) || (ci == 0 && cj == 1))) atomicAdd(&A.Kfs[off], vv);   // :396-407
                if (A.Krhsfs && ci <= 1 && cj == 2 && r_crfs >= 0)                                         // :417-422
                  atomicAdd(&A.Krhsfs[((int64_t)r_crfs * dim + (int64_t)p * r_len + slot) * dim + q], -vv);
              }
            }
      }
    }
    // ---- Rw (dim x dim_w blocks)
    if (DENSE ? (A.out1 != nullptr) : (A.Rw != nullptr || A.Rwfs != nullptr)) {
      for (int ab = tid; ab < npair; ab += BLOCK) {
        const int a = ab / nn, b = ab - a * nn;
        double v[3][3];
        int sgv[3][3], mv[3][3], sg2v[3][3], m2v[3][3];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            v[p][k] = 0.0;
            sgv[p][k] = 0;
            mv[p][k] = m2v[p][k] = 0;
            sg2v[p][k] = 0;
            if (p < dim && k < dw) {
              int m = 0;
              sgv[p][k] = curl_term(dim, p, k, &m);  // (curl w)_p picks  sg * d_m w_k
              mv[p][k] = m;
              // reduced: alpha_w c Bc[k][(a,p)] H_b with (curl v)_k = eps_{k m p} d_m v_p
              int m2 = 0;
              if (dim == 2) {  // w = d_x v_y - d_y v_x
                m2 = 1 - p;
                sg2v[p][k] = p == 0 ? -1 : 1;
              } else {
                sg2v[p][k] = curl_term(3, k, p, &m2);
              }
              m2v[p][k] = m2;
            }
          }
        for (int g = 0; g < nga; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          const double cg = P[dd], ha = A.H[0][(int64_t)g * nn + a];
#pragma unroll
          for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k)
              if (sgv[p][k] != 0) v[p][k] += cg * ha * (double)sgv[p][k] * P[dd + 1 + mv[p][k] * nn + b];
        }
        for (int g = nga; g < ngt; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          const double cg = P[dd], hb = A.H[1][(int64_t)(g - nga) * nn + b];
#pragma unroll
          for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int k = 0; k < 3; ++k)
              if (sgv[p][k] != 0) v[p][k] += cg * A.alpha_w * (double)sg2v[p][k] * P[dd + 1 + m2v[p][k] * nn + a] * hb;
        }
        if (!DENSE) {
          locate(ab, a, b);
          if (r_len < 0) continue;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (p < dim && k < dw) {
              const double vv = v[p][k];
              if (DENSE) {
                A.out1[(int64_t)(a * dim + p) * (dw * nn) + b * dw + k] = vv;
              } else {
                int64_t rd = (int64_t)ids[a] * dim + p;
                const int ci = A.bcmask ? A.bcmask[rd] : 0;
                int64_t off = ((int64_t)r_lo * dim + (int64_t)p * r_len + slot) * dw + k;
                if (vv != 0.0) {
                  if (ci == 0 && A.Rw) atomicAdd(&A.Rw[off], vv);
                  if (ci == 1 && A.Rwfs) atomicAdd(&A.Rwfs[off], vv);      // base_problem.py:412-413
                }
              }
            }
      }
    }
    // ---- Rd (dim x 1 blocks)
    if (DENSE ? (A.out2 != nullptr) : (A.Rd != nullptr || A.Rdfs != nullptr)) {
      for (int ab = tid; ab < npair; ab += BLOCK) {
        const int a = ab / nn, b = ab - a * nn;
        double v[3] = {0.0, 0.0, 0.0};
        for (int g = 0; g < nga; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          const double cg = P[dd], ha = A.H[0][(int64_t)g * nn + a];
#pragma unroll
          for (int p = 0; p < 3; ++p)
            if (p < dim) v[p] -= cg * ha * P[dd + 1 + p * nn + b];
        }
        for (int g = nga; g < ngt; ++g) {
          const double* P = pt + (int64_t)g * pt_stride;
          const double cg = P[dd], hb = A.H[1][(int64_t)(g - nga) * nn + b];
#pragma unroll
          for (int p = 0; p < 3; ++p)
            if (p < dim) v[p] += cg * A.alpha_d * P[dd + 1 + p * nn + a] * hb;
        }
        if (!DENSE) {
          locate(ab, a, b);
          if (r_len < 0) continue;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p)
          if (p < dim) {
            if (DENSE) {
              A.out2[(int64_t)(a * dim + p) * nn + b] = v[p];
            } else {
              int64_t rd = (int64_t)ids[a] * dim + p;
              const int ci = A.bcmask ? A.bcmask[rd] : 0;
              int64_t off = (int64_t)r_lo * dim + (int64_t)p * r_len + slot;
              if (ci == 0 && A.Rd) atomicAdd(&A.Rd[off], v[p]);
              if (ci == 1 && A.Rdfs) atomicAdd(&A.Rdfs[off], v[p]);        // base_problem.py:415-416
            }
          }
      }
    }
  }
}

// Unit diagonal on imposed DOFs: Mat.setIndices2One (mat_generator.py:113-118), single-rank
// semantics (diag = 1).  One thread per owned DOF.  With the no-slip split: K, Krhs get 1 on every
// non-free DOF, Kfs gets -1 on the tangential no-slip DOFs (base_problem.py:441-442) so that K + Kfs
// keeps only the doubly imposed DOFs eliminated, Krhsfs gets 1 on those (:449-450).
__global__ void bc_identity_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                   const uint8_t* __restrict__ mask, int64_t n_owned, int ndof, double* __restrict__ K,
                                   double* __restrict__ Krhs, double* __restrict__ Kfs, double* __restrict__ Krhsfs,
                                   const int32_t* __restrict__ rcrow, const int32_t* __restrict__ rcrow_fs) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_owned * ndof; t += (int64_t)gridDim.x * blockDim.x) {
    const int cls = mask[t];
    if (!cls) continue;
    int64_t i = t / ndof;
    int p = (int)(t - i * ndof);
    int lo = rowptr[i], len = rowptr[i + 1] - lo;
    int slot = find_slot(colidx, lo, len, (int)i);
    int64_t off = ((int64_t)lo * ndof + (int64_t)p * len + slot) * ndof + p;
    if (K) K[off] = 1.0;
    if (Krhs) {
      const int cr = rcrow ? rcrow[i] : lo;      // (an imposed row is always stored by a compact matrix)
      if (cr >= 0) Krhs[((int64_t)cr * ndof + (int64_t)p * len + slot) * ndof + p] = 1.0;
    }
    if (Kfs && cls == 1) Kfs[off] -= 1.0;
    if (Krhsfs && cls == 2) {
      const int cr = rcrow_fs ? rcrow_fs[i] : lo;
      if (cr >= 0) Krhsfs[((int64_t)cr * ndof + (int64_t)p * len + slot) * ndof + p] = 1.0;
    }
  }
}

// Linear simplices (constant gradients): one element per lane, no LDS, no barriers.  L_ab = (sum_g w_g) detJ
// G_a.G_b with G = J^-1 Hrs; rows owned by this rank and not eliminated are scatter-added with FP64 atomics,
// the slot found by bisection in the (short: ~7 / ~15 entries) sorted row.  Same elimination rule as the
// generic kernel.  The irregular-indexing workload of BASELINE.json configs[4].
template <int DIM>
__global__ void __launch_bounds__(256) assemble_p1_laplace_kernel(const int32_t* __restrict__ conn, const double* __restrict__ xyz,
                                                                    int64_t n_elem, int64_t n_owned,
                                                                    const int32_t* __restrict__ rowptr,
                                                                    const int32_t* __restrict__ colidx,
                                                                    const uint8_t* __restrict__ bcmask,
                                                                    const double* __restrict__ hrs, double wsum,
                                                                    double* __restrict__ A, double* __restrict__ Arhs,
                                                                    const int32_t* __restrict__ rcrow) {
  constexpr int NN = DIM + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elem) return;
  int ids[NN];
  double X[NN][DIM];
  if (DIM == 3) {
    const int4 q = *reinterpret_cast<const int4*>(conn + e * 4);
    ids[0] = q.x, ids[1] = q.y, ids[2] = q.z, ids[NN - 1] = q.w;
  } else {
#pragma unroll
    for (int a = 0; a < NN; ++a) ids[a] = conn[e * NN + a];
  }
#pragma unroll
  for (int a = 0; a < NN; ++a)
#pragma unroll
    for (int d = 0; d < DIM; ++d) X[a][d] = xyz[(int64_t)ids[a] * DIM + d];
  double H[DIM][NN];
#pragma unroll
  for (int d = 0; d < DIM; ++d)
#pragma unroll
    for (int a = 0; a < NN; ++a) H[d][a] = hrs[d * NN + a];  // uniform: scalar loads
  double J[DIM * DIM], Ji[DIM * DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d)
#pragma unroll
    for (int x = 0; x < DIM; ++x) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < NN; ++a) s += H[d][a] * X[a][x];
      J[d * DIM + x] = s;
    }
  const double cw = wsum * inv_det(J, Ji, DIM);
  double G[DIM][NN];
#pragma unroll
  for (int x = 0; x < DIM; ++x)
#pragma unroll
    for (int a = 0; a < NN; ++a) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < DIM; ++d) s += Ji[x * DIM + d] * H[d][a];
      G[x][a] = s;
    }
  bool mc[NN];
#pragma unroll
  for (int a = 0; a < NN; ++a) mc[a] = bcmask && bcmask[ids[a]];
#pragma unroll
  for (int a = 0; a < NN; ++a) {
    if (ids[a] >= n_owned || mc[a]) continue;
    const int lo = rowptr[ids[a]], len = rowptr[ids[a] + 1] - lo;
#pragma unroll
    for (int b = 0; b < NN; ++b) {
      double v = 0.0;
#pragma unroll
      for (int x = 0; x < DIM; ++x) v += G[x][a] * G[x][b];
      v *= cw;
      const int sl = find_slot(colidx, lo, len, ids[b]);
      const int64_t off = (int64_t)lo + sl;
      if (mc[b]) {
        const int cr = rcrow ? rcrow[ids[a]] : lo;
        if (Arhs && cr >= 0) atomicAdd(&Arhs[(int64_t)cr + sl], -v);
      } else if (A) {
        atomicAdd(&A[off], v);
      }
    }
  }
}

// ---- High-order KLE elements on the FP64 matrix cores -----------------------------------------------------------
// For nn >~ 64 nodes per element the blocks are dense contractions over the Gauss points,
//   S_f  = sum_full c G_d[a] G_d[b]           T_pq = sum_red c G_p[a] G_q[b]
//   U_m  = sum_full c H[a]  G_m[b]            V_m  = sum_red c G_m[a] H[b]
//   K[p][q]  = d_pq (S_f + aw sum_d T_dd) + ad T_pq - aw T_qp                                (spectral.py:131,152-153)
//   Rw[p][k] = sg_pk U_m(p,k) + aw sg2_pk V_m2(p,k)      Rd[p] = -U_p + ad V_p               (:132-133,155-156)
// i.e. small GEMMs with the points as the K dimension: v_mfma_f64_16x16x4_f64 (lane l: A[i = l&15][k = l>>4],
// B[k = l>>4][j = l&15], D col = l&15, row = (l>>4) + 4 reg).  One workgroup per element, each of its 4 waves owns one
// 16x16 tile of node pairs per round with all 16 accumulator tiles in registers; the points pass through LDS in chunks.
typedef double pyn_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) assemble_kle_ho_mfma_kernel(AsmArgs A, int CH) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int dim = A.dim, nn = A.nn, nc = A.nc, dd = dim * dim;
  const int nga = A.ngp[0], ngb = A.ngp[1], ngt = nga + ngb;
  const int nn16 = (nn + 15) & ~15, nt16 = nn16 >> 4;
  double* Xs = reinterpret_cast<double*>(smem_raw);                      // [nc*dim]
  int32_t* ids = reinterpret_cast<int32_t*>(Xs + nc * dim);             // [nn]
  double* Gs = reinterpret_cast<double*>(ids + ((nn + 1) & ~1));        // [dim][CH][nn16]
  double* Hs = Gs + (size_t)dim * CH * nn16;                             // [CH][nn16]
  double* cs = Hs + (size_t)CH * nn16;                                   // [CH]
  const int pt_stride = dd + 1 + dim * nn;
  double* pt = A.gscratch + (int64_t)blockIdx.x * A.gscratch_stride;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dw = dim == 2 ? 1 : 3;
  const int li = lane & 15, lk = lane >> 4;

  int sgv[3][3], mv[3][3], sg2v[3][3], m2v[3][3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sgv[p][k] = sg2v[p][k] = 0;
      mv[p][k] = m2v[p][k] = 0;
      if (p < dim && k < dw) {
        int m = 0;
        sgv[p][k] = curl_term(dim, p, k, &m);
        mv[p][k] = m;
        int m2 = 0;
        if (dim == 2) {
          m2 = 1 - p;
          sg2v[p][k] = p == 0 ? -1 : 1;
        } else {
          sg2v[p][k] = curl_term(3, k, p, &m2);
        }
        m2v[p][k] = m2;
      }
    }

  for (int64_t eq = blockIdx.x; eq < A.n_elem; eq += gridDim.x) {
    const int64_t e = A.esel ? A.esel[eq] : eq;
    __syncthreads();
    for (int t = tid; t < nn; t += 256) ids[t] = A.conn[e * nn + t];
    for (int t = tid; t < nc * dim; t += 256) {
      int cn = t / dim, x = t - cn * dim;
      Xs[t] = A.xyz[(int64_t)A.conn[e * nn + cn] * dim + x];
    }
    __syncthreads();
    for (int g = tid; g < ngt; g += 256) {   // geometry at every point (spectral.py:120-122,140-142)
      const int q = g < nga ? 0 : 1;
      const int gl = g < nga ? g : g - nga;
      const double* hc = A.HrsCoo[q] + (int64_t)gl * dim * nc;
      double J[9], Ji[9];
      for (int d = 0; d < dim; ++d)
        for (int x = 0; x < dim; ++x) {
          double sacc = 0.0;
          for (int cn = 0; cn < nc; ++cn) sacc += hc[d * nc + cn] * Xs[cn * dim + x];
          J[d * dim + x] = sacc;
        }
      double det = inv_det(J, Ji, dim);
      double* P = pt + (int64_t)g * pt_stride;
      for (int i = 0; i < dd; ++i) P[i] = Ji[i];
      P[dd] = A.w[q][gl] * det;
    }
    __syncthreads();
    for (int t = tid; t < ngt * dim * nn; t += 256) {   // G = J^-1 Hrs (:121,141)
      int g = t / (dim * nn);
      int r = t - g * dim * nn;
      int d = r / nn, a = r - d * nn;
      const int q = g < nga ? 0 : 1;
      const int gl = g < nga ? g : g - nga;
      const double* hrs = A.Hrs[q] + (int64_t)gl * dim * nn;
      double* P = pt + (int64_t)g * pt_stride;
      double sacc = 0.0;
      for (int x = 0; x < dim; ++x) sacc += P[d * dim + x] * hrs[x * nn + a];
      P[dd + 1 + d * nn + a] = sacc;
    }
    __syncthreads();

    // ---- tiles of 16 x 16 node pairs, four at a time (one per wave)
    const int n_tiles = nt16 * nt16;
    for (int t0 = 0; t0 < n_tiles; t0 += 4) {
      const int tile = t0 + wave;
      const bool active = tile < n_tiles;
      const int ta = active ? tile / nt16 : 0, tb = active ? tile - ta * nt16 : 0;
      const int a0 = ta * 16, b0 = tb * 16;
      pyn_d4 S = {0, 0, 0, 0}, T[3][3], U[3], V[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        U[p] = S;
        V[p] = S;
#pragma unroll
        for (int q = 0; q < 3; ++q) T[p][q] = S;
      }
      for (int rule = 0; rule < 2; ++rule) {
        const int gbeg = rule == 0 ? 0 : nga, gend = rule == 0 ? nga : ngt;
        for (int g0 = gbeg; g0 < gend; g0 += CH) {
          __syncthreads();
          // stage CH points (zero-padded past the rule's end and past nn)
          for (int t = tid; t < CH * nn16; t += 256) {
            const int kk = t / nn16, a = t - kk * nn16, g = g0 + kk;
            const bool ok = g < gend && a < nn;
            const double* P = pt + (int64_t)(ok ? g : 0) * pt_stride;
#pragma unroll
            for (int d = 0; d < 3; ++d)
              if (d < dim) Gs[((size_t)d * CH + kk) * nn16 + a] = ok ? P[dd + 1 + d * nn + a] : 0.0;
            Hs[(size_t)kk * nn16 + a] = ok ? A.H[rule][(int64_t)(g - gbeg) * nn + a] : 0.0;
            if (a == 0) cs[kk] = g < gend ? P[dd] : 0.0;
          }
          __syncthreads();
          if (!active) continue;
          for (int k4 = 0; k4 < CH; k4 += 4) {
            const int kk = k4 + lk;
            const double cg = cs[kk];
            double ga[3], gb[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              ga[d] = d < dim ? Gs[((size_t)d * CH + kk) * nn16 + a0 + li] : 0.0;
              gb[d] = d < dim ? Gs[((size_t)d * CH + kk) * nn16 + b0 + li] : 0.0;
            }
            const double ha = Hs[(size_t)kk * nn16 + a0 + li], hb = Hs[(size_t)kk * nn16 + b0 + li];
            if (rule == 0) {
#pragma unroll
              for (int d = 0; d < 3; ++d)
                if (d < dim) {
                  S = __builtin_amdgcn_mfma_f64_16x16x4f64(cg * ga[d], gb[d], S, 0, 0, 0);
                  U[d] = __builtin_amdgcn_mfma_f64_16x16x4f64(cg * ha, gb[d], U[d], 0, 0, 0);
                }
            } else {
#pragma unroll
              for (int p = 0; p < 3; ++p)
                if (p < dim) {
                  V[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(cg * ga[p], hb, V[p], 0, 0, 0);
#pragma unroll
                  for (int q = 0; q < 3; ++q)
                    if (q < dim) T[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cg * ga[p], gb[q], T[p][q], 0, 0, 0);
                }
            }
          }
        }
      }
      if (!active) continue;
      // ---- combine and scatter: lane holds rows (lane>>4) + 4 r, column lane&15 of the tile
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = a0 + lk + 4 * r, b = b0 + li;
        if (a >= nn || b >= nn) continue;
        const int row = ids[a];
        if (row >= A.n_owned) continue;
        const int lo = A.rowptr[row], len = A.rowptr[row + 1] - lo;
        const int sl = find_slot(A.colidx, lo, len, ids[b]);
        double tdd = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d)
          if (d < dim) tdd += T[d][d][r];
        const double diag = S[r] + A.alpha_w * tdd;
        double uu[3] = {U[0][r], U[1][r], U[2][r]}, vv3[3] = {V[0][r], V[1][r], V[2][r]};
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          if (p >= dim) continue;
          const int ci = A.bcmask ? A.bcmask[(int64_t)row * dim + p] : 0;
          if (ci != 0) continue;
          if (A.K || A.Krhs) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              if (q >= dim) continue;
              double v = A.alpha_d * T[p][q][r] - A.alpha_w * T[q][p][r];
              if (p == q) v += diag;
              const int cj = A.bcmask ? A.bcmask[(int64_t)ids[b] * dim + q] : 0;
              const int64_t off = ((int64_t)lo * dim + (int64_t)p * len + sl) * dim + q;
              if (cj == 0) {
                if (A.K) atomicAdd(&A.K[off], v);
              } else if (A.Krhs) {
                const int cr = A.rcrow ? A.rcrow[row] : lo;
                if (cr >= 0) atomicAdd(&A.Krhs[((int64_t)cr * dim + (int64_t)p * len + sl) * dim + q], -v);
              }
            }
          }
          if (A.Rw) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              if (k >= dw || sgv[p][k] == 0) continue;
              const double v = (double)sgv[p][k] * pick3(uu, mv[p][k]) + A.alpha_w * (double)sg2v[p][k] * pick3(vv3, m2v[p][k]);
              if (v != 0.0) atomicAdd(&A.Rw[((int64_t)lo * dim + (int64_t)p * len + sl) * dw + k], v);
            }
          }
          if (A.Rd) atomicAdd(&A.Rd[(int64_t)lo * dim + (int64_t)p * len + sl], A.alpha_d * vv3[p] - uu[p]);
        }
      }
    }
  }
}

size_t generic_smem(int dim, int nn, int nc, int ngt, bool pt_lds) {
  size_t s = (size_t)nc * dim * sizeof(double) + (size_t)((nn + 1) & ~1) * sizeof(int32_t);
  if (pt_lds) s += (size_t)ngt * (dim * dim + 1 + dim * nn) * sizeof(double);
  return s;
}

// Which form of the generic kernel an element of nn nodes with ngt points in flight takes (AsmPlan::generic): 1 64 threads, 2 256
// threads with the point data in LDS, 3 ... in global scratch, 4 ... and the Gauss points staged through LDS in chunks of `ch`
// (high-order KLE elements; stageable: plain KLE targets of an assembly), 5 the FP64 matrix cores with chunks of `ch_mfma`
struct GenericPick {
  int sub = 0, ch = 0, ch_mfma = 0;
  bool pt_lds = false;
};
GenericPick generic_pick(int dim, int nn, int nc, int ngt, bool stageable, const AsmKnobs& k) {
  GenericPick g;
  g.pt_lds = (size_t)ngt * (dim * dim + 1 + dim * nn) * sizeof(double) <= 40 * 1024;
  if (stageable && !g.pt_lds && !k.no_ho) {
    const size_t cs = (size_t)((dim * nn + nn + 1 + 1) & ~1) * sizeof(double);
    g.ch = (int)std::max<size_t>(1, std::min<size_t>(16, (48 * 1024) / cs));
  }
  if (g.ch > 0 && nn >= 48 && !k.no_ho_mfma) {
    // dense enough for the FP64 matrix cores: largest chunk of points (multiple of 4) whose staging fits the LDS
    const size_t nn16 = (size_t)((nn + 15) & ~15);
    for (int q = 16; q >= 4 && !g.ch_mfma; q -= 4)
      if (generic_smem(dim, nn, nc, ngt, false) + ((size_t)(dim + 1) * q * nn16 + q) * sizeof(double) <= 96 * 1024) g.ch_mfma = q;
  }
  g.sub = g.ch_mfma ? 5 : (nn <= 8 ? 1 : (g.pt_lds ? 2 : (g.ch ? 4 : 3)));
  return g;
}

int ngt_of(const int* ngp, int form, int op_rule) {
  const int qa = form == PYN_FORM_OPERATOR ? op_rule : (form == PYN_FORM_MASS_NODAL ? 2 : 0);
  return ngp[qa] + (form == PYN_FORM_KLE ? ngp[1] : 0);
}

int fill_args(pyn_ctx* c, AsmArgs& A, int form) {
  A = AsmArgs();   // no mask, no target, no subset, no scratch
  A.conn = c->d_conn;
  A.xyz = c->d_xyz;
  A.n_elem = c->n_elem;
  A.n_owned = c->n_owned;
  A.dim = c->dim;
  A.nn = c->nn;
  A.nc = c->nc;
  for (int q = 0; q < 3; ++q) {
    A.ngp[q] = c->quad[q].ngp;
    A.w[q] = c->quad[q].w;
    A.H[q] = c->quad[q].H;
    A.Hrs[q] = c->quad[q].Hrs;
    A.HrsCoo[q] = c->quad[q].HrsCoo;
  }
  A.rowptr = c->d_rowptr;
  A.colidx = c->d_colidx;
  A.form = form;
  if (form == PYN_FORM_OPERATOR) return PYN_OK;  // rule checked by the caller
  const int qa = form == PYN_FORM_MASS_NODAL ? 2 : 0;
  PYN_CHECK(c->quad[qa].ngp > 0, "element tables for rule %d not set", qa);
  if (form == PYN_FORM_KLE) PYN_CHECK(c->quad[1].ngp > 0, "reduced-rule tables not set");
  return PYN_OK;
}

template <bool DENSE>
int launch_generic(pyn_ctx* c, const AsmKnobs& k, AsmArgs& A, int64_t n_work, int* sub = nullptr) {
  const int ngt = ngt_of(A.ngp, A.form, A.op_rule);
  const size_t pt_bytes = (size_t)ngt * (c->dim * c->dim + 1 + c->dim * c->nn) * sizeof(double);
  const bool stageable = !DENSE && A.form == PYN_FORM_KLE && !A.Kfs && !A.Krhsfs && !A.Rwfs && !A.Rdfs;
  const GenericPick g = generic_pick(c->dim, c->nn, c->nc, ngt, stageable, k);
  if (sub) *sub = g.sub;
  const bool small = c->nn <= 8;
  int grid = (int)std::min<int64_t>(n_work, small ? 256 * 32 : 256 * 4);
  if (!g.pt_lds) {
    A.gscratch_stride = (int64_t)(pt_bytes / sizeof(double));
    PYN_TRY(pyn_ensure_work(c, (size_t)grid * pt_bytes));
    A.gscratch = c->d_work;
  }
  size_t smem = generic_smem(c->dim, c->nn, c->nc, ngt, g.pt_lds);
  if (g.ch > 0) {   // high-order KLE elements (point data in global scratch): stage the Gauss points through LDS, see the kernel
    const size_t cs = (size_t)((c->dim * c->nn + c->nn + 1 + 1) & ~1) * sizeof(double);
    PYN_CHECK(smem + g.ch * cs <= 160 * 1024, "element too large for the high-order staging buffer");
    A.ho_chunk = g.ch;
    smem += g.ch * cs;
  }
  if (g.ch_mfma > 0) {
    const size_t nn16 = (size_t)((c->nn + 15) & ~15);
    const size_t lds = generic_smem(c->dim, c->nn, c->nc, ngt, false) + ((size_t)(c->dim + 1) * g.ch_mfma * nn16 + g.ch_mfma) * sizeof(double);
    // (a size that follows the element: set at every launch, another context of the device may have set less)
    PYN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(assemble_kle_ho_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    assemble_kle_ho_mfma_kernel<<<grid, 256, lds, c->stream>>>(A, g.ch_mfma);
    PYN_HIP(hipGetLastError());
    return PYN_OK;
  }
  if (smem > 64 * 1024) PYN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(assemble_generic_kernel<256, false, DENSE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  if (small) {
    assemble_generic_kernel<64, true, DENSE><<<grid, 64, smem, c->stream>>>(A);
  } else if (g.pt_lds) {
    assemble_generic_kernel<256, true, DENSE><<<grid, 256, smem, c->stream>>>(A);
  } else {
    assemble_generic_kernel<256, false, DENSE><<<grid, 256, smem, c->stream>>>(A);
  }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

// ---- pieces every entry point shares -------------------------------------------------------------------------------------------
int zero_blocks(pyn_ctx* c, double* val, int64_t blocks, int br, int bc) {
  if (val) PYN_HIP(hipMemsetAsync(val, 0, (size_t)blocks * br * bc * sizeof(double), c->stream));
  return PYN_OK;
}

// identity rows / zero rows of the imposed DOFs in K (and Kfs), Krhs (and Krhsfs)
void launch_bc_identity(pyn_ctx* c, int ndof, double* K, double* Krhs, double* Kfs, double* Krhsfs, const int32_t* rcrow,
                        const int32_t* rcrow_fs) {
  const int64_t n = c->n_owned * ndof;
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
  bc_identity_kernel<<<grid, 256, 0, c->stream>>>(c->d_rowptr, c->d_colidx, c->d_bcmask, c->n_owned, ndof, K, Krhs, Kfs, Krhsfs, rcrow, rcrow_fs);
}

// end of the timed numeric phase (it began with the record of c->ev0) + the record pyn_assemble_last reports
int asm_finish(pyn_ctx* c, const AsmPlan& P, const AsmRequest& rq) {
  PYN_HIP(hipEventRecord(c->ev1, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  float ms = 0;
  PYN_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->timers[PYN_T_ASSEMBLE] = ms;
  const int64_t r[7] = {P.kind, P.shape, P.k_closed, P.rw_closed, P.kind == AK_GENERIC ? rq.generic : 0, rq.krhs_completed, rq.dinv_written};
  std::copy(r, r + 7, c->asm_last);
  c->asm_last[7] += 1;
  c->asm_last_rows[0] = rq.rows_form;
  c->asm_last_rows[1] = rq.rows_grid;
  return PYN_OK;
}

// ---- the choice ------------------------------------------------------------------------------------------------------------------
// The static halves of the three structured families: what must hold before the device facts they read are worth gathering
// (asm_facts) and before they can be chosen (asm_choose).
bool rowrun_asked(const AsmRequest& rq) {   // K (+ Krhs, Rw) or Rw alone of the KLE form, the scalar Laplacian
  if (rq.variant == 0 || rq.Rd) return false;
  return rq.form == PYN_FORM_KLE ? rq.K || (rq.Rw && !rq.Krhs) : rq.form == PYN_FORM_LAPLACE && rq.K && !rq.Rw;
}
bool rowrun_static(const AsmRequest& rq, const AsmFacts& f, const AsmKnobs& k) {
  if (!f.ho3_valid || f.ho3_tabs_nn != f.nn || f.ngp0 < 1) return false;
  if (rq.form == PYN_FORM_OPERATOR)
    return rq.op_rule == PYN_Q_NODAL && f.ho3_tabs_ok2 && rq.op_nterms <= PYN_HO3_MAX_TERMS && !k.no_ho3_operator;
  return rowrun_asked(rq) && f.ho3_tabs_ok0 && !(f.ngl == 2 && f.dim == 3) && (rq.form != PYN_FORM_KLE || f.ho3_tabs_ok1);
}
bool lattice_static(const AsmRequest& rq, const AsmFacts& f) {
  return rq.variant != 0 && rq.form == PYN_FORM_LAPLACE && rq.K && !rq.Rw && !rq.Rd && f.lat_valid && !f.plan0_user && f.ngp0 == 8;
}
bool kle_lattice_static(const AsmRequest& rq, const AsmFacts& f, const AsmKnobs& k) {   // (Rw alone is a legal request of the ABI)
  return rq.variant != 0 && rq.form == PYN_FORM_KLE && (rq.K || (rq.Rw && !rq.Krhs)) && !rq.Rd && !f.plan1_user && f.lat_valid &&
         f.ngp0 == 8 && f.ngp1 == 1 && !k.no_kle_lattice;
}
// the patch-plan kernels fit the request and the element (a plan is another matter)
bool patch_static(const AsmRequest& rq, const AsmFacts& f, const AsmKnobs& k) {
  if (rq.variant == 0 || !rq.K || rq.Rd || f.dim != 3) return false;
  if (rq.form == PYN_FORM_KLE) return f.nn == 8 && f.ngp0 == 8 && f.ngp1 == 1;
  return rq.form == PYN_FORM_LAPLACE && !rq.Rw && ((f.nn == 4 && f.const_grad && !k.no_p1_tiled) || (f.nn == 8 && f.ngp0 == 8));
}
int table_id(int id, int last) { return id >= 1 && id <= last ? id : 0; }   // ids a PYNAMA_*_TILE table does not number: its default arm

}  // namespace

#define PYN_F(f, e) k.f = getenv(e) != nullptr;
// (negative stands for "not set" where being set matters -- d < 0: a negative value that IS set reads as 0, which every such switch
// treats as that value: the default arm of a tile table, at least one workgroup)
#define PYN_I(f, e, d) \
  if (const char* v = getenv(e)) k.f = d < 0 ? std::max(atoi(v), 0) : atoi(v);
AsmKnobs asm_knobs() { AsmKnobs k; PYN_ASM_KNOBS(PYN_F, PYN_I) PYN_ASM_LAUNCH_KNOBS(PYN_F, PYN_I) return k; }
AsmKnobs lat_fill_knobs() { AsmKnobs k; PYN_LAT_FILL_KNOBS(PYN_F, PYN_I) return k; }
#undef PYN_F
#undef PYN_I

// Today's cascade, once: row-run view -> lattice / march -> KLE lattice -> patch plan -> P1 -> generic.  Host only.
AsmPlan asm_choose(const AsmRequest& rq, const AsmFacts& f, const AsmKnobs& k) {
  AsmPlan P;
  const bool kle = rq.form == PYN_FORM_KLE, op = rq.form == PYN_FORM_OPERATOR;
  const bool aff = f.mesh_affine == 1 && !k.no_affine;   // every element a parallelepiped and the shortcut tables in use
  P.rowrun_candidate = f.ho3_valid && rowrun_asked(rq);
  if (rowrun_static(rq, f, k) && f.ho3_affine == 1 && !k.no_ho3_lattice) {
    P.kind = AK_ROWRUN;
    P.shape = pyn_ho3_run_length(f.dim, f.ngl, op, k.ho3_run);
    P.k_closed = rq.K != nullptr;
    P.rw_closed = rq.Rw != nullptr;
    return P;
  }
  const bool compact = rq.Krhs && rq.rcrow;   // lattice, march and patch kernels cannot address a compact target: krhs_pending
  if (lattice_static(rq, f)) {
    P.krhs_pending = compact;
    P.k_closed = aff && f.aff_standard;
    P.dinv = !k.no_dinv;
    if (!P.k_closed && f.q1_gauss_standard && f.lat_std_ok == 1 && k.lattice_tile < 0 && !k.no_march) {   // general geometry: FP64-bound
      P.kind = AK_MARCH;
      P.shape = k.march_tile == 4 ? 0 : table_id(k.march_tile, 14);
    } else {
      P.kind = AK_LATTICE;
      P.shape = table_id(k.lattice_tile >= 0 ? k.lattice_tile : (P.k_closed ? 0 : 1), 9);
    }
    return P;
  }
  if (kle_lattice_static(rq, f, k)) {
    const bool affine = aff && f.aff_standard && f.aff_rw_standard;
    if (affine || (f.q1_gauss_standard && f.q1_red_standard && !k.no_kle_general)) {
      P.kind = AK_KLE_LATTICE;
      P.shape = affine ? table_id(k.kle_lattice_tile, 4) : 0;
      P.kle_general = !affine;
      P.k_closed = affine && rq.K;
      P.rw_closed = affine && rq.Rw;
      return P;
    }
  }
  // a graph without a plan gets the automatic one whenever its elements are the patch kernels' (fitting tables or not, as ever)
  const bool plan = kle ? f.plan1_present : f.plan0_present;
  P.want_plan = !plan && !(kle ? f.plan1_unfit : f.plan0_unfit) && rq.variant != 0 && rq.K && !rq.Rd && f.dim == 3 &&
                (kle ? f.nn == 8 : rq.form == PYN_FORM_LAPLACE && !rq.Rw && (f.nn == 8 || (f.nn == 4 && f.const_grad)));
  if (patch_static(rq, f, k) && (plan || P.want_plan)) {
    P.kind = AK_PATCH;
    P.krhs_pending = compact;
    if (kle) {
      P.k_closed = aff && f.aff_standard;
      P.rw_closed = rq.Rw && aff && f.aff_rw_standard;
    } else {
      P.k_closed = f.nn == 8 && aff && f.aff_standard && !k.tiled_ablate && !k.no_lean_plan;
    }
    return P;
  }
  const int ngp[3] = {f.ngp0, f.ngp1, f.ngp2};
  if (rq.form == PYN_FORM_LAPLACE && f.nn == f.dim + 1 && f.const_grad && !k.no_p1)
    P.kind = AK_P1;
  else
    P.generic = generic_pick(f.dim, f.nn, f.nc, ngt_of(ngp, rq.form, rq.op_rule), kle, k).sub;
  return P;
}

// The facts of the context.  Device work only where the static facts make its reader a candidate: the geometry pre-pass of the row-run
// kernels (every row-run assembly, part of the timed phase), the two lattice checks and the all-affine check of the patch kernels
// (cached per mesh / graph; the patch kernels' only once a plan exists, as the automatic plan is built first).
int asm_facts(pyn_ctx* c, const AsmRequest& rq, const AsmKnobs& k, AsmFacts* f) {
  f->dim = c->dim;
  f->nn = c->nn;
  f->nc = c->nc;
  f->ngl = c->box.ngl;
  f->ngp0 = c->quad[0].ngp;
  f->ngp1 = c->quad[1].ngp;
  f->ngp2 = c->quad[2].ngp;
  f->const_grad = c->quad[0].const_grad;
  f->q1_gauss_standard = c->q1_gauss_standard;
  f->q1_red_standard = c->q1_red_standard;
  f->aff_standard = c->aff_standard;
  f->aff_rw_standard = c->aff_rw_standard;
  f->lat_valid = c->lat.valid;
  f->ho3_valid = c->ho3.valid;
  f->ho3_tabs_nn = c->ho3_tabs_nn;
  f->ho3_tabs_ok0 = c->ho3_tabs_ok[0];
  f->ho3_tabs_ok1 = c->ho3_tabs_ok[1];
  f->ho3_tabs_ok2 = c->ho3_tabs_ok[2];
  f->plan0_present = c->plan[0].npatch > 0;
  f->plan1_present = c->plan[1].npatch > 0;
  f->plan0_user = c->plan[0].user;
  f->plan1_user = c->plan[1].user;
  f->plan0_unfit = c->plan_unfit[0] || f->plan_declined;
  f->plan1_unfit = c->plan_unfit[1] || f->plan_declined;
  if (rowrun_static(rq, *f, k) && !f->geom_done) {
    PYN_TRY(pyn_ho3_prepare(c));
    f->geom_done = true;
  }
  f->ho3_affine = c->ho3.affine;
  const bool kle = rq.form == PYN_FORM_KLE;
  if (lattice_static(rq, *f) || kle_lattice_static(rq, *f, k)) PYN_TRY(pyn_lattice_checks(c, k));
  if (patch_static(rq, *f, k) && (kle ? f->plan1_present : f->plan0_present) && !k.no_affine &&
      (kle ? c->aff_standard || (rq.Rw && c->aff_rw_standard) : c->nn == 8 && c->aff_standard && !k.tiled_ablate && !k.no_lean_plan)) {
    int all_aff = 0;
    PYN_TRY(pyn_mesh_all_affine(c, &all_aff));
  }
  f->mesh_affine = c->mesh_affine;
  f->lat_std_ok = c->lat_std_ok;
  return PYN_OK;
}

namespace {

// Does the imposed-column matrix `id` already hold zeros wherever the current Dirichlet set leaves zeros (DMat::rhs_clean)?  Read
// BEFORE mat_ptr marks the matrix as changing.
bool rhs_is_clean(pyn_ctx* c, const AsmKnobs& k, int id) {
  if (id < 0 || id >= (int)c->mats.size() || !c->mats[id].live || k.rhs_full_write) return false;
  const int64_t s = c->mats[id].rhs_clean;
  return s == PYN_RHS_ANY || s == c->bc_stamp;
}

// crow != null: the argument may be a compact imposed-column matrix (Krhs, Krhsfs, Arhs); its row selection is brought to the current
// Dirichlet set (values zeroed when it had to be rebuilt) and handed back, null for a matrix with the graph's full pattern
int mat_ptr(pyn_ctx* c, int id, int br, int bc, const char* name, double** out, const int32_t** crow = nullptr) {
  *out = nullptr;
  if (crow) *crow = nullptr;
  if (id < 0) return PYN_OK;
  PYN_TRY(pyn_check_mat(c, id, name));
  DMat& m = c->mats[id];
  PYN_CHECK(m.br == br && m.bc == bc, "%s must have block shape %dx%d (has %dx%d)", name, br, bc, m.br, m.bc);
  PYN_CHECK(crow || !m.rhs_compact, "%s: a compact imposed-column matrix (pyn_mat_create_rhs) can only be the Krhs / Arhs target", name);
  if (m.rhs_compact) {
    PYN_TRY(pyn_rhs_ensure(c, m, true));   // laid out for the Dirichlet set of THIS assembly
    *crow = m.c_crow;
  }
  m.touch();  // values are about to change
  *out = m.val;
  return PYN_OK;
}

// blocks stored by the matrix behind a raw value pointer of this assembly (the compact Krhs target, or the graph's count)
int64_t rhs_blocks(const pyn_ctx* c, int id) { return id >= 0 ? pyn_mat_blocks(c, c->mats[id]) : c->nnzb; }

// The actor: facts, choice, one switch onto the launchers, completion of a compact Krhs, record.  op_terms / op_coef: the device
// copies of an operator's terms.
int asm_run(pyn_ctx* c, AsmRequest& rq, const AsmKnobs& k, const int32_t* op_terms = nullptr, const double* op_coef = nullptr) {
  PYN_CHECK(c->d_rowptr, "pyn_csr_symbolic first");
  const bool kle = rq.form == PYN_FORM_KLE, op = rq.form == PYN_FORM_OPERATOR;
  const int ndof = kle ? c->dim : 1, dw = c->dim == 2 ? 1 : 3;
  if (c->d_bcmask && !op) PYN_CHECK(c->bc_ndof == ndof, "bc mask has ndof=%d, form needs %d", c->bc_ndof, ndof);
  AsmArgs A;
  PYN_TRY(fill_args(c, A, rq.form));
  A.bcmask = op ? nullptr : c->d_bcmask;
  A.alpha_d = rq.alpha_d;
  A.alpha_w = rq.alpha_w;
  A.K = rq.K;
  A.Krhs = rq.Krhs;
  A.Rw = rq.Rw;
  A.Rd = rq.Rd;
  A.rcrow = rq.rcrow;
  A.op_rule = rq.op_rule;
  A.op_br = rq.op_br;
  A.op_bc = rq.op_bc;
  A.op_nterms = rq.op_nterms;
  A.op_terms = op_terms;
  A.op_coef = op_coef;
  PYN_HIP(hipEventRecord(c->ev0, c->stream));
  AsmFacts f;
  AsmPlan P;
  for (;;) {   // the one loop-back: the patch kernels' turn without a plan builds the automatic one, which may not fit (or be switched off)
    PYN_TRY(asm_facts(c, rq, k, &f));
    P = asm_choose(rq, f, k);
    if (!P.want_plan) break;
    PYN_TRY(pyn_patch_plan_default(c, kle));
    f.plan_declined = !c->plan[kle].npatch;
  }
  PYN_CHECK(!(k.ho3_require && P.rowrun_candidate && P.kind != AK_ROWRUN),
            "PYNAMA_HO3_REQUIRE: the ngl = 3 lattice kernels declined this assembly (non-affine cell or tables missing)");
  switch (P.kind) {
    case AK_ROWRUN: PYN_TRY(pyn_assemble_ho3_lattice(c, rq, k, P)); break;   // no atomics, every row written once
    case AK_LATTICE:
    case AK_MARCH: PYN_TRY(pyn_assemble_lattice(c, rq, k, P)); break;
    case AK_KLE_LATTICE: PYN_TRY(pyn_assemble_kle_lattice(c, rq, k, P)); break;
    case AK_PATCH: PYN_TRY(pyn_assemble_patch(c, rq, k, P)); break;
    default: {   // scatter-add path: values start from zero (the other families write every entry themselves)
      const int br = op ? rq.op_br : ndof, bc = op ? rq.op_bc : ndof;
      PYN_TRY(zero_blocks(c, rq.K, c->nnzb, br, bc));
      PYN_TRY(zero_blocks(c, rq.Krhs, rq.krhs_blocks, ndof, ndof));
      PYN_TRY(zero_blocks(c, rq.Rw, c->nnzb, ndof, dw));
      PYN_TRY(zero_blocks(c, rq.Rd, c->nnzb, ndof, 1));
      if (P.kind == AK_P1) {
        const QuadTab& q0 = c->quad[0];
        const auto p1 = c->dim == 3 ? assemble_p1_laplace_kernel<3> : assemble_p1_laplace_kernel<2>;
        p1<<<(int)((c->n_elem + 255) / 256), 256, 0, c->stream>>>(c->d_conn, c->d_xyz, c->n_elem, c->n_owned, c->d_rowptr, c->d_colidx,
                                                                   c->d_bcmask, q0.Hrs, q0.wsum, rq.K, rq.Krhs, rq.rcrow);
        PYN_HIP(hipGetLastError());
      } else {
        PYN_TRY(launch_generic<false>(c, k, A, c->n_elem, &rq.generic));
      }
      if (!op && c->d_bcmask && (rq.K || rq.Krhs)) launch_bc_identity(c, ndof, rq.K, rq.Krhs, nullptr, nullptr, rq.rcrow, nullptr);
    }
  }
  if (P.krhs_pending) {
    // the kernel family that took K cannot address a compact Krhs: -K_e[free, bc] comes from the elements that hold an imposed node
    // (a few per cent of the mesh) through the generic kernel, into the zeroed compact matrix
    PYN_TRY(pyn_bc_elements(c));
    PYN_TRY(zero_blocks(c, rq.Krhs, rq.krhs_blocks, ndof, ndof));
    if (c->n_esel > 0) {
      AsmArgs B = A;
      B.K = B.Rw = B.Rd = nullptr;
      B.esel = c->d_esel;
      B.n_elem = c->n_esel;
      PYN_TRY(launch_generic<false>(c, k, B, c->n_esel));
    }
    if (c->d_bcmask) launch_bc_identity(c, ndof, nullptr, rq.Krhs, nullptr, nullptr, rq.rcrow, nullptr);
    rq.krhs_completed = true;
  }
  return asm_finish(c, P, rq);
}

}  // namespace

extern "C" int pyn_assemble_kle(pyn_ctx* c, double alpha_d, double alpha_w, int K, int Krhs, int Rw, int Rd, int variant) {
  PYN_CHECK(c, "ctx is NULL");
  PYN_HIP(hipSetDevice(c->device));
  const int dim = c->dim, dw = dim == 2 ? 1 : 3;
  const AsmKnobs k = asm_knobs();
  AsmRequest rq;
  rq.form = PYN_FORM_KLE;
  rq.variant = variant;
  rq.alpha_d = alpha_d;
  rq.alpha_w = alpha_w;
  PYN_TRY(mat_ptr(c, K, dim, dim, "K", &rq.K));
  rq.rhs_clean = Krhs != K && rhs_is_clean(c, k, Krhs);   // (read before mat_ptr marks the matrix as changing)
  PYN_TRY(mat_ptr(c, Krhs, dim, dim, "Krhs", &rq.Krhs, &rq.rcrow));
  if (rq.rcrow) rq.rhs_clean = false;                     // a compact matrix has no zero blocks to skip: every stored row is written
  PYN_TRY(mat_ptr(c, Rw, dim, dw, "Rw", &rq.Rw));
  PYN_TRY(mat_ptr(c, Rd, dim, 1, "Rd", &rq.Rd));
  rq.krhs_blocks = rhs_blocks(c, Krhs);
  PYN_TRY(asm_run(c, rq, k));
  if (rq.Krhs && rq.K) c->mats[Krhs].rhs_clean = c->bc_stamp;   // exactly the imposed-column matrix of this Dirichlet set
  return PYN_OK;
}

extern "C" int pyn_assemble_kle_noslip(pyn_ctx* c, double alpha_d, double alpha_w, const int* mat_ids /*[8]*/) {
  PYN_CHECK(c && mat_ids, "NULL argument");
  PYN_CHECK(c->d_rowptr, "pyn_csr_symbolic first");
  PYN_CHECK(c->d_bcmask && c->bc_ndof == c->dim, "pyn_bc_set(dim, classes) first: 0 free, 1 tangential no-slip, 2 imposed");
  PYN_HIP(hipSetDevice(c->device));
  const int dim = c->dim, dw = dim == 2 ? 1 : 3;
  const int shapes[8][2] = {{dim, dim}, {dim, dim}, {dim, dw}, {dim, 1}, {dim, dim}, {dim, dim}, {dim, dw}, {dim, 1}};
  const char* names[8] = {"K", "Krhs", "Rw", "Rd", "Kfs", "Krhsfs", "Rwfs", "Rdfs"};
  AsmArgs A;
  PYN_TRY(fill_args(c, A, PYN_FORM_KLE));
  A.bcmask = c->d_bcmask;
  A.alpha_d = alpha_d;
  A.alpha_w = alpha_w;
  double** const ptr[8] = {&A.K, &A.Krhs, &A.Rw, &A.Rd, &A.Kfs, &A.Krhsfs, &A.Rwfs, &A.Rdfs};
  const int32_t** const crow[8] = {nullptr, &A.rcrow, nullptr, nullptr, nullptr, &A.rcrow_fs, nullptr, nullptr};   // compact: Krhs, Krhsfs
  for (int i = 0; i < 8; ++i) {
    PYN_TRY(mat_ptr(c, mat_ids[i], shapes[i][0], shapes[i][1], names[i], ptr[i], crow[i]));
    PYN_TRY(zero_blocks(c, *ptr[i], rhs_blocks(c, mat_ids[i]), shapes[i][0], shapes[i][1]));
  }
  AsmRequest rq;   // the split has the generic kernel only
  PYN_HIP(hipEventRecord(c->ev0, c->stream));
  PYN_TRY(launch_generic<false>(c, asm_knobs(), A, c->n_elem, &rq.generic));
  launch_bc_identity(c, dim, A.K, A.Krhs, A.Kfs, A.Krhsfs, A.rcrow, A.rcrow_fs);
  return asm_finish(c, AsmPlan(), rq);
}

extern "C" int pyn_assemble_scalar(pyn_ctx* c, int form, int Aid, int Arhs, int variant) {
  PYN_CHECK(c, "ctx is NULL");
  PYN_CHECK(form == PYN_FORM_LAPLACE || form == PYN_FORM_MASS_NODAL || form == PYN_FORM_MASS_FULL, "bad scalar form");
  PYN_HIP(hipSetDevice(c->device));
  const AsmKnobs k = asm_knobs();
  AsmRequest rq;
  rq.form = form;
  rq.variant = variant;
  rq.rhs_clean = Arhs != Aid && rhs_is_clean(c, k, Arhs);
  PYN_TRY(mat_ptr(c, Aid, 1, 1, "A", &rq.K));
  PYN_TRY(mat_ptr(c, Arhs, 1, 1, "Arhs", &rq.Krhs, &rq.rcrow));
  if (rq.rcrow) rq.rhs_clean = false;
  rq.krhs_blocks = rhs_blocks(c, Arhs);
  // the Jacobi data of A: kernels that see whole rows (lattice store phases) write 1 / diagonal on the way out
  if (Aid >= 0 && form == PYN_FORM_LAPLACE && !k.no_dinv) {
    DMat& m = c->mats[Aid];
    if (!m.dinv) PYN_HIP(m.dinv.alloc((size_t)c->n_owned));
    rq.dinv = m.dinv;
  }
  PYN_TRY(asm_run(c, rq, k));
  if (rq.dinv_written) c->mats[Aid].dinv_valid = true;
  if (rq.Krhs && rq.K) c->mats[Arhs].rhs_clean = c->bc_stamp;
  return PYN_OK;
}

extern "C" int pyn_assemble_last(pyn_ctx* c, int64_t* info) {
  PYN_CHECK(c && info, "NULL argument");
  std::copy(c->asm_last, c->asm_last + 8, info);
  return PYN_OK;
}

extern "C" int pyn_assemble_last_rows(pyn_ctx* c, int64_t* info) {
  PYN_CHECK(c && info, "NULL argument");
  std::copy(c->asm_last_rows, c->asm_last_rows + 2, info);
  return PYN_OK;
}

// request slots, then the facts and the knobs in the order of their tables in pyn_internal.h
#define PYN_ASM_REQUEST "form,variant,K,Krhs,Rw,Rd,krhs_compact,op_rule,op_nterms"
extern "C" int pyn_assemble_choose_layout(char* buf, int len) {
#define PYN_X(f) #f ","
#define PYN_F(f, e) #f ","
#define PYN_I(f, e, d) #f ","
  const char* layout = "request:" PYN_ASM_REQUEST ";facts:" PYN_ASM_FACTS(PYN_X) ";knobs:" PYN_ASM_KNOBS(PYN_F, PYN_I);
#undef PYN_X
#undef PYN_F
#undef PYN_I
  PYN_CHECK(buf && len > (int)strlen(layout), "pyn_assemble_choose_layout: the buffer needs %zu bytes", strlen(layout) + 1);
  strcpy(buf, layout);
  return PYN_OK;
}

extern "C" int pyn_assemble_choose(const int64_t* request, const int64_t* facts, const int64_t* knobs, int64_t* out) {
  PYN_CHECK(request && facts && knobs && out, "pyn_assemble_choose: NULL argument");
  static double target;
  static const int32_t crow = 0;
  AsmRequest rq;
  rq.form = (int)request[0];
  rq.variant = (int)request[1];
  rq.K = request[2] ? &target : nullptr;
  rq.Krhs = request[3] ? &target : nullptr;
  rq.Rw = request[4] ? &target : nullptr;
  rq.Rd = request[5] ? &target : nullptr;
  rq.rcrow = request[6] ? &crow : nullptr;
  rq.op_rule = (int)request[7];
  rq.op_nterms = (int)request[8];
  AsmFacts f;
  AsmKnobs k;
#define PYN_X(m) f.m = (int)*facts++;
#define PYN_F(m, e) k.m = *knobs++ > 0;
#define PYN_I(m, e, d) \
  if (*knobs++ >= 0) k.m = (int)knobs[-1];
  PYN_ASM_FACTS(PYN_X)
  PYN_ASM_KNOBS(PYN_F, PYN_I)
#undef PYN_X
#undef PYN_F
#undef PYN_I
  const AsmPlan P = asm_choose(rq, f, k);
  const int64_t r[8] = {P.kind, P.shape, P.k_closed, P.rw_closed, P.generic, P.krhs_pending, P.dinv, P.rowrun_candidate};
  std::copy(r, r + 8, out);
  return PYN_OK;
}

extern "C" int pyn_elem_local(pyn_ctx* c, int form, double alpha_d, double alpha_w, const double* corners, double* out0,
                              double* out1, double* out2) {
  PYN_CHECK(c && corners, "NULL argument");
  PYN_CHECK(c->nn > 0, "pyn_mesh_set first (it fixes dim / nn)");
  PYN_HIP(hipSetDevice(c->device));
  const int dim = c->dim, nn = c->nn, dw = dim == 2 ? 1 : 3;
  const bool kle = form == PYN_FORM_KLE;
  size_t n0 = kle ? (size_t)dim * nn * dim * nn : (size_t)nn * nn;
  size_t n1 = kle ? (size_t)dim * nn * dw * nn : 0;
  size_t n2 = kle ? (size_t)dim * nn * nn : 0;
  size_t ncor = (size_t)c->nc * dim;
  PYN_HIP(c->d_eloc.grow(n0 + n1 + n2 + ncor));
  double* d_cor = c->d_eloc;
  double* d0 = d_cor + ncor;
  double* d1 = d0 + n0;
  double* d2 = d1 + n1;
  PYN_HIP(hipMemcpyAsync(d_cor, corners, ncor * sizeof(double), hipMemcpyHostToDevice, c->stream));
  AsmArgs A;
  PYN_TRY(fill_args(c, A, form));
  A.alpha_d = alpha_d;
  A.alpha_w = alpha_w;
  A.corners = d_cor;
  A.out0 = out0 ? d0 : nullptr;
  A.out1 = (kle && out1) ? d1 : nullptr;
  A.out2 = (kle && out2) ? d2 : nullptr;
  PYN_TRY(launch_generic<true>(c, asm_knobs(), A, 1));
  if (out0) PYN_HIP(hipMemcpyAsync(out0, d0, n0 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (kle && out1) PYN_HIP(hipMemcpyAsync(out1, d1, n1 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (kle && out2) PYN_HIP(hipMemcpyAsync(out2, d2, n2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}

// ---- first-order operator blocks (SrT / DivSrT / Curl of Spectral.getElemKLEOperators, spectral.py:159-218)
static int upload_terms(pyn_ctx* c, int nterms, const int32_t* terms, const double* coef, DevBuf<int32_t>& dt, DevBuf<double>& dc) {
  PYN_TRY(dev_upload(dt, terms, (size_t)nterms * 3, c->stream));
  return dev_upload(dc, coef, (size_t)nterms, c->stream);
}

static int check_operator(pyn_ctx* c, int rule, int br, int bc, int nterms, const int32_t* terms, const double* coef) {
  PYN_CHECK(c && terms && coef, "NULL argument");
  PYN_CHECK(rule >= 0 && rule < 3 && c->quad[rule].ngp > 0, "element tables for rule %d not set", rule);
  PYN_CHECK(br >= 1 && br <= 6 && bc >= 1 && bc <= 6 && nterms >= 1 && nterms <= 64, "bad operator shape");
  for (int k = 0; k < nterms; ++k)
    PYN_CHECK(terms[3 * k] >= 0 && terms[3 * k] < br && terms[3 * k + 1] >= 0 && terms[3 * k + 1] < bc && terms[3 * k + 2] >= 0 &&
                  terms[3 * k + 2] < c->dim,
              "operator term %d out of range", k);
  return PYN_OK;
}

extern "C" int pyn_assemble_operator(pyn_ctx* c, int rule, int nterms, const int32_t* terms, const double* coef, int mat_id) {
  PYN_TRY(pyn_check_mat(c, mat_id, "pyn_assemble_operator"));
  DMat& M = c->mats[mat_id];
  PYN_CHECK(!M.rhs_compact, "pyn_assemble_operator: the target must have the graph's full pattern");
  PYN_TRY(check_operator(c, rule, M.br, M.bc, nterms, terms, coef));
  PYN_HIP(hipSetDevice(c->device));
  DevBuf<int32_t> dt;   // (their release at the end of the call waits for the kernels that read them)
  DevBuf<double> dc;
  PYN_TRY(upload_terms(c, nterms, terms, coef, dt, dc));
  AsmRequest rq;
  rq.form = PYN_FORM_OPERATOR;
  rq.op_rule = rule;
  rq.op_br = M.br;
  rq.op_bc = M.bc;
  rq.op_nterms = nterms;
  rq.op_terms = terms;
  rq.op_coef = coef;
  rq.K = M.val;
  M.touch();
  PYN_TRY(asm_run(c, rq, asm_knobs(), dt, dc));   // structured meshes of parallelepipeds: the row-run kernels, else scatter-add
  return PYN_OK;
}

extern "C" int pyn_elem_operator_local(pyn_ctx* c, int rule, int br, int bc, int nterms, const int32_t* terms,
                                       const double* coef, const double* corners, double* out) {
  PYN_CHECK(corners && out, "NULL argument");
  PYN_TRY(check_operator(c, rule, br, bc, nterms, terms, coef));
  PYN_HIP(hipSetDevice(c->device));
  const size_t n0 = (size_t)br * c->nn * bc * c->nn, ncor = (size_t)c->nc * c->dim;
  PYN_HIP(c->d_eloc.grow(n0 + ncor));
  DevBuf<int32_t> dt;   // (their release at the end of the call waits for the kernels that read them)
  DevBuf<double> dc;
  PYN_TRY(upload_terms(c, nterms, terms, coef, dt, dc));
  PYN_HIP(hipMemcpyAsync(c->d_eloc, corners, ncor * sizeof(double), hipMemcpyHostToDevice, c->stream));
  AsmArgs A;
  PYN_TRY(fill_args(c, A, PYN_FORM_OPERATOR));
  A.op_rule = rule;
  A.op_br = br;
  A.op_bc = bc;
  A.op_nterms = nterms;
  A.op_terms = dt;
  A.op_coef = dc;
  A.corners = c->d_eloc;
  A.out0 = c->d_eloc + ncor;
  PYN_TRY(launch_generic<true>(c, asm_knobs(), A, 1));
  PYN_HIP(hipMemcpyAsync(out, A.out0, n0 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}
