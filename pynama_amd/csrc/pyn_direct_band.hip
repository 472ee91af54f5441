// Direct solve of BANDED systems: LU with partial pivoting in band storage on the device (LAPACK gbtrf / gbtrs semantics).
//
// The reference's hard-wired default is `-ksp_type preonly -pc_type lu` (src/solver/ksp_solver.py:13-16, makefile:7).  The dense
// path (pyn_direct.hip) stops at 8,192 rows; the stiffness of a structured mesh in the library's lattice numbering (x fastest) is
// narrowly banded -- the band grows with the mesh face, not its volume -- so a banded factorisation solves the reference's own case
// sizes (2-D 50 x 50 and 3-D 9^3 at ngl 3, about 20 k rows) and far larger structured systems directly.  No reordering: the band is
// that of the existing numbering, kl / ku from the node graph.
//
// Storage (row-major, one band row per matrix row, int64 indices): row i holds columns [i - kl - NB + 1, i + kl + ku], i.e.
// W = 2 kl + ku + NB doubles; column c of row i is at AB[i W + c - i + kl + NB - 1].  The columns right of the diagonal are U
// (bandwidth kl + ku: the fill of the row interchanges); left of it the multipliers of L.  Interchanges are applied to L inside a
// panel of NB columns, as gbtrf does with its work array: a multiplier can then move up to NB - 1 further below the band, which is
// what the NB - 1 extra columns hold.  Between panels L is not permuted; the forward solve applies panel by panel
// w <- L_p^-1 P_p w on the window of NB + kl rows of panel p.
//
// Factorisation, per panel of NB = 64 columns (three launches, none per column):
//   (1) band_panel_kernel, ONE workgroup of 1024 threads: the (NB + kl) x NB panel column by column -- pivot search within the kl + 1
//       rows below the diagonal, interchange across the panel's columns, multipliers -- with rank-1 updates restricted to sub-blocks
//       of SB = 8 columns; after a sub-block, its 8 rows of U and the remaining panel columns below it are updated at once.  The
//       panel's interchanges are recorded as a gather over the window (perm).
//   (2) band_swap_trsm_kernel, one thread per trailing column c in [kb + NB, kb + NB + kl + ku): the window's interchanges as one
//       gather of the column, then U12 = L11^-1 A12.
//   (3) band_gemm_kernel: A22 -= L21 U12 on the kl x (kl + ku) window, 64 x 64 tiles through LDS (lu_gemm_kernel's shape).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pyn_internal.h"

namespace {

constexpr int BNB = 64;          // panel width = solve block
constexpr int BSB = 8;           // sub-block of the panel factorisation
constexpr int PANEL_THREADS = 1024;
constexpr int64_t BAND_MAX_KL = 12288;   // the panel's window permutation lives in LDS: (NB + kl) ints

struct Band {
  double* AB;
  int64_t n, W, kl, ku;
  __device__ __forceinline__ int64_t off() const { return kl + BNB - 1; }
  // address of (r, c); callers keep c - r in [-(kl + NB - 1), kl + ku]
  __device__ __forceinline__ double* at(int64_t r, int64_t c) const { return AB + r * W + (c - r + off()); }
  __device__ __forceinline__ bool upper_in(int64_t r, int64_t c) const { return c - r <= kl + ku; }
  // entries right of the band are zero and not stored (narrow bands: a panel is wider than kl + ku)
  __device__ __forceinline__ double ld(int64_t r, int64_t c) const { return upper_in(r, c) ? *at(r, c) : 0.0; }
  __device__ __forceinline__ void st(int64_t r, int64_t c, double v) const {
    if (upper_in(r, c)) *at(r, c) = v;
  }
};

// largest node distance below / above the diagonal of the (owned, ghost-free) node graph
__global__ void __launch_bounds__(256) band_width_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                         int64_t n_nodes, int* __restrict__ out) {
  __shared__ int sl[256], su[256];
  int lo = 0, up = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_nodes; i += (int64_t)gridDim.x * 256)
    for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int64_t d = (int64_t)colidx[e] - i;
      lo = max(lo, (int)max((int64_t)0, -d));
      up = max(up, (int)max((int64_t)0, d));
    }
  sl[threadIdx.x] = lo;
  su[threadIdx.x] = up;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sl[threadIdx.x] = max(sl[threadIdx.x], sl[threadIdx.x + s]);
      su[threadIdx.x] = max(su[threadIdx.x], su[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicMax(out, sl[0]);
    atomicMax(out + 1, su[0]);
  }
}

__global__ void band_from_bcsr_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const double* __restrict__ val,
                                      int64_t n_nodes, int b, Band B) {
  for (int64_t i = blockIdx.x; i < n_nodes; i += gridDim.x) {
    const int lo = rowptr[i], len = rowptr[i + 1] - lo;
    for (int e = threadIdx.x; e < len * b * b; e += blockDim.x) {
      const int p = e / (len * b), rem = e - p * len * b, k = rem / b, q = rem - k * b;
      *B.at(i * b + p, (int64_t)colidx[lo + k] * b + q) = val[((int64_t)lo * b) * b + e];
    }
  }
}

// (|a|, row) argmax over the workgroup, ties to the smaller row; NaN never wins (a NaN column reports best = -1: zero pivot)
__device__ void block_argmax(double best, int64_t bi, double* sv, int64_t* si, double* bout, int64_t* iout) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int s = 32; s > 0; s >>= 1) {
    const double ob = __shfl_xor(best, s);
    const int64_t oi = __shfl_xor(bi, s);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) {
    sv[wv] = best;
    si[wv] = bi;
  }
  __syncthreads();
  if (t == 0) {
    double b0 = sv[0];
    int64_t i0 = si[0];
    for (int w = 1; w < PANEL_THREADS / 64; ++w)
      if (sv[w] > b0 || (sv[w] == b0 && si[w] < i0)) {
        b0 = sv[w];
        i0 = si[w];
      }
    *bout = b0;
    *iout = i0;
  }
  __syncthreads();
}

// (1) the panel [kb, kb + nbp) in one workgroup; perm[q] (q < window): window row q of the permuted panel came from window row perm[q]
__global__ void __launch_bounds__(PANEL_THREADS) band_panel_kernel(Band B, int64_t kb, int nbp, int* __restrict__ perm,
                                                                   int* __restrict__ flag) {
  extern __shared__ int pl[];    // [NB + kl]
  __shared__ double sv[PANEL_THREADS / 64], prow[BNB], Us[BSB][BNB];
  __shared__ int64_t si[PANEL_THREADS / 64], piv_s;
  __shared__ double best_s;
  const int t = threadIdx.x;
  const int64_t n = B.n, kl = B.kl;
  const int64_t win = min((int64_t)BNB + kl, n - kb);
  for (int64_t q = t; q < win; q += PANEL_THREADS) pl[q] = (int)q;
  __syncthreads();
  for (int sb = 0; sb < nbp; sb += BSB) {
    const int sbe = min(sb + BSB, nbp);
    for (int j = sb; j < sbe; ++j) {
      const int64_t k = kb + j, rend = min(n, k + kl + 1);
      double best = -1.0;
      int64_t bi = k;
      for (int64_t r = k + t; r < rend; r += PANEL_THREADS) {
        const double a = fabs(*B.at(r, k));
        if (a > best) {
          best = a;
          bi = r;
        }
      }
      block_argmax(best, bi, sv, si, &best_s, &piv_s);
      const int64_t p = piv_s;
      if (t == 0) {
        if (!(best_s > 0.0) && *flag == 0) *flag = (int)(k + 1);   // singular (or NaN) column; the first one is reported
        const int a = pl[j];
        pl[j] = pl[p - kb];
        pl[p - kb] = a;
      }
      if (p != k && t < nbp) {   // interchange across the panel's columns
        const double a = B.ld(k, kb + t);
        B.st(k, kb + t, B.ld(p, kb + t));
        B.st(p, kb + t, a);
      }
      __syncthreads();
      if (t < nbp) prow[t] = B.ld(k, kb + t);
      __syncthreads();
      const double inv = 1.0 / prow[j];
      for (int64_t r = k + 1 + t; r < rend; r += PANEL_THREADS) {
        double* Lr = B.at(r, k);
        const double l = Lr[0] * inv;
        Lr[0] = l;
        for (int c = j + 1; c < sbe; ++c)
          if (B.upper_in(r, kb + c)) Lr[c - j] = fma(-l, prow[c], Lr[c - j]);
      }
      __syncthreads();
    }
    if (sbe < nbp) {
      // rows kb + sb .. kb + sbe - 1 of U for the panel's remaining columns: unit-lower solve with the sub-block's L
      const int c = sbe + t;
      if (c < nbp) {
        double u[BSB];
#pragma unroll
        for (int i = 0; i < BSB; ++i) u[i] = sb + i < sbe ? B.ld(kb + sb + i, kb + c) : 0.0;
#pragma unroll
        for (int i = 1; i < BSB; ++i)
#pragma unroll
          for (int m = 0; m < i; ++m)
            if (sb + i < sbe) u[i] = fma(-*B.at(kb + sb + i, kb + sb + m), u[m], u[i]);
#pragma unroll
        for (int i = 0; i < BSB; ++i)
          if (sb + i < sbe) {
            B.st(kb + sb + i, kb + c, u[i]);
            Us[i][c] = u[i];
          }
      }
      __syncthreads();
      // the rows below: A(r, c) -= L(r, sb..sbe) U(sb..sbe, c), one row per wave and step, lane = column
      const int cc = t & 63, rg = t >> 6;
      const int64_t rlim = min(n, kb + sbe + kl);
      if (sbe + cc < nbp)
        for (int64_t r = kb + sbe + rg; r < rlim; r += PANEL_THREADS / 64) {
          if (!B.upper_in(r, kb + sbe + cc)) continue;
          const double* Lr = B.at(r, kb + sb);
          double a = *B.at(r, kb + sbe + cc);
          for (int i = 0; i < sbe - sb; ++i) a = fma(-Lr[i], Us[i][sbe + cc], a);
          *B.at(r, kb + sbe + cc) = a;
        }
      __syncthreads();
    }
  }
  for (int64_t q = t; q < win; q += PANEL_THREADS) perm[q] = pl[q];
}

// (2) the window's interchanges on the trailing columns, then U12 = L11^-1 A12 (one thread per column, L11 at uniform addresses)
__global__ void __launch_bounds__(256) band_swap_trsm_kernel(Band B, int64_t kb, int nbp, const int* __restrict__ perm) {
  __shared__ int top[BNB];
  __shared__ int low_dst[BNB], low_src[BNB];
  __shared__ int nlow;
  const int t = threadIdx.x;
  const int64_t n = B.n, win = min((int64_t)BNB + B.kl, n - kb);
  if (t == 0) nlow = 0;
  if (t < nbp) top[t] = perm[t];
  __syncthreads();
  for (int64_t q = nbp + t; q < win; q += 256) {   // rows below the panel that received a panel row
    const int s = perm[q];
    if (s != q) {
      const int m = atomicAdd(&nlow, 1);
      low_dst[m] = (int)q;
      low_src[m] = s;
    }
  }
  __syncthreads();
  const int64_t c = kb + nbp + (int64_t)blockIdx.x * 256 + t;
  if (c >= min(n, kb + nbp + B.kl + B.ku)) return;
  double u[BNB];
#pragma unroll
  for (int j = 0; j < BNB; ++j) {
    const int64_t r = kb + (j < nbp ? top[j] : 0);
    u[j] = (j < nbp && B.upper_in(r, c)) ? *B.at(r, c) : 0.0;
  }
  for (int m = 0; m < nlow; ++m) {   // sources are panel rows, read before any of them is written
    const int64_t r = kb + low_dst[m], s = kb + low_src[m];
    if (B.upper_in(r, c)) *B.at(r, c) = B.upper_in(s, c) ? *B.at(s, c) : 0.0;
  }
#pragma unroll
  for (int i = 1; i < BNB; ++i) {
    if (i < nbp) {
      const double* Li = B.at(kb + i, kb);
      double a = u[i];
#pragma unroll
      for (int j = 0; j < i; ++j) a = fma(-Li[j], u[j], a);
      u[i] = a;
    }
  }
#pragma unroll
  for (int j = 0; j < BNB; ++j)
    if (j < nbp && B.upper_in(kb + j, c)) *B.at(kb + j, c) = u[j];
}

// (3) A22 -= L21 U12: rows [kb + nbp, kb + nbp + kl), columns [kb + nbp, kb + nbp + kl + ku); 64 x 64 tile per workgroup, 4 x 4 per thread
__global__ void __launch_bounds__(256) band_gemm_kernel(Band B, int64_t kb, int nbp, int64_t r_end, int64_t c_end) {
  __shared__ double As[64][BNB + 1];
  __shared__ double Bs[BNB][64];
  const int64_t i0 = kb + nbp + (int64_t)blockIdx.y * 64, c0 = kb + nbp + (int64_t)blockIdx.x * 64;
  if (c0 - (i0 + 63) > B.kl + B.ku) return;   // the whole tile right of the band
  const int t = threadIdx.x;
  for (int e = t; e < 64 * BNB; e += 256) {
    const int r = e / BNB, k = e % BNB;
    As[r][k] = (i0 + r < r_end && k < nbp) ? *B.at(i0 + r, kb + k) : 0.0;
  }
  for (int e = t; e < BNB * 64; e += 256) {
    const int k = e / 64, cc = e % 64;
    const int64_t c = c0 + cc;
    Bs[k][cc] = (c < c_end && k < nbp && B.upper_in(kb + k, c)) ? *B.at(kb + k, c) : 0.0;
  }
  __syncthreads();
  const int tx = t & 15, ty = t >> 4;
  double acc[4][4] = {};
#pragma unroll 8
  for (int k = 0; k < BNB; ++k) {
    double a[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = As[ty * 4 + r][k];
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = Bs[k][tx + 16 * q];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[r][q] = fma(a[r], b[q], acc[r][q]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t i = i0 + ty * 4 + r, c = c0 + tx + 16 * q;
      if (i < r_end && c < c_end && B.upper_in(i, c)) *B.at(i, c) -= acc[r][q];
    }
}

// value of lane k (compile-time constant after unrolling) in every lane
__device__ __forceinline__ double lane_bcast(double v, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

// forward step of panel p: window rows q of (P_p w) -- the block's nbp rows solved with L11 (redundantly in wave 0 of every
// workgroup, lane = row) into z, rows nbp .. win - 1 minus L21 y into dst.  Rows [kb, kb + kl) of w are the previous panel's dst
// (src), rows from kb + kl on have not been touched yet and are read from b.  src is only read: workgroups that start late still
// find the unpermuted values.
__global__ void __launch_bounds__(256) band_fwd_kernel(Band B, int64_t kb, int nbp, const int* __restrict__ perm, const double* __restrict__ src,
                                                       const double* __restrict__ b, double* __restrict__ dst, double* __restrict__ z) {
  __shared__ double ws[64];
  const int t = threadIdx.x, lane = t & 63;
  const int64_t n = B.n, win = min((int64_t)BNB + B.kl, n - kb), fresh = kb + B.kl;
  auto rd = [&](int64_t g) { return g < fresh ? src[g] : b[g]; };
  if (t < 64) {
    const int r = min(lane, nbp - 1);
    double R[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) R[j] = j < r ? *B.at(kb + r, kb + j) : 0.0;
    double wv = rd(kb + perm[r]);
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const double wk = lane_bcast(wv, k);
      if (lane > k && k < nbp) wv = fma(-R[k], wk, wv);
    }
    ws[lane] = lane < nbp ? wv : 0.0;
  }
  __syncthreads();
  const int sub = t >> 4, q4 = t & 15;
  const double s0 = ws[4 * q4], s1 = ws[4 * q4 + 1], s2 = ws[4 * q4 + 2], s3 = ws[4 * q4 + 3];
  for (int64_t q = nbp + (int64_t)blockIdx.x * 16 + sub; q < win; q += (int64_t)gridDim.x * 16) {
    const double* r = B.at(kb + q, kb + 4 * q4);
    double a = 0.0;
    if (4 * q4 + 3 < nbp) a = fma(r[3], s3, fma(r[2], s2, fma(r[1], s1, r[0] * s0)));
    else
      for (int j = 0; j < 4; ++j)
        if (4 * q4 + j < nbp) a = fma(r[j], ws[4 * q4 + j], a);
    a += __shfl_xor(a, 8, 16);
    a += __shfl_xor(a, 4, 16);
    a += __shfl_xor(a, 2, 16);
    a += __shfl_xor(a, 1, 16);
    if (q4 == 0) dst[kb + q] = rd(kb + perm[q]) - a;
  }
  if (blockIdx.x == 0 && t < nbp) z[kb + t] = ws[t];
}

// backward step of the block [kb, kb + nb): U11 solve in wave 0 of every workgroup, then the rows above within the band (kl + ku)
// minus U12 x; the solved block goes to out (w[kb ..] stays as it was for workgroups that start late)
__global__ void __launch_bounds__(256) band_bwd_kernel(Band B, int64_t kb, int nb, double* __restrict__ w, double* __restrict__ out) {
  __shared__ double ws[64];
  const int t = threadIdx.x, lane = t & 63;
  const int64_t kw = B.kl + B.ku;
  if (t < 64) {
    const int r = min(lane, nb - 1);
    double R[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) R[j] = (j >= r && j < nb && j - r <= kw) ? *B.at(kb + r, kb + j) : 0.0;
    double wv = w[kb + r];
#pragma unroll
    for (int k = 63; k >= 0; --k) {
      if (lane == k && k < nb) wv = wv / R[k];
      const double wk = lane_bcast(wv, k);
      if (lane < k && k < nb) wv = fma(-R[k], wk, wv);
    }
    ws[lane] = lane < nb ? wv : 0.0;
  }
  __syncthreads();
  const int64_t r0 = max((int64_t)0, kb - kw);
  const int sub = t >> 4, q4 = t & 15;
  for (int64_t i = r0 + (int64_t)blockIdx.x * 16 + sub; i < kb; i += (int64_t)gridDim.x * 16) {
    double a = 0.0;
    for (int j = 4 * q4; j < 4 * q4 + 4; ++j)
      if (j < nb && kb + j - i <= kw) a = fma(*B.at(i, kb + j), ws[j], a);
    a += __shfl_xor(a, 8, 16);
    a += __shfl_xor(a, 4, 16);
    a += __shfl_xor(a, 2, 16);
    a += __shfl_xor(a, 1, 16);
    if (q4 == 0) w[i] -= a;
  }
  if (blockIdx.x == 0 && t < nb) out[kb + t] = ws[t];
}

// out[0] = ||b - w||^2, out[1] = ||b||^2 (one workgroup)
__global__ void __launch_bounds__(1024) band_resid_kernel(const double* __restrict__ w, const double* __restrict__ b, int64_t n, double* __restrict__ out) {
  __shared__ double sr[1024], sb[1024];
  double r = 0.0, q = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const double d = b[i] - w[i];
    r = fma(d, d, r);
    q = fma(b[i], b[i], q);
  }
  sr[threadIdx.x] = r;
  sb[threadIdx.x] = q;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sr[threadIdx.x] += sr[threadIdx.x + s];
      sb[threadIdx.x] += sb[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sr[0];
    out[1] = sb[0];
  }
}

struct BandShape {
  int64_t n = 0, kl = 0, ku = 0, W = 0, npanel = 0, band_bytes = 0, perm_bytes = 0, bytes = 0;
};

int band_check(pyn_ctx* c, int mat_id, const char* what) {
  PYN_TRY(pyn_check_mat(c, mat_id, what));
  const DMat& A = c->mats[mat_id];
  PYN_CHECK(A.br == A.bc, "%s: the banded LU needs a square block size (br %d != bc %d)", what, A.br, A.bc);
  PYN_CHECK(!A.rhs_compact, "%s: a compact imposed-column matrix (pyn_mat_create_rhs) is a right-hand-side operator, not a system matrix", what);
  PYN_CHECK(c->nranks == 1 && !c->detached, "%s: the banded LU runs on one rank (this context has %d)", what, c->nranks);
  PYN_CHECK(c->n_ghost == 0, "%s: the banded LU needs a context without ghost nodes (%lld here)", what, (long long)c->n_ghost);
  PYN_CHECK(c->d_rowptr && c->n_owned > 0, "%s: no node graph (pyn_csr_symbolic first)", what);
  return PYN_OK;
}

int band_shape(pyn_ctx* c, const DMat& A, BandShape* s) {
  int h[2] = {0, 0};
  PYN_HIP(hipMemsetAsync(c->d_flag, 0, 2 * sizeof(int), c->stream));
  band_width_kernel<<<(int)std::min<int64_t>((c->n_owned + 255) / 256, 1024), 256, 0, c->stream>>>(c->d_rowptr, c->d_colidx, c->n_owned, c->d_flag);
  PYN_HIP(hipMemcpyAsync(h, c->d_flag, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  PYN_HIP(hipGetLastError());
  const int b = A.br;
  s->n = c->n_owned * b;
  s->kl = (int64_t)h[0] * b + b - 1;
  s->ku = (int64_t)h[1] * b + b - 1;
  s->W = 2 * s->kl + s->ku + BNB;
  s->npanel = (s->n + BNB - 1) / BNB;
  s->band_bytes = s->n * s->W * (int64_t)sizeof(double);
  s->perm_bytes = s->npanel * (BNB + s->kl) * (int64_t)sizeof(int);
  s->bytes = s->band_bytes + s->perm_bytes;
  return PYN_OK;
}

// factors of A in band storage, cached in the matrix until its values change
int band_factor(pyn_ctx* c, DMat& A, const BandShape& s, int64_t max_bytes) {
  if (A.band_valid && A.band_n == s.n && A.band_kl == s.kl && A.band_ku == s.ku) return PYN_OK;
  PYN_CHECK(s.kl <= BAND_MAX_KL, "banded LU: lower half-bandwidth %lld exceeds the panel limit %lld (reorder the mesh or use the Krylov solvers)",
            (long long)s.kl, (long long)BAND_MAX_KL);
  PYN_CHECK(s.bytes <= max_bytes, "banded LU: the factors take %lld bytes, above the cap max_bytes = %lld (kl %lld, ku %lld, %lld rows)",
            (long long)s.bytes, (long long)max_bytes, (long long)s.kl, (long long)s.ku, (long long)s.n);
  const bool fits = A.band && A.band_n == s.n && A.band_kl == s.kl && A.band_ku == s.ku;
  if (!fits) {
    A.release_band();
    size_t fr = 0, tot = 0;
    PYN_HIP(hipMemGetInfo(&fr, &tot));
    PYN_CHECK((size_t)s.bytes + ((size_t)64 << 20) <= fr,
              "banded LU: the factors take %lld bytes, more than the free device memory (%lld bytes; kl %lld, ku %lld, %lld rows)",
              (long long)s.bytes, (long long)fr, (long long)s.kl, (long long)s.ku, (long long)s.n);
    PYN_HIP(A.band.alloc((size_t)(s.n * s.W)));
    PYN_HIP(A.band_perm.alloc((size_t)(s.npanel * (BNB + s.kl)) + 1));
    A.band_n = s.n;
    A.band_kl = s.kl;
    A.band_ku = s.ku;
  }
  hipStream_t st = c->stream;
  const Band B{A.band, s.n, s.W, s.kl, s.ku};
  int* flag = A.band_perm + s.npanel * (BNB + s.kl);
  PYN_HIP(hipMemsetAsync(A.band, 0, (size_t)s.band_bytes, st));
  PYN_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  band_from_bcsr_kernel<<<(int)std::min<int64_t>(c->n_owned, 4096), 256, 0, st>>>(c->d_rowptr, c->d_colidx, A.val, c->n_owned, A.br, B);
  const size_t lds = (size_t)(BNB + s.kl) * sizeof(int);
  for (int64_t p = 0; p < s.npanel; ++p) {
    const int64_t kb = p * BNB;
    const int nbp = (int)std::min<int64_t>(BNB, s.n - kb);
    int* perm = A.band_perm + p * (BNB + s.kl);
    band_panel_kernel<<<1, PANEL_THREADS, lds, st>>>(B, kb, nbp, perm, flag);
    const int64_t c_end = std::min(s.n, kb + nbp + s.kl + s.ku), r_end = std::min(s.n, kb + nbp + s.kl);
    const int64_t nc = c_end - (kb + nbp), nr = r_end - (kb + nbp);
    if (nc > 0) {
      band_swap_trsm_kernel<<<(int)((nc + 255) / 256), 256, 0, st>>>(B, kb, nbp, perm);
      if (nr > 0) band_gemm_kernel<<<dim3((int)((nc + 63) / 64), (int)((nr + 63) / 64)), 256, 0, st>>>(B, kb, nbp, r_end, c_end);
    }
  }
  int h = 0;
  PYN_HIP(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  PYN_HIP(hipStreamSynchronize(st));
  PYN_HIP(hipGetLastError());
  PYN_CHECK(h == 0, "banded LU: zero pivot in column %d of %lld (the matrix is singular)", h - 1, (long long)s.n);
  A.band_valid = true;
  return PYN_OK;
}

}  // namespace

extern "C" int pyn_direct_band_info(pyn_ctx* c, int mat_id, int64_t* kl, int64_t* ku, int64_t* bytes) {
  PYN_TRY(band_check(c, mat_id, "pyn_direct_band_info"));
  PYN_CHECK(kl && ku && bytes, "NULL argument");
  PYN_HIP(hipSetDevice(c->device));
  BandShape s;
  PYN_TRY(band_shape(c, c->mats[mat_id], &s));
  *kl = s.kl;
  *ku = s.ku;
  *bytes = s.bytes;
  return PYN_OK;
}

extern "C" int pyn_solve_direct_band(pyn_ctx* c, int mat_id, int bv, int xv, int64_t max_bytes, pyn_solve_info* info) {
  PYN_TRY(band_check(c, mat_id, "pyn_solve_direct_band"));
  PYN_TRY(pyn_check_vec(c, bv, "pyn_solve_direct_band b"));
  PYN_TRY(pyn_check_vec(c, xv, "pyn_solve_direct_band x"));
  PYN_CHECK(info, "NULL argument");
  PYN_CHECK(bv != xv, "b and x must differ");
  DMat& A = c->mats[mat_id];
  PYN_CHECK(c->vecs[bv].bs == A.br && c->vecs[xv].bs == A.br, "vector block size mismatch");
  PYN_HIP(hipSetDevice(c->device));
  memset(info, 0, sizeof(*info));
  BandShape s;
  PYN_TRY(band_shape(c, A, &s));
  const int64_t n = s.n;
  PYN_TRY(pyn_ensure_work(c, (size_t)4 * n * sizeof(double)));
  hipStream_t st = c->stream;
  PYN_HIP(hipEventRecord(c->ev0, st));
  PYN_TRY(band_factor(c, A, s, max_bytes));
  const Band B{A.band, n, s.W, s.kl, s.ku};
  double* b = c->vecs[bv].d;
  double* x = c->vecs[xv].d;
  double* pp[2] = {c->d_work, c->d_work + n};
  double* z = c->d_work + 2 * n;
  const double* src = b;
  for (int64_t p = 0; p < s.npanel; ++p) {   // forward: z = L^-1 P b, panel by panel (src / dst alternate)
    const int64_t kb = p * BNB;
    const int nbp = (int)std::min<int64_t>(BNB, n - kb);
    const int64_t rows = std::min<int64_t>(BNB + s.kl, n - kb) - nbp;
    double* dst = pp[p & 1];
    band_fwd_kernel<<<(int)std::max<int64_t>(1, std::min<int64_t>((rows + 15) / 16, 1024)), 256, 0, st>>>(
        B, kb, nbp, A.band_perm + p * (BNB + s.kl), src, b, dst, z);
    src = dst;
  }
  for (int64_t kb = ((n - 1) / BNB) * BNB; kb >= 0; kb -= BNB) {   // backward: blocks of z solved into x, the rows above updated in z
    const int nb = (int)std::min<int64_t>(BNB, n - kb);
    const int64_t rows = kb - std::max<int64_t>(0, kb - s.kl - s.ku);
    band_bwd_kernel<<<(int)std::max<int64_t>(1, std::min<int64_t>((rows + 15) / 16, 1024)), 256, 0, st>>>(B, kb, nb, z, x);
  }
  PYN_HIP(hipEventRecord(c->ev1, st));
  double* w = c->d_work + 3 * n;   // true residual through the sparse matrix
  PYN_TRY(pyn_spmv_raw(c, A, x, w));
  band_resid_kernel<<<1, 1024, 0, st>>>(w, b, n, c->d_scal);
  PYN_HIP(hipMemcpyAsync(c->h_scal, c->d_scal, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  PYN_HIP(hipStreamSynchronize(st));
  PYN_HIP(hipGetLastError());
  const double rr = c->h_scal[0], bb = c->h_scal[1];
  float ms = 0;
  PYN_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  info->solve_ms = ms;
  info->iters = 1;                       // PETSc reports one "iteration" for preonly
  info->true_resid = bb > 0 ? sqrt(rr / bb) : sqrt(rr);
  info->rnorm = sqrt(rr);
  info->rnorm0 = sqrt(bb);
  info->reason = (info->true_resid == info->true_resid) ? PYN_CONVERGED_ITS : PYN_DIVERGED_NANORINF;
  c->timers[PYN_T_SOLVE] = ms;
  return PYN_OK;
}
