// Explicit Runge-Kutta vector passes of TsSolver (pynama_amd/solver/ts_solver.py), the time integrator of
// BaseProblem.startSolver (the reference's TsSolver(PETSc.TS): -ts_type rk -ts_rk_type 5bs, adaptive, MATCHSTEP).
//
// Two kernels, both over the owned entries of a vector (n_owned*bs; ghosts are left alone), on the context stream:
//  * maxpy_kernel:       y = x + sum_j w_j v_j, j < m <= 8     -- the stage vectors Y_i = X + h sum_j a_ij K_j, and the
//                        roll-back of a rejected step (w = -h b)
//  * step_finish_kernel: x += sum_j h b_j k_j in place; optionally the per-block partial sums of
//                        (|d_i| / (atol + rtol max(|x_i|, |x_i + d_i|)))^2 and of the entry count, d = sum_j h (bhat_j - b_j) k_j
//                        over the UPDATED x -- finished by pyn_reduce_host (one block, all-reduced over the ranks): the weighted
//                        RMS norm is the only device->host read of a step.
// The stage pointers and weights travel by value in the kernel arguments.  Per entry the sum runs in fixed j order with fma.
// Entries go in pairs through 16-byte loads and stores when every pointer is 16-byte aligned, the rest (an odd tail, or all of
// it otherwise) one by one.  y may be x: no __restrict__ on the state.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "pyn_internal.h"

namespace {

struct StageArgs {
  const double* v[PYN_TS_MAX_STAGES];
  double w[PYN_TS_MAX_STAGES];   // maxpy weights, or h b_j
  double d[PYN_TS_MAX_STAGES];   // h (bhat_j - b_j) (finish with estimate)
};

inline int ts_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 511) / 512, PYN_MAX_PARTIALS)); }

// entries [0, 2 nv) as nv pairs, [2 nv, n) one by one
template <int M>
__global__ void __launch_bounds__(256) maxpy_kernel(double* y, const double* x, StageArgs a, int64_t nv, int64_t n) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = t0; i < nv; i += stride) {
    double2 r = reinterpret_cast<const double2*>(x)[i];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double2 v = reinterpret_cast<const double2*>(a.v[j])[i];
      r.x = fma(a.w[j], v.x, r.x);
      r.y = fma(a.w[j], v.y, r.y);
    }
    reinterpret_cast<double2*>(y)[i] = r;
  }
  for (int64_t i = 2 * nv + t0; i < n; i += stride) {
    double r = x[i];
#pragma unroll
    for (int j = 0; j < M; ++j) r = fma(a.w[j], a.v[j][i], r);
    y[i] = r;
  }
}

__device__ inline double wrms_term(double xn, double d, double atol, double rtol) {
  const double e = fabs(d) / (atol + rtol * fmax(fabs(xn), fabs(xn + d)));
  return e * e;
}

// part[0..grid): sum of the error terms, part[PYN_MAX_PARTIALS + 0..grid): entry count (EST only)
template <int M, bool EST>
__global__ void __launch_bounds__(256) step_finish_kernel(double* x, StageArgs a, int64_t nv, int64_t n, double atol, double rtol,
                                                          double* __restrict__ part) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  double acc = 0.0, cnt = 0.0;
  for (int64_t i = t0; i < nv; i += stride) {
    double2 r = reinterpret_cast<const double2*>(x)[i];
    double2 d = make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double2 k = reinterpret_cast<const double2*>(a.v[j])[i];
      r.x = fma(a.w[j], k.x, r.x);
      r.y = fma(a.w[j], k.y, r.y);
      if (EST) {
        d.x = fma(a.d[j], k.x, d.x);
        d.y = fma(a.d[j], k.y, d.y);
      }
    }
    reinterpret_cast<double2*>(x)[i] = r;
    if (EST) {
      acc += wrms_term(r.x, d.x, atol, rtol) + wrms_term(r.y, d.y, atol, rtol);
      cnt += 2.0;
    }
  }
  for (int64_t i = 2 * nv + t0; i < n; i += stride) {
    double r = x[i], d = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double k = a.v[j][i];
      r = fma(a.w[j], k, r);
      if (EST) d = fma(a.d[j], k, d);
    }
    x[i] = r;
    if (EST) {
      acc += wrms_term(r, d, atol, rtol);
      cnt += 1.0;
    }
  }
  if (EST) {
    block_partial(acc, part);
    __syncthreads();
    block_partial(cnt, part + PYN_MAX_PARTIALS);
  }
}

// checks shared by both entries: x and the m stage vectors exist and agree in block size; pairs only if all are 16-byte aligned
int stage_args(pyn_ctx* c, int x, int m, const int* ids, const char* what, StageArgs& a, int64_t& n, int64_t& nv) {
  PYN_TRY(pyn_check_vec(c, x, what));
  PYN_CHECK(m >= 0 && m <= PYN_TS_MAX_STAGES, "%s: %d stage vectors, at most %d", what, m, PYN_TS_MAX_STAGES);
  PYN_CHECK(m == 0 || ids, "%s: ids is NULL", what);
  const int bs = c->vecs[x].bs;
  bool pairs = ((uintptr_t)c->vecs[x].d.get() & 15) == 0;
  for (int j = 0; j < PYN_TS_MAX_STAGES; ++j) {
    a.v[j] = nullptr;
    a.w[j] = a.d[j] = 0.0;
  }
  for (int j = 0; j < m; ++j) {
    PYN_TRY(pyn_check_vec(c, ids[j], what));
    PYN_CHECK(c->vecs[ids[j]].bs == bs, "%s: stage vector %d has block size %d, x has %d", what, j, c->vecs[ids[j]].bs, bs);
    a.v[j] = c->vecs[ids[j]].d;
    pairs = pairs && ((uintptr_t)a.v[j] & 15) == 0;
  }
  n = c->n_owned * bs;
  nv = pairs ? n / 2 : 0;
  return PYN_OK;
}

}  // namespace

extern "C" int pyn_vec_maxpy(pyn_ctx* c, int y, int x, int m, const int* ids, const double* w) {
  StageArgs a;
  int64_t n = 0, nv = 0;
  PYN_TRY(stage_args(c, x, m, ids, "pyn_vec_maxpy", a, n, nv));
  PYN_TRY(pyn_check_vec(c, y, "pyn_vec_maxpy y"));
  PYN_CHECK(c->vecs[y].bs == c->vecs[x].bs, "pyn_vec_maxpy: block size mismatch (y %d, x %d)", c->vecs[y].bs, c->vecs[x].bs);
  PYN_CHECK(m == 0 || w, "pyn_vec_maxpy: w is NULL");
  if (((uintptr_t)c->vecs[y].d.get() & 15) != 0) nv = 0;
  for (int j = 0; j < m; ++j) a.w[j] = w[j];
  double* yd = c->vecs[y].d;
  const double* xd = c->vecs[x].d;
  const int g = ts_grid(n);
  hipStream_t s = c->stream;
  switch (m) {
#define PYN_MAXPY(M) \
  case M: maxpy_kernel<M><<<g, 256, 0, s>>>(yd, xd, a, nv, n); break
    PYN_MAXPY(0); PYN_MAXPY(1); PYN_MAXPY(2); PYN_MAXPY(3); PYN_MAXPY(4);
    PYN_MAXPY(5); PYN_MAXPY(6); PYN_MAXPY(7); PYN_MAXPY(8);
#undef PYN_MAXPY
  }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

extern "C" int pyn_ts_step_finish(pyn_ctx* c, int x, int m, const int* ids, const double* hb, const double* hd, double atol,
                                  double rtol, double* wnorm) {
  StageArgs a;
  int64_t n = 0, nv = 0;
  PYN_TRY(stage_args(c, x, m, ids, "pyn_ts_step_finish", a, n, nv));
  PYN_CHECK(m == 0 || hb, "pyn_ts_step_finish: hb is NULL");
  PYN_CHECK(!wnorm || m == 0 || hd, "pyn_ts_step_finish: an error estimate needs hd");
  for (int j = 0; j < m; ++j) {
    PYN_CHECK(ids[j] != x, "pyn_ts_step_finish: stage vector %d is x", j);
    a.w[j] = hb[j];
    if (wnorm) a.d[j] = hd[j];
  }
  double* xd = c->vecs[x].d;
  const int g = ts_grid(n);
  hipStream_t s = c->stream;
  switch (m * 2 + (wnorm ? 1 : 0)) {
#define PYN_FINISH(M)                                                                                   \
  case 2 * M: step_finish_kernel<M, false><<<g, 256, 0, s>>>(xd, a, nv, n, atol, rtol, c->d_part); break; \
  case 2 * M + 1: step_finish_kernel<M, true><<<g, 256, 0, s>>>(xd, a, nv, n, atol, rtol, c->d_part); break
    PYN_FINISH(0); PYN_FINISH(1); PYN_FINISH(2); PYN_FINISH(3); PYN_FINISH(4);
    PYN_FINISH(5); PYN_FINISH(6); PYN_FINISH(7); PYN_FINISH(8);
#undef PYN_FINISH
  }
  PYN_HIP(hipGetLastError());
  if (!wnorm) return PYN_OK;
  double sums[2];
  PYN_TRY(pyn_reduce_host(c, 2, g, 0, sums));   // finishing block + all-reduce of (sum, count) over the communicator
  *wnorm = sums[1] > 0.0 ? sqrt(sums[0] / sums[1]) : 0.0;
  return PYN_OK;
}
