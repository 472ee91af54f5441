// Immersed boundary on the device: discrete-delta interpolation to Lagrangian markers, spreading back to the lattice, and the
// implicit velocity correction of Wu & Shu -- the roles of the reference's ImmersedBoundaryStatic.buildIBMMatrix /
// computeVelocityCorrection (src/cases/immersed_boundary.py) and of the marker bookkeeping of src/domain/immersed_body.py, which
// loop over markers on the host and fill PETSc matrices H, S and H S.  Here nothing is assembled as a sparse matrix:
//
//   W_kj = prod_d phi((x_jd - X_kd) / h_d)      phi: Peskin's 4-point or Roma's 3-point kernel, recomputed where it is used
//   (H u)_k = sum_j W_kj u_j                    16 lanes per marker (2-D) / one wave per marker (3-D), fixed shuffle tree
//   (S q)_j = sum_k W_kj c_k q_k,  c_k = dl_k / prod_d h_d     node-major lists: (node, marker) pairs sorted by node with a stable
//                                               radix sort, one thread per affected node sums its run in marker order -- no atomics
//   A = H S,  A_kl = c_l prod_d g_d(k, l),  g_d = sum_i phi(r_ik) phi(r_il) over the lattice lines both stencils hold
//                                               (separable closed form, one thread per entry), factored once per marker position
//                                               by the dense LU of pyn_direct.hip
//   correction: A q = U_B - H u per component with the cached factors, u += S q; then H u = U_B.
//
// The grid must be a uniform node lattice (structured box mesh of ngl 2 or 3, no jitter, one rank): checked against the device
// coordinates.  Every stencil must stay inside the lattice's second-outermost node layer, so imposed boundary nodes never change.
// Sums have a fixed order everywhere: repeated calls give identical bits.
#include <hipcub/hipcub.hpp>
#include <hipcub/iterator/counting_input_iterator.hpp>

#include <cmath>
#include <vector>

#include "pyn_internal.h"

struct IbmState {
  bool valid = false;
  bool lattice_ok = false;      // the device coordinates were verified against lower / h (kept until they change)
  int kernel = 0, dim = 0, width = 0, ns = 0;   // ns = width^dim stencil nodes per marker
  int64_t n = 0, naff = 0, builds = 0;
  int N[3] = {1, 1, 1};
  double lower[3] = {0, 0, 0}, h[3] = {1, 1, 1};
  int64_t cap_n = 0, cap_pairs = 0;
  DevBuf<double> X;             // [n][dim]
  DevBuf<double> cw;            // [n] c_k = dl_k / prod h
  DevBuf<int32_t> base;         // [n][dim] first lattice line of the marker's stencil per axis
  DevBuf<double> A;             // [n][n] row-major
  DevBuf<double> lu;            // its factors
  DevBuf<int> piv;              // [2 n + 1]
  DevBuf<double> rq;            // [dim][n] residual, [dim][n] forcing, [n] solve scratch, [n][dim] host-layout staging
  DevBuf<int32_t> key0, key1, val0, val1;   // (node, pair) before / after the sort
  DevBuf<int32_t> flag;         // [pairs] run heads
  DevBuf<int32_t> segptr;       // [naff + 1] first sorted pair of every affected node
  DevBuf<int32_t> nodes;        // [naff]
  DevBuf<int32_t> smk;          // [pairs] marker of the sorted pair
  DevBuf<double> sw;            // [pairs] W_kj c_k of the sorted pair
  DevBuf<unsigned char> tmp;    // hipCUB scratch (grown on demand)
  DevBuf<int64_t> d_cnt;
};

void IbmStateDelete::operator()(IbmState* s) const { delete s; }

namespace {

struct IbmGrid {
  int dim, n;
  int N[3];
  double lower[3], h[3];
};

// phi(r), r in units of h.  KERN 0: Peskin's 4-point kernel (the reference's fourGrid), 1: Roma's 3-point kernel (threeGrid)
template <int KERN>
__device__ __forceinline__ double ibm_phi(double r) {
  const double a = fabs(r);
  if (KERN == 0) {
    if (a < 1.0) return (3.0 - 2.0 * a + sqrt(1.0 + 4.0 * a - 4.0 * a * a)) * 0.125;
    if (a < 2.0) return (5.0 - 2.0 * a - sqrt(-7.0 + 12.0 * a - 4.0 * a * a)) * 0.125;
    return 0.0;
  }
  if (a <= 0.5) return (1.0 + sqrt(1.0 - 3.0 * a * a)) / 3.0;
  if (a < 1.5) {
    const double b = 1.0 - a;
    return (5.0 - 3.0 * a - sqrt(1.0 - 3.0 * b * b)) / 6.0;
  }
  return 0.0;
}

// weight of lattice line i of axis d for a marker at coordinate X: phi(((lower + i h) - X) / h)
template <int KERN>
__device__ __forceinline__ double ibm_w1(const IbmGrid& G, int d, int i, double X) {
  const double x = __dadd_rn(G.lower[d], __dmul_rn((double)i, G.h[d]));
  return ibm_phi<KERN>(__dsub_rn(x, X) / G.h[d]);
}

// the local nodes are lower + i h, numbered x fastest?  *bad = 1 otherwise (plain store: every writer writes the same value)
__global__ void ibm_lattice_check_kernel(IbmGrid G, const double* __restrict__ xyz, int64_t n_node, int* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_node) return;
  int64_t r = j;
  bool off = false;
  for (int d = 0; d < G.dim; ++d) {
    const int i = (int)(r % G.N[d]);
    r /= G.N[d];
    const double x = G.lower[d] + (double)i * G.h[d];
    const double tol = 1e-12 * G.h[d] * (double)(G.N[d] - 1);
    if (!(fabs(xyz[j * G.dim + d] - x) <= tol)) off = true;
  }
  if (off) *bad = 1;
}

// A_kl = c_l prod_d sum_i phi(r_ik) phi(r_il): one thread per entry
template <int KERN>
__global__ void __launch_bounds__(256) ibm_matrix_kernel(IbmGrid G, const double* __restrict__ X, const double* __restrict__ cw,
                                                         const int32_t* __restrict__ base, double* __restrict__ A) {
  constexpr int W = KERN == 0 ? 4 : 3;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)G.n * G.n) return;
  const int k = (int)(t / G.n), l = (int)(t - (int64_t)k * G.n);
  double a = cw[l];
  for (int d = 0; d < G.dim; ++d) {
    const int bk = base[k * G.dim + d], bl = base[l * G.dim + d];
    const double Xk = X[k * G.dim + d], Xl = X[l * G.dim + d];
    double g = 0.0;
#pragma unroll
    for (int o = 0; o < W; ++o) {
      const int i = bk + o;
      if (i >= bl && i < bl + W) g = fma(ibm_w1<KERN>(G, d, i, Xk), ibm_w1<KERN>(G, d, i, Xl), g);
    }
    a *= g;
  }
  A[t] = a;
}

// (node, pair) of every stencil entry, pair = marker * ns + s, s = ox + W (oy + W oz)
__global__ void ibm_pairs_kernel(IbmGrid G, int W, int ns, const int32_t* __restrict__ base, int32_t* __restrict__ key,
                                 int32_t* __restrict__ val) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)G.n * ns) return;
  const int k = (int)(p / ns);
  int s = (int)(p - (int64_t)k * ns);
  int64_t node = 0, stride = 1;
  for (int d = 0; d < G.dim; ++d) {
    node += (int64_t)(base[k * G.dim + d] + s % W) * stride;
    s /= W;
    stride *= G.N[d];
  }
  key[p] = (int32_t)node;
  val[p] = (int32_t)p;
}

// the sorted pairs: marker, W_kj c_k, and whether the pair starts a node's run
template <int KERN>
__global__ void ibm_sorted_kernel(IbmGrid G, int ns, const double* __restrict__ X, const double* __restrict__ cw,
                                  const int32_t* __restrict__ base, const int32_t* __restrict__ key, const int32_t* __restrict__ val,
                                  int32_t* __restrict__ smk, double* __restrict__ sw, int32_t* __restrict__ flag) {
  constexpr int W = KERN == 0 ? 4 : 3;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)G.n * ns) return;
  const int pair = val[p], k = pair / ns;
  int s = pair - k * ns;
  double w = cw[k];
  for (int d = 0; d < G.dim; ++d) {
    w *= ibm_w1<KERN>(G, d, base[k * G.dim + d] + s % W, X[k * G.dim + d]);
    s /= W;
  }
  smk[p] = k;
  sw[p] = w;
  flag[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}

__global__ void ibm_nodes_kernel(const int32_t* __restrict__ key, int32_t* __restrict__ segptr, int64_t naff, int32_t total,
                                 int32_t* __restrict__ nodes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < naff) nodes[i] = key[segptr[i]];
  if (i == naff) segptr[naff] = total;
}

// H u at the markers.  2-D: 16 lanes per marker (lane = ox + 4 oy of the stencil), 3-D: 64 lanes (ox + 4 oy + 16 oz); every lane
// recomputes its own weight, loads its node's DIM components, and a fixed xor tree over the lane group sums them.
// ub == nullptr: out[k][comp] = (H u)_k; else out[comp][k] = ub[k][comp] - (H u)_k (one contiguous right-hand side per component)
template <int KERN, int DIM>
__global__ void __launch_bounds__(256) ibm_interp_kernel(IbmGrid G, const double* __restrict__ X, const int32_t* __restrict__ base,
                                                         const double* __restrict__ u, const double* __restrict__ ub,
                                                         double* __restrict__ out) {
  constexpr int W = KERN == 0 ? 4 : 3, LANES = DIM == 2 ? 16 : 64;
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
  const int s = threadIdx.x & (LANES - 1);
  const int k = (int)(g < G.n ? g : G.n - 1);      // spare lane groups redo the last marker and write nothing
  int o[3] = {s & 3, (s >> 2) & 3, s >> 4};
  bool act = true;
  double w = 1.0;
  int64_t node = 0, stride = 1;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    if (o[d] >= W) {
      act = false;
      o[d] = 0;
    }
    const int i = base[k * DIM + d] + o[d];
    w *= ibm_w1<KERN>(G, d, i, X[k * DIM + d]);
    node += (int64_t)i * stride;
    stride *= G.N[d];
  }
  double acc[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc[c] = act ? w * u[node * DIM + c] : 0.0;
#pragma unroll
  for (int m = LANES / 2; m > 0; m >>= 1)
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] += __shfl_xor(acc[c], m, LANES);
  if (s == 0 && g < G.n) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      if (ub) out[(int64_t)c * G.n + k] = ub[k * DIM + c] - acc[c];
      else out[k * DIM + c] = acc[c];
    }
  }
}

// u_j += sum_k W_kj c_k q_k over the node's run of sorted pairs, in marker order; q[k * sk + c * sc]
template <int DIM>
__global__ void ibm_spread_kernel(int64_t naff, const int32_t* __restrict__ nodes, const int32_t* __restrict__ segptr,
                                  const int32_t* __restrict__ smk, const double* __restrict__ sw, const double* __restrict__ q,
                                  int64_t sk, int64_t sc, double* __restrict__ u) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= naff) return;
  double acc[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
  for (int p = segptr[i]; p < segptr[i + 1]; ++p) {
    const double w = sw[p];
    const int64_t k = smk[p];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = fma(w, q[k * sk + c * sc], acc[c]);
  }
  const int64_t j = nodes[i];
#pragma unroll
  for (int c = 0; c < DIM; ++c) u[j * DIM + c] += acc[c];
}

IbmGrid grid_of(const IbmState& S) {
  IbmGrid G;
  G.dim = S.dim;
  G.n = (int)S.n;
  for (int d = 0; d < 3; ++d) {
    G.N[d] = S.N[d];
    G.lower[d] = S.lower[d];
    G.h[d] = S.h[d];
  }
  return G;
}

int ibm_alloc(IbmState& S, int64_t n, int dim, int64_t pairs) {
  if (n <= S.cap_n && pairs <= S.cap_pairs) return PYN_OK;
  S.cap_n = S.cap_pairs = 0;   // a failure below leaves no capacity (and no valid set): the next pyn_ibm_set allocates all of them again
  PYN_HIP(S.X.alloc((size_t)n * 3));
  PYN_HIP(S.cw.alloc((size_t)n));
  PYN_HIP(S.base.alloc((size_t)n * 3));
  PYN_HIP(S.A.alloc((size_t)n * n));
  PYN_HIP(S.lu.alloc((size_t)n * n));
  PYN_HIP(S.piv.alloc((size_t)(2 * n + 1)));
  PYN_HIP(S.rq.alloc((size_t)n * 10));
  for (DevBuf<int32_t>* p : {&S.key0, &S.key1, &S.val0, &S.val1, &S.flag, &S.nodes, &S.smk}) PYN_HIP(p->alloc((size_t)pairs));
  PYN_HIP(S.segptr.alloc((size_t)(pairs + 1)));
  PYN_HIP(S.sw.alloc((size_t)pairs));
  S.cap_n = n;
  S.cap_pairs = pairs;
  return PYN_OK;
}

template <int KERN>
int ibm_build(pyn_ctx* c, IbmState& S) {
  hipStream_t s = c->stream;
  const IbmGrid G = grid_of(S);
  const int64_t n = S.n, pairs = n * S.ns;
  const int total = (int)pairs;
  ibm_matrix_kernel<KERN><<<(unsigned)((n * n + 255) / 256), 256, 0, s>>>(G, S.X, S.cw, S.base, S.A);
  ibm_pairs_kernel<<<(unsigned)((pairs + 255) / 256), 256, 0, s>>>(G, S.width, S.ns, S.base, S.key0, S.val0);
  PYN_HIP(hipGetLastError());
  // stable sort by node: markers keep their index order inside a node's run
  size_t tb = 0, tb2 = 0;
  PYN_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, S.key0.get(), S.key1.get(), S.val0.get(), S.val1.get(), total, 0, 32, s));
  hipcub::CountingInputIterator<int32_t> ids(0);
  PYN_HIP(hipcub::DeviceSelect::Flagged(nullptr, tb2, ids, S.flag.get(), S.segptr.get(), S.d_cnt.get(), total, s));
  PYN_HIP(S.tmp.grow(std::max(tb, tb2)));
  PYN_HIP(hipcub::DeviceRadixSort::SortPairs(S.tmp.get(), tb, S.key0.get(), S.key1.get(), S.val0.get(), S.val1.get(), total, 0, 32, s));
  ibm_sorted_kernel<KERN><<<(unsigned)((pairs + 255) / 256), 256, 0, s>>>(G, S.ns, S.X, S.cw, S.base, S.key1, S.val1, S.smk, S.sw, S.flag);
  PYN_HIP(hipGetLastError());
  PYN_HIP(hipcub::DeviceSelect::Flagged(S.tmp.get(), tb2, ids, S.flag.get(), S.segptr.get(), S.d_cnt.get(), total, s));
  int64_t naff = 0;
  PYN_HIP(hipMemcpyAsync(&naff, S.d_cnt, sizeof(naff), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  PYN_CHECK(naff > 0 && naff <= pairs, "pyn_ibm_set: internal error, %lld affected nodes of %lld pairs", (long long)naff, (long long)pairs);
  S.naff = naff;
  ibm_nodes_kernel<<<(unsigned)((naff + 1 + 255) / 256), 256, 0, s>>>(S.key1, S.segptr, naff, total, S.nodes);
  PYN_HIP(hipGetLastError());
  PYN_HIP(hipMemcpyAsync(S.lu, S.A, (size_t)n * n * sizeof(double), hipMemcpyDeviceToDevice, s));
  PYN_TRY(pyn_dense_lu_factor(c, S.lu, S.piv, n));
  return PYN_OK;
}

template <int KERN>
int ibm_interp_launch(pyn_ctx* c, const IbmState& S, const double* u, const double* ub, double* out) {
  const IbmGrid G = grid_of(S);
  if (S.dim == 2)
    ibm_interp_kernel<KERN, 2><<<(unsigned)((S.n * 16 + 255) / 256), 256, 0, c->stream>>>(G, S.X, S.base, u, ub, out);
  else
    ibm_interp_kernel<KERN, 3><<<(unsigned)((S.n * 64 + 255) / 256), 256, 0, c->stream>>>(G, S.X, S.base, u, ub, out);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

int ibm_interp(pyn_ctx* c, const IbmState& S, const double* u, const double* ub, double* out) {
  return S.kernel == 0 ? ibm_interp_launch<0>(c, S, u, ub, out) : ibm_interp_launch<1>(c, S, u, ub, out);
}

int ibm_spread(pyn_ctx* c, const IbmState& S, const double* q, int64_t sk, int64_t sc, double* u) {
  const unsigned grid = (unsigned)((S.naff + 255) / 256);
  if (S.dim == 2) ibm_spread_kernel<2><<<grid, 256, 0, c->stream>>>(S.naff, S.nodes, S.segptr, S.smk, S.sw, q, sk, sc, u);
  else ibm_spread_kernel<3><<<grid, 256, 0, c->stream>>>(S.naff, S.nodes, S.segptr, S.smk, S.sw, q, sk, sc, u);
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

// the marker set and a velocity vector of its block size
int ibm_ready(pyn_ctx* c, const char* what, int u_vec) {
  PYN_CHECK(c, "ctx is NULL");
  PYN_CHECK(c->ibm && c->ibm->valid, "%s: no marker set (pyn_ibm_set first)", what);
  if (u_vec < 0) return PYN_OK;
  PYN_TRY(pyn_check_vec(c, u_vec, what));
  PYN_CHECK(c->vecs[u_vec].bs == c->ibm->dim, "%s: the vector has block size %d, the velocity of this marker set has %d", what,
            c->vecs[u_vec].bs, c->ibm->dim);
  PYN_HIP(hipSetDevice(c->device));
  return PYN_OK;
}

}  // namespace

extern "C" int pyn_ibm_set(pyn_ctx* c, int kernel, int dim, int64_t n, const double* X, const double* dl, const double* lower,
                           const double* h) {
  PYN_CHECK(c && X && dl && lower && h, "NULL argument");
  if (c->ibm) c->ibm->valid = false;      // a refused set leaves no marker set behind
  PYN_CHECK(kernel == 0 || kernel == 1, "pyn_ibm_set: kernel %d is neither 0 (4-point) nor 1 (3-point)", kernel);
  PYN_CHECK(c->n_elem > 0, "pyn_ibm_set: pyn_mesh_set first");
  PYN_CHECK(c->nranks == 1 && c->n_ghost == 0, "pyn_ibm_set: the immersed boundary runs on one rank (no ghost nodes)");
  PYN_CHECK(dim == c->dim, "pyn_ibm_set: dim %d differs from the mesh's %d", dim, c->dim);
  int kind = 0, nx = 0, ny = 0, nz = 0;
  PYN_TRY(pyn_mesh_topology(c, &kind, &nx, &ny, &nz));
  PYN_CHECK(kind >= 1 && kind <= 3, "pyn_ibm_set: needs a structured lattice mesh of ngl 2 or 3 (pyn_mesh_topology kind 1, 2 or 3); this mesh has kind 0");
  const int N[3] = {nx, ny, dim == 3 ? nz : 1};
  PYN_CHECK((int64_t)N[0] * N[1] * N[2] == c->n_node, "pyn_ibm_set: the lattice %d x %d x %d does not hold the mesh's %lld nodes", N[0], N[1],
            N[2], (long long)c->n_node);
  PYN_CHECK(n > 0, "pyn_ibm_set: no markers (n = %lld)", (long long)n);
  PYN_CHECK(n <= pyn_direct_max_rows(), "pyn_ibm_set: %lld markers exceed the dense limit of %d", (long long)n, pyn_direct_max_rows());
  double vol = 1.0;
  for (int d = 0; d < dim; ++d) {
    PYN_CHECK(std::isfinite(lower[d]) && std::isfinite(h[d]) && h[d] > 0.0, "pyn_ibm_set: lower / h of axis %d is not a finite positive spacing", d);
    vol *= h[d];
  }
  const int W = kernel == 0 ? 4 : 3;
  std::vector<int32_t> base((size_t)n * dim);
  std::vector<double> cw((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    PYN_CHECK(std::isfinite(dl[k]), "pyn_ibm_set: dl[%lld] is not finite", (long long)k);
    cw[k] = dl[k] / vol;
    for (int d = 0; d < dim; ++d) {
      const double x = X[k * dim + d];
      PYN_CHECK(std::isfinite(x), "pyn_ibm_set: marker %lld has a non-finite coordinate", (long long)k);
      const double s = (x - lower[d]) / h[d];
      // first line of the support: |r| < 2 (4-point) -> floor(s) - 1 .. + 3; |r| < 3/2 (3-point) -> round(s) - 1 .. + 1
      const double b = std::floor(kernel == 0 ? s : s + 0.5) - 1.0;
      PYN_CHECK(b >= 1.0 && b + W - 1 <= (double)(N[d] - 2),
                "pyn_ibm_set: the support of marker %lld reaches the outermost node layer of axis %d (stencil lines %.0f .. %.0f of 0 .. %d; "
                "they must lie in 1 .. %d)", (long long)k, d, b, b + W - 1, N[d] - 1, N[d] - 2);
      base[k * dim + d] = (int32_t)b;
    }
  }
  PYN_HIP(hipSetDevice(c->device));
  if (!c->ibm) c->ibm.reset(new IbmState());
  IbmState& S = *c->ibm;
  hipStream_t s = c->stream;
  if (!S.d_cnt) PYN_HIP(S.d_cnt.alloc(1));
  bool same = S.lattice_ok && S.dim == dim;
  for (int d = 0; d < dim && same; ++d) same = S.N[d] == N[d] && S.lower[d] == lower[d] && S.h[d] == h[d];
  S.dim = dim;
  for (int d = 0; d < 3; ++d) {
    S.N[d] = N[d];
    S.lower[d] = d < dim ? lower[d] : 0.0;
    S.h[d] = d < dim ? h[d] : 1.0;
  }
  if (!same) {
    S.lattice_ok = false;
    IbmGrid G = grid_of(S);
    int bad = 0;
    int* d_bad = reinterpret_cast<int*>(S.d_cnt.get());
    PYN_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    ibm_lattice_check_kernel<<<(unsigned)((c->n_node + 255) / 256), 256, 0, s>>>(G, c->d_xyz, c->n_node, d_bad);
    PYN_HIP(hipGetLastError());
    PYN_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    PYN_HIP(hipStreamSynchronize(s));
    PYN_CHECK(bad == 0, "pyn_ibm_set: the nodes are not the uniform lattice lower + i h (to 1e-12 of the box extent): jittered, stretched or "
                        "differently sized meshes have no discrete delta here");
    S.lattice_ok = true;
  }
  S.kernel = kernel;
  S.width = W;
  S.ns = dim == 2 ? W * W : W * W * W;
  S.n = n;
  PYN_TRY(ibm_alloc(S, n, dim, n * S.ns));
  PYN_HIP(hipMemcpyAsync(S.X, X, (size_t)n * dim * sizeof(double), hipMemcpyHostToDevice, s));
  PYN_HIP(hipMemcpyAsync(S.cw, cw.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
  PYN_HIP(hipMemcpyAsync(S.base, base.data(), (size_t)n * dim * sizeof(int32_t), hipMemcpyHostToDevice, s));
  PYN_HIP(hipStreamSynchronize(s));      // the host arrays go out of scope
  PYN_TRY(kernel == 0 ? ibm_build<0>(c, S) : ibm_build<1>(c, S));
  S.builds += 1;
  S.valid = true;
  return PYN_OK;
}

extern "C" int pyn_ibm_interp(pyn_ctx* c, int u_vec, double* out) {
  PYN_TRY(ibm_ready(c, "pyn_ibm_interp", u_vec));
  PYN_CHECK(out, "NULL argument");
  const IbmState& S = *c->ibm;
  double* stage = S.rq + (size_t)S.n * 7;
  PYN_TRY(ibm_interp(c, S, c->vecs[u_vec].d, nullptr, stage));
  PYN_HIP(hipMemcpyAsync(out, stage, (size_t)S.n * S.dim * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}

extern "C" int pyn_ibm_spread(pyn_ctx* c, const double* q, int u_vec) {
  PYN_TRY(ibm_ready(c, "pyn_ibm_spread", u_vec));
  PYN_CHECK(q, "NULL argument");
  const IbmState& S = *c->ibm;
  double* stage = S.rq + (size_t)S.n * 7;
  PYN_HIP(hipMemcpyAsync(stage, q, (size_t)S.n * S.dim * sizeof(double), hipMemcpyHostToDevice, c->stream));
  PYN_TRY(ibm_spread(c, S, stage, S.dim, 1, c->vecs[u_vec].d));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}

extern "C" int pyn_ibm_correct(pyn_ctx* c, int u_vec, const double* ub, double* q_out) {
  PYN_TRY(ibm_ready(c, "pyn_ibm_correct", u_vec));
  PYN_CHECK(ub && q_out, "NULL argument");
  const IbmState& S = *c->ibm;
  const int64_t n = S.n;
  double *r = S.rq, *q = S.rq + 3 * n, *z = S.rq + 6 * n, *stage = S.rq + 7 * n;
  double* u = c->vecs[u_vec].d;
  PYN_HIP(hipMemcpyAsync(stage, ub, (size_t)n * S.dim * sizeof(double), hipMemcpyHostToDevice, c->stream));
  PYN_TRY(ibm_interp(c, S, u, stage, r));                                     // r = U_B - H u, [component][marker]
  for (int d = 0; d < S.dim; ++d) PYN_TRY(pyn_dense_lu_solve(c, S.lu, S.piv, n, r + d * n, q + d * n, z));
  PYN_TRY(ibm_spread(c, S, q, 1, n, u));                                      // u += S q
  std::vector<double> hq((size_t)n * S.dim);
  PYN_HIP(hipMemcpyAsync(hq.data(), q, hq.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  for (int64_t k = 0; k < n; ++k)
    for (int d = 0; d < S.dim; ++d) q_out[k * S.dim + d] = hq[(size_t)d * n + k];
  return PYN_OK;
}

extern "C" int pyn_ibm_matrix_get(pyn_ctx* c, double* A) {
  PYN_TRY(ibm_ready(c, "pyn_ibm_matrix_get", -1));
  PYN_CHECK(A, "NULL argument");
  PYN_HIP(hipSetDevice(c->device));
  const IbmState& S = *c->ibm;
  PYN_HIP(hipMemcpyAsync(A, S.A, (size_t)S.n * S.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}

extern "C" int pyn_ibm_info(pyn_ctx* c, int64_t* info) {
  PYN_TRY(ibm_ready(c, "pyn_ibm_info", -1));
  PYN_CHECK(info, "NULL argument");
  const IbmState& S = *c->ibm;
  info[0] = S.n;
  info[1] = S.width;
  info[2] = S.naff;
  info[3] = S.builds;
  return PYN_OK;
}

extern "C" int pyn_ibm_clear(pyn_ctx* c) {
  PYN_TRY(ibm_ready(c, "pyn_ibm_clear", -1));
  PYN_HIP(hipSetDevice(c->device));
  PYN_HIP(hipStreamSynchronize(c->stream));
  c->ibm.reset();
  return PYN_OK;
}
