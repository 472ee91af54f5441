// Analytic fields and constant values on node sets: what DMPlexDom.applyFunctionVecToVec / applyValuesToVec (the reference's
// src/domain/dmplex.py:262-296) do per node on the host with the closed-form fields of src/cases/custom_func.py, as one launch.
//
//  * node sets: sorted owned local node ids kept on the device, range-checked once when they are created
//  * field_kernel<F>:     vec[node*bs + k] = field_k(xyz[node]) over a set (or over every owned node); one lane per node, grid-stride,
//                         a gather of dim coordinates and a scatter of bs values, no LDS, no atomics
//  * set_nodes_kernel<B>: vec[node*B + k] = values[k] for the components of a mask
// Both are stream-ordered and copy nothing: parameters and values travel by value in the kernel arguments.
//
// Rounding contract of the fields: every coordinate-independent factor -- the decay exp(...), 2 pi e, 6 (2 pi e)^2,
// 9 nu e (2 pi)^3, -2 pi (1/Lx + 1/Ly) ... -- is computed by the caller with the reference's own Python expression; the kernel
// rounds each phase k x_d once, takes one sincos per axis it needs, and multiplies the factors one rounding at a time in the
// left-to-right order of the Python expression.  Contraction is switched off for this whole file (the pragma below; hipcc's default
// would fuse the two-term fields' a c1 - b c2 into a multiply and a fused multiply-add, and __dmul_rn / __dsub_rn are plain * and -
// in this toolchain, so they do not prevent it).  The result differs from the host function only by the last bits of sin and cos.
#include <cstdint>

#include "pyn_internal.h"

#pragma clang fp contract(off)

namespace {

struct FieldInfo {
  int dim, bs, nparams;
};
// row = PYN_FIELD_*
constexpr FieldInfo FIELD_INFO[PYN_FIELD_COUNT] = {{2, 2, 2}, {2, 1, 3}, {3, 3, 2}, {3, 3, 2}, {3, 3, 2},
                                                   {3, 3, 2}, {2, 2, 1}, {2, 1, 1}, {2, 1, 2}, {2, 1, 4}};

struct FieldParams {
  double p[PYN_FIELD_MAX_PARAMS];
};

// one rounding per product (contraction is off in this file)
__device__ __forceinline__ double mul(double a, double b) { return a * b; }

// out[0 .. bs) at the point X; P.p[] as the table of include/pynama_hip.h lists them
template <int F>
__device__ __forceinline__ void field_at(const FieldParams& P, const double* X, double* out) {
  const double k = P.p[0];
  if (F == PYN_FIELD_TG2D_VEL || F == PYN_FIELD_TG2D_VORT) {
    double sx, cx, sy, cy;
    sincos(mul(k, X[0]), &sx, &cx);
    sincos(mul(k, X[1]), &sy, &cy);
    if (F == PYN_FIELD_TG2D_VEL) {
      const double e = P.p[1];
      out[0] = mul(mul(cx, sy), e);
      out[1] = mul(mul(-sx, cy), e);
    } else {
      out[0] = mul(mul(mul(P.p[1], cx), cy), P.p[2]);
    }
  } else if (F >= PYN_FIELD_TG3D_VEL && F <= PYN_FIELD_TG3D_DIFF) {
    double sx, cx, sy, cy, sz, cz;
    sincos(mul(k, X[0]), &sx, &cx);
    sincos(mul(k, X[1]), &sy, &cy);
    sincos(mul(k, X[2]), &sz, &cz);
    const double a = P.p[1];
    if (F == PYN_FIELD_TG3D_VEL) {
      out[0] = mul(mul(mul(cx, sy), sz), a);
      out[1] = mul(mul(mul(sx, cy), sz), a);
      out[2] = mul(mul(mul(mul(-2.0, sx), sy), cz), a);
    } else if (F == PYN_FIELD_TG3D_VORT) {
      out[0] = mul(mul(mul(mul(-3.0, a), sx), cy), cz);
      out[1] = mul(mul(mul(mul(3.0, a), cx), sy), cz);
      out[2] = 0.0;
    } else if (F == PYN_FIELD_TG3D_CONV) {
      out[0] = mul(mul(mul(mul(-a, sy), cy), sz), cz);
      out[1] = mul(mul(mul(mul(a, sx), cx), sz), cz);
      out[2] = 0.0;
    } else {
      out[0] = mul(mul(mul(a, sx), cy), cz);
      out[1] = mul(mul(mul(-a, cx), sy), cz);
      out[2] = 0.0;
    }
  } else {
    const double k2 = mul(2.0, k);   // 4 pi = 2 (2 pi), exact
    double s1, c1, s2, c2;
    sincos(mul(k, X[1]), &s1, &c1);    // 2 pi y
    sincos(mul(k2, X[0]), &s2, &c2);   // 4 pi x
    if (F == PYN_FIELD_SEN2D_VEL) {
      out[0] = s1;
      out[1] = s2;
    } else if (F == PYN_FIELD_SEN2D_VORT) {
      out[0] = mul(k2, c2) - mul(k, c1);
    } else if (F == PYN_FIELD_SEN2D_CONV) {
      out[0] = mul(mul(P.p[1], s1), s2);
    } else {
      out[0] = mul(P.p[1], mul(P.p[2], c1) - mul(P.p[3], c2));
    }
  }
}

// set == nullptr: the nodes 0 .. n-1
template <int F>
__global__ void __launch_bounds__(256) field_kernel(FieldParams P, const int32_t* __restrict__ set, int64_t n,
                                                    const double* __restrict__ xyz, double* __restrict__ vec) {
  constexpr int DIM = FIELD_INFO[F].dim, BS = FIELD_INFO[F].bs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t node = set ? (int64_t)set[i] : i;
    double X[DIM], out[BS];
#pragma unroll
    for (int d = 0; d < DIM; ++d) X[d] = xyz[node * DIM + d];
    field_at<F>(P, X, out);
#pragma unroll
    for (int q = 0; q < BS; ++q) vec[node * BS + q] = out[q];
  }
}

struct NodeValues {
  double v[6];
};

template <int BS>
__global__ void __launch_bounds__(256) set_nodes_kernel(NodeValues V, unsigned mask, const int32_t* __restrict__ set, int64_t n,
                                                        double* __restrict__ vec) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t node = set ? (int64_t)set[i] : i;
#pragma unroll
    for (int q = 0; q < BS; ++q)
      if (mask & (1u << q)) vec[node * BS + q] = V.v[q];
  }
}

inline int nodes_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, PYN_MAX_PARTIALS)); }

// the nodes a call addresses: the set's, or every owned node (set_id -1)
int resolve_set(pyn_ctx* c, int set_id, const char* what, const int32_t** set, int64_t* n) {
  if (set_id == -1) {
    *set = nullptr;
    *n = c->n_owned;
    return PYN_OK;
  }
  PYN_CHECK(set_id >= 0 && set_id < (int)c->nodesets.size() && c->nodesets[set_id].live, "%s: invalid node set handle %d", what, set_id);
  *set = c->nodesets[set_id].d;
  *n = c->nodesets[set_id].n;
  return PYN_OK;
}

}  // namespace

extern "C" int pyn_nodeset_create(pyn_ctx* c, int64_t n, const int32_t* nodes, int* set_id) {
  PYN_CHECK(c && set_id, "NULL argument");
  PYN_CHECK(c->n_node > 0, "pyn_nodeset_create: pyn_mesh_set first");
  PYN_CHECK(n >= 0 && n <= c->n_owned, "pyn_nodeset_create: %lld nodes, the rank owns %lld", (long long)n, (long long)c->n_owned);
  PYN_CHECK(n == 0 || nodes, "pyn_nodeset_create: nodes is NULL");
  for (int64_t i = 0; i < n; ++i) {
    PYN_CHECK(nodes[i] >= 0 && nodes[i] < c->n_owned, "pyn_nodeset_create: nodes[%lld] = %d outside the owned nodes [0, %lld)",
              (long long)i, nodes[i], (long long)c->n_owned);
    PYN_CHECK(i == 0 || nodes[i] > nodes[i - 1], "pyn_nodeset_create: nodes[%lld] = %d after %d: not strictly increasing", (long long)i,
              nodes[i], nodes[i - 1]);
  }
  PYN_HIP(hipSetDevice(c->device));
  DNodeSet s;
  s.n = n;
  PYN_TRY(dev_upload(s.d, nodes, (size_t)n, c->stream));
  if (n) PYN_HIP(hipStreamSynchronize(c->stream));   // nodes is borrowed for the call only
  s.live = true;
  c->nodesets.push_back(std::move(s));
  *set_id = (int)c->nodesets.size() - 1;
  return PYN_OK;
}

extern "C" int pyn_nodeset_destroy(pyn_ctx* c, int set_id) {
  PYN_CHECK(c, "ctx is NULL");
  PYN_CHECK(set_id >= 0 && set_id < (int)c->nodesets.size() && c->nodesets[set_id].live, "pyn_nodeset_destroy: invalid node set handle %d",
            set_id);
  PYN_HIP(hipStreamSynchronize(c->stream));   // a queued launch may still read it
  c->nodesets[set_id] = DNodeSet();
  return PYN_OK;
}

extern "C" int pyn_field_info(int field, int* dim, int* bs, int* nparams) {
  PYN_CHECK(field >= 0 && field < PYN_FIELD_COUNT, "pyn_field_info: unknown field %d", field);
  if (dim) *dim = FIELD_INFO[field].dim;
  if (bs) *bs = FIELD_INFO[field].bs;
  if (nparams) *nparams = FIELD_INFO[field].nparams;
  return PYN_OK;
}

extern "C" int pyn_field_eval(pyn_ctx* c, int field, const double* params, int nparams, int set_id, int vec_id) {
  PYN_CHECK(c, "ctx is NULL");
  PYN_CHECK(field >= 0 && field < PYN_FIELD_COUNT, "pyn_field_eval: unknown field %d", field);
  const FieldInfo& I = FIELD_INFO[field];
  PYN_CHECK(c->n_node > 0 && c->d_xyz, "pyn_field_eval: pyn_mesh_set first");
  PYN_CHECK(I.dim == c->dim, "pyn_field_eval: field %d is %d-D, the mesh is %d-D", field, I.dim, c->dim);
  PYN_TRY(pyn_check_vec(c, vec_id, "pyn_field_eval"));
  DVec& v = c->vecs[vec_id];
  PYN_CHECK(v.bs == I.bs, "pyn_field_eval: field %d has %d components, the vector has block size %d", field, I.bs, v.bs);
  PYN_CHECK(nparams == I.nparams && params, "pyn_field_eval: field %d takes %d parameters, got %d", field, I.nparams, params ? nparams : 0);
  const int32_t* set = nullptr;
  int64_t n = 0;
  PYN_TRY(resolve_set(c, set_id, "pyn_field_eval", &set, &n));
  if (n == 0) return PYN_OK;
  FieldParams P;
  for (int j = 0; j < PYN_FIELD_MAX_PARAMS; ++j) P.p[j] = j < nparams ? params[j] : 0.0;
  const int g = nodes_grid(n);
  hipStream_t s = c->stream;
  switch (field) {
#define PYN_FIELD(F) \
  case F: field_kernel<F><<<g, 256, 0, s>>>(P, set, n, c->d_xyz, v.d); break
    PYN_FIELD(PYN_FIELD_TG2D_VEL); PYN_FIELD(PYN_FIELD_TG2D_VORT); PYN_FIELD(PYN_FIELD_TG3D_VEL); PYN_FIELD(PYN_FIELD_TG3D_VORT);
    PYN_FIELD(PYN_FIELD_TG3D_CONV); PYN_FIELD(PYN_FIELD_TG3D_DIFF); PYN_FIELD(PYN_FIELD_SEN2D_VEL); PYN_FIELD(PYN_FIELD_SEN2D_VORT);
    PYN_FIELD(PYN_FIELD_SEN2D_CONV); PYN_FIELD(PYN_FIELD_SEN2D_DIFF);
#undef PYN_FIELD
  }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

extern "C" int pyn_vec_set_nodes(pyn_ctx* c, int vec_id, int set_id, const double* values, int nvalues, const uint8_t* dofs) {
  PYN_TRY(pyn_check_vec(c, vec_id, "pyn_vec_set_nodes"));
  DVec& v = c->vecs[vec_id];
  PYN_CHECK(values && nvalues == v.bs, "pyn_vec_set_nodes: %d values for a vector of block size %d", values ? nvalues : 0, v.bs);
  const int32_t* set = nullptr;
  int64_t n = 0;
  PYN_TRY(resolve_set(c, set_id, "pyn_vec_set_nodes", &set, &n));
  NodeValues V;
  unsigned mask = 0;
  for (int q = 0; q < 6; ++q) V.v[q] = q < v.bs ? values[q] : 0.0;
  for (int q = 0; q < v.bs; ++q)
    if (!dofs || dofs[q]) mask |= 1u << q;
  if (n == 0 || mask == 0) return PYN_OK;
  const int g = nodes_grid(n);
  hipStream_t s = c->stream;
  switch (v.bs) {
#define PYN_SETN(B) \
  case B: set_nodes_kernel<B><<<g, 256, 0, s>>>(V, mask, set, n, v.d); break
    PYN_SETN(1); PYN_SETN(2); PYN_SETN(3); PYN_SETN(4); PYN_SETN(5); PYN_SETN(6);
#undef PYN_SETN
  }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}
