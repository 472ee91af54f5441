// The one detector of structured topology: is the connectivity that of the reference's box mesh of order ngl >= 2
// (src/domain/dmplex.py:8-21, 42-61: (ngl - 1) nelem + 1 nodes per axis, numbered lexicographically, cells in the reference's local
// node order), or a rank's slab of one?  Fills pyn_ctx::box (BoxLattice, pyn_internal.h); the kernel families then admit the mesh
// through their views (pyn_lattice_view, pyn_ho3_view, pyn_ho_view).
#include <algorithm>

#include "pyn_internal.h"

// Reference position (i, j[, k]) of every local point of an n^dim tensor set in the reference's vertex / edge / face / interior order
// (src/elements/spectral.py:220-271 in 2-D, :346-431 in 3-D)
void ref_local_lattice(int n, int dim, std::vector<int>& out) {
  out.clear();
  auto push = [&](int i, int j, int k) {
    out.push_back(i);
    out.push_back(j);
    if (dim == 3) out.push_back(k);
  };
  if (n == 1) {
    push(0, 0, 0);
    return;
  }
  const int m = n - 1;
  if (dim == 2) {
    const int v[4][2] = {{m, m}, {0, m}, {0, 0}, {m, 0}};
    for (auto& p : v) push(p[0], p[1], 0);
    for (int a = 0; a < 4; ++a) {
      const int* p0 = v[a];
      const int* p1 = v[(a + 1) % 4];
      for (int s = 1; s < m; ++s) push(p0[0] + s * (p1[0] - p0[0]) / m, p0[1] + s * (p1[1] - p0[1]) / m, 0);
    }
    for (int i = 1; i < m; ++i)
      for (int j = m - 1; j >= 1; --j) push(i, j, 0);
    return;
  }
  const int v[8][3] = {{0, 0, 0}, {0, m, 0}, {m, m, 0}, {m, 0, 0}, {0, 0, m}, {m, 0, m}, {m, m, m}, {0, m, m}};
  const int edges[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {3, 5}, {4, 0}, {1, 7}, {6, 2}};
  for (auto& p : v) push(p[0], p[1], p[2]);
  for (auto& e : edges) {
    const int* p0 = v[e[0]];
    const int* p1 = v[e[1]];
    for (int s = 1; s < m; ++s)
      push(p0[0] + s * (p1[0] - p0[0]) / m, p0[1] + s * (p1[1] - p0[1]) / m, p0[2] + s * (p1[2] - p0[2]) / m);
  }
  for (int j = m - 1; j >= 1; --j)
    for (int i = 1; i < m; ++i) push(i, j, 0);   // face t = -1
  for (int j = 1; j < m; ++j)
    for (int i = m - 1; i >= 1; --i) push(i, j, m);   // face t = +1
  for (int i = m - 1; i >= 1; --i)
    for (int k = 1; k < m; ++k) push(i, 0, k);   // face s = -1
  for (int i = 1; i < m; ++i)
    for (int k = m - 1; k >= 1; --k) push(i, m, k);   // face s = +1
  for (int k = m - 1; k >= 1; --k)
    for (int j = m - 1; j >= 1; --j) push(m, j, k);   // face r = +1
  for (int k = 1; k < m; ++k)
    for (int j = 1; j < m; ++j) push(0, j, k);   // face r = -1
  for (int k = m - 1; k >= 1; --k)
    for (int j = m - 1; j >= 1; --j)
      for (int i = 1; i < m; ++i) push(i, j, k);
}

// lattice offset of every local node of the box mesh: the reference position, flipped on both axes in 2-D (dmplex.py: x ~ -r, y ~ -s)
void mesh_local_lattice(int ngl, int dim, std::vector<int>& loc) {
  ref_local_lattice(ngl, dim, loc);
  if (dim == 2)
    for (int& v : loc) v = ngl - 1 - v;
}

// every entry of the connectivity against the closed form of the lattice (one thread per entry; `bad` counts the mismatches)
__global__ void box_conn_verify_kernel(const int32_t* __restrict__ conn, const int32_t* __restrict__ P, const int32_t* __restrict__ loc, int dim,
                                       int nn, int m, int64_t ne, int EX, int EY, int NX, int64_t per_layer, int* __restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ne * nn) return;
  const int64_t e = t / nn;
  const int a = (int)(t - e * nn);
  const int ex = (int)(e % EX), ey = (int)((e / EX) % EY);
  const int64_t el = e / per_layer;
  const int32_t* l = loc + a * dim;
  const int64_t id = (int64_t)P[m * el + l[dim - 1]] + (int64_t)(m * ey + (dim == 3 ? l[1] : 0)) * NX + m * ex + l[0];
  if (conn[t] != id) atomicAdd(bad, 1);
}

// `at(i)`: entry i of the local connectivity as the host sees it (the uploaded array, or the closed form of pyn_mesh_box); the shape
// guessed from O(element rows + layers) entries is checked against ALL of c->d_conn on the device.  Applies what every view asks for;
// the views add their own limits.
int pyn_box_detect(pyn_ctx* c, const ConnAt& at) {
  const int dim = c->dim, nn = c->nn, ngl = c->ngl;
  if (ngl < 2 || c->n_elem < 1) return PYN_OK;
  const int m = ngl - 1;
  std::vector<int> loc;
  mesh_local_lattice(ngl, dim, loc);
  std::vector<int> a_of((size_t)nn, -1);   // local node at tensor position i + ngl (j + ngl k)
  for (int a = 0; a < nn; ++a) {
    int t = 0;
    for (int d = dim - 1; d >= 0; --d) t = t * ngl + loc[a * dim + d];
    a_of[t] = a;
  }
  const int a0 = a_of[0];
  const int64_t ne = c->n_elem;
  const int32_t c0 = at(a0);
  int64_t EX = 1;
  while (EX < ne && at(EX * nn + a0) == c0 + m * EX) ++EX;
  if (ne % EX) return PYN_OK;
  const int64_t NX = m * EX + 1;
  int64_t EY = 1;
  if (dim == 3) {
    while (EY * EX < ne && at(EY * EX * nn + a0) == c0 + m * EY * NX) ++EY;
    if ((ne / EX) % EY) return PYN_OK;
  }
  const int64_t per_layer = EX * EY, EL = ne / per_layer;   // EL: cell layers along the slow axis
  const int64_t NY = dim == 3 ? m * EY + 1 : 1, PS = NX * NY, npl = m * EL + 1;
  if (PS * npl != c->n_node || PS > INT32_MAX / 2) return PYN_OK;
  std::vector<int32_t> P((size_t)npl, -1);
  const int stride_s = dim == 3 ? ngl * ngl : ngl;     // tensor stride of the slow axis
  for (int64_t l = 0; l < EL; ++l)
    for (int j = 0; j < ngl; ++j) {
      const int32_t base = at(l * per_layer * nn + a_of[j * stride_s]);
      if (P[m * l + j] >= 0 && P[m * l + j] != base) return PYN_OK;
      P[m * l + j] = base;
    }
  // planes are disjoint blocks of PS ids; the owned ones are consecutive along the slow axis and carry ids 0 .. n_owned-1
  std::vector<int32_t> sorted(P);
  std::sort(sorted.begin(), sorted.end());
  for (int64_t j = 0; j < npl; ++j)
    if (sorted[j] != j * PS) return PYN_OK;
  if (c->n_owned % PS) return PYN_OK;
  const int n_own = (int)(c->n_owned / PS);
  int p0 = -1;
  for (int64_t j = 0; j < npl; ++j)
    if (P[j] == 0) p0 = (int)j;
  if (p0 < 0 || p0 + n_own > npl) return PYN_OK;
  for (int j = 0; j < n_own; ++j)
    if (P[p0 + j] != (int64_t)j * PS) return PYN_OK;
  DevBuf<int32_t> d_P, d_loc;
  DevBuf<int> d_bad;
  int bad = 0;
  const std::vector<int32_t> loc32(loc.begin(), loc.end());
  PYN_TRY(dev_upload(d_P, (const int32_t*)P.data(), (size_t)npl, c->stream));
  PYN_TRY(dev_upload(d_loc, loc32.data(), loc32.size(), c->stream));
  PYN_HIP(d_bad.alloc(1));
  PYN_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), c->stream));
  box_conn_verify_kernel<<<(unsigned)((ne * nn + 255) / 256), 256, 0, c->stream>>>(c->d_conn, d_P, d_loc, dim, nn, m, ne, (int)EX, (int)EY, (int)NX,
                                                                                 per_layer, d_bad);
  PYN_HIP(hipGetLastError());
  PYN_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  if (bad) return PYN_OK;
  BoxLattice& B = c->box;
  B.d_P = std::move(d_P);
  B.P = P;
  B.dim = dim;
  B.ngl = ngl;
  B.EX = (int)EX;
  B.EY = (int)EY;
  B.EL = (int)EL;
  B.NX = (int)NX;
  B.NY = (int)NY;
  B.npl = (int)npl;
  B.p_own0 = p0;
  B.n_own = n_own;
  B.valid = true;
  return PYN_OK;
}
