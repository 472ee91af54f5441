// Geometric multigrid preconditioner for CG on structured lattice meshes (PETSc's -pc_type mg, PCMG).
//
// Jacobi-PCG needs a number of iterations that grows with 1/h (15,740 at 2-D 1024^2 ngl 3); a V-cycle whose cost is a few fine
// products makes the count independent of the mesh.  Every mesh that reaches the fast paths is a structured lattice, so the
// hierarchy is geometric:
//   levels   level 0 is the matrix itself; a lattice of 2M cells per axis coarsens to M cells (coarse node I = fine node 2I).  An
//            ngl 3 lattice of E cells has the node lattice of a Q1 lattice of 2E cells, so p-coarsening to Q1 and h-coarsening are
//            the same step.  Coarsening stops when an axis has an odd cell count, at max_levels, or at <= coarse_max_rows rows.
//   P        tensor-product linear interpolation per component: coincident nodes copy, edge midpoints take 1/2 of each end, face
//            centres 1/4, cell centres 1/8.  P is zero in decoupled fine rows and in decoupled coarse columns.
//   decoupled DOFs: rows whose only non-zero is the diagonal (the Dirichlet rows the assemblies leave), detected from the values
//            at level 0; a coarse DOF is decoupled when its coincident fine DOF is, and its row is that fine diagonal.
//   A_c      = P^T A P on the device, stored as a dense Q1 stencil [node][3^d][b][b] (offsets x fastest, k = sum (o_a + 1) 3^a):
//            an ngl 3 fine row reaches +-2 fine nodes, i.e. +-1 coarse node, so every coarse level is a 3^d stencil.
//   smoother Chebyshev of degree k with Jacobi scaling on [emin, emax] * lambda, lambda estimating lambda_max(D^-1 A) from a few
//            seeded CG (Lanczos) steps per level; the same polynomial before and after the coarse correction, zero start, so that the
//            V-cycle is symmetric; decoupled rows take z = r / a_ii exactly.
//   coarsest the dense LU of pyn_direct.hip on a dense image of the coarsest stencil.
//   ngl >= 4 box lattices (pyn_ctx::ho_valid; pyn_mesh_topology kind 0) take one other first step: level 1 is the Q1 lattice of the same
//            cells (coarse node I = fine node (ngl - 1) I, any cell count), P0 interpolates linearly at the GLL nodes, and
//            S1 = P0^T A P0 is probed through 3^d b assembled products (mg_ho_probe); the mg_ho kernels are the 0 <-> 1 transfers.
// Level 0 is multiplied by whatever the caller supplies (the assembled product or the matrix-free shell); levels >= 1 by the
// stencil kernels below, with the Chebyshev step fused into the product, the residual into the restriction and the prolongation
// into the add.  Everything is FP64.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "pyn_internal.h"

namespace {

// node lattice of one level: id = P[z] + y nx + x (3-D), P[y] + x (2-D); level 0 keeps the mesh's plane order, coarse levels are
// lexicographic.  nz = 1 in 2-D.
struct Grid {
  int dim, nx, ny, nz;
  const int32_t* P;      // [slow-axis planes]: first id of the plane
  const int32_t* invP;   // [planes]: plane slot (id / plane size) -> slow-axis index
  __device__ __forceinline__ int plane() const { return dim == 3 ? nx * ny : nx; }
  __device__ __forceinline__ int64_t id(int x, int y, int z) const {
    return dim == 3 ? (int64_t)P[z] + (int64_t)y * nx + x : (int64_t)P[y] + x;
  }
  __device__ __forceinline__ void coords(int64_t i, int& x, int& y, int& z) const {
    const int pl = plane();
    const int64_t slot = i / pl;
    const int rem = (int)(i - slot * pl);
    const int s = invP[slot];
    if (dim == 3) {
      x = rem % nx;
      y = rem / nx;
      z = s;
    } else {
      x = rem;
      y = s;
      z = 0;
    }
  }
  __device__ __forceinline__ bool in(int x, int y, int z) const { return x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz; }
  __device__ __forceinline__ int64_t nodes() const { return (int64_t)nx * ny * nz; }
  // lexicographic index t -> coordinates (kernels that walk every node of a level)
  __device__ __forceinline__ void lex(int64_t t, int& x, int& y, int& z) const {
    x = (int)(t % nx);
    const int64_t r = t / nx;
    y = (int)(r % ny);
    z = (int)(r / ny);
  }
};

template <int D>
__device__ __forceinline__ void st_off(int k, int& ox, int& oy, int& oz) {
  ox = k % 3 - 1;
  oy = (k / 3) % 3 - 1;
  oz = D == 3 ? k / 9 - 1 : 0;
}
__device__ __forceinline__ double pw(int a) { return a == 0 ? 1.0 : 0.5; }   // 1-D interpolation weight of offset a in {-1, 0, 1}

inline int grid_for(int64_t n, int block = 256) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + block - 1) / block, 1 << 20)); }

// ---- set-up kernels ----------------------------------------------------------------------------------------------------------

// level 0: a_ii and "decoupled" (every other stored entry of the scalar row is zero) per scalar row
__global__ void mg_decouple0_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const double* __restrict__ val,
                                    int64_t n_nodes, int b, uint8_t* __restrict__ dec, double* __restrict__ diag) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_nodes * b; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = r / b;
    const int p = (int)(r - i * b);
    const int lo = rowptr[i], len = rowptr[i + 1] - lo;
    const double* v = val + ((int64_t)lo * b + (int64_t)p * len) * b;
    double a = 0.0;
    bool off = false;
    for (int e = 0; e < len * b; ++e) {
      const bool d = colidx[lo + e / b] == (int)i && e % b == p;
      if (d) a = v[e];
      else off |= v[e] != 0.0;
    }
    diag[r] = a;
    dec[r] = off ? 0 : 1;
  }
}

// coarse DOF decoupled <=> its coincident fine DOF is; its diagonal is that fine diagonal
// (coarse node I = fine node m I: m = 2 between h-levels, ngl - 1 below a high-order level 0)
__global__ void mg_coarse_dec_kernel(Grid f, Grid cg, int b, int m, const uint8_t* __restrict__ dec_f, const double* __restrict__ diag_f,
                                     uint8_t* __restrict__ dec_c, double* __restrict__ diag_c) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cg.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int x, y, z;
    cg.lex(t, x, y, z);
    const int64_t I = cg.id(x, y, z), i = f.id(m * x, m * y, m * z);
    for (int p = 0; p < b; ++p) {
      dec_c[I * b + p] = dec_f[i * b + p];
      diag_c[I * b + p] = diag_f[i * b + p];
    }
  }
}

// A_c = P^T A P from the block-CSR values of level 0: one wave per coarse node I.  For each of the 3^d fine nodes i around 2I, the
// row's columns are located by their lattice offset from i (an LDS table over +-2 per axis), then every lane accumulates its
// outputs (k, p, q) over the fine children j of J = I + o_k present in the row.  Deterministic: no atomics.
template <int B, int D>
__global__ void __launch_bounds__(64) mg_galerkin0_kernel(Grid f, Grid cg, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                          const double* __restrict__ val, const uint8_t* __restrict__ dec_f,
                                                          const uint8_t* __restrict__ dec_c, const double* __restrict__ diag_c,
                                                          double* __restrict__ Sc, int* __restrict__ bad) {
  constexpr int NST = D == 3 ? 27 : 9, NOUT = NST * B * B, NP = D == 3 ? 125 : 25, NR = (NOUT + 63) / 64;
  __shared__ int pos[NP];
  const int lane = threadIdx.x;
  for (int64_t t = blockIdx.x; t < cg.nodes(); t += gridDim.x) {
    int X, Y, Z;
    cg.lex(t, X, Y, Z);
    const int64_t I = cg.id(X, Y, Z);
    double acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
    for (int a = 0; a < NST; ++a) {
      int ax, ay, az;
      st_off<D>(a, ax, ay, az);
      const int fx = 2 * X + ax, fy = 2 * Y + ay, fz = 2 * Z + az;
      if (!f.in(fx, fy, fz)) continue;   // uniform over the wave
      const int64_t i = f.id(fx, fy, fz);
      const int lo = rowptr[i], len = rowptr[i + 1] - lo;
      for (int e = lane; e < NP; e += 64) pos[e] = -1;
      __syncthreads();
      for (int e = lane; e < len; e += 64) {
        int jx, jy, jz;
        f.coords(colidx[lo + e], jx, jy, jz);
        const int dx = jx - fx, dy = jy - fy, dz = jz - fz;
        if (abs(dx) > 2 || abs(dy) > 2 || abs(dz) > 2) atomicExch(bad, 1);
        else pos[(dx + 2) + 5 * (dy + 2) + (D == 3 ? 25 * (dz + 2) : 0)] = e;
      }
      __syncthreads();
      const double wa = pw(ax) * pw(ay) * pw(az);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int o = lane + 64 * r;
        if (o >= NOUT) break;
        const int k = o / (B * B), p = (o / B) % B, q = o % B;
        if (dec_f[i * B + p] || dec_c[I * B + p]) continue;
        int ox, oy, oz;
        st_off<D>(k, ox, oy, oz);
        const int JX = X + ox, JY = Y + oy, JZ = Z + oz;
        if (!cg.in(JX, JY, JZ) || dec_c[cg.id(JX, JY, JZ) * B + q]) continue;
        double s = 0.0;
        for (int cc = 0; cc < NST; ++cc) {
          int cx, cy, cz;
          st_off<D>(cc, cx, cy, cz);
          const int dx = 2 * ox + cx - ax, dy = 2 * oy + cy - ay, dz = 2 * oz + cz - az;
          if (abs(dx) > 2 || abs(dy) > 2 || abs(dz) > 2) continue;
          const int e = pos[(dx + 2) + 5 * (dy + 2) + (D == 3 ? 25 * (dz + 2) : 0)];
          if (e < 0 || dec_f[(int64_t)colidx[lo + e] * B + q]) continue;
          s = fma(pw(cx) * pw(cy) * pw(cz), val[((int64_t)lo * B + (int64_t)p * len + e) * B + q], s);
        }
        acc[r] = fma(wa, s, acc[r]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int o = lane + 64 * r;
      if (o >= NOUT) break;
      const int k = o / (B * B), p = (o / B) % B, q = o % B;
      double v = acc[r];
      if (dec_c[I * B + p]) v = (k == NST / 2 && p == q) ? diag_c[I * B + p] : 0.0;
      Sc[I * NOUT + o] = v;
    }
  }
}

// A_c = P^T A_f P between two stencil levels: one thread per (coarse node, stencil entry), its b x b block
template <int B, int D>
__global__ void __launch_bounds__(256) mg_galerkin_kernel(Grid f, Grid cg, const double* __restrict__ Sf, const uint8_t* __restrict__ dec_f,
                                                          const uint8_t* __restrict__ dec_c, const double* __restrict__ diag_c,
                                                          double* __restrict__ Sc) {
  constexpr int NST = D == 3 ? 27 : 9;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cg.nodes() * NST; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tn = t / NST;
    const int k = (int)(t - tn * NST);
    int X, Y, Z, ox, oy, oz;
    cg.lex(tn, X, Y, Z);
    st_off<D>(k, ox, oy, oz);
    const int64_t I = cg.id(X, Y, Z);
    const int JX = X + ox, JY = Y + oy, JZ = Z + oz;
    double acc[B][B] = {};
    if (cg.in(JX, JY, JZ)) {
      const int64_t J = cg.id(JX, JY, JZ);
      for (int a = 0; a < NST; ++a) {
        int ax, ay, az;
        st_off<D>(a, ax, ay, az);
        const int fx = 2 * X + ax, fy = 2 * Y + ay, fz = 2 * Z + az;
        if (!f.in(fx, fy, fz)) continue;
        const int64_t i = f.id(fx, fy, fz);
        const double wa = pw(ax) * pw(ay) * pw(az);
        for (int cc = 0; cc < NST; ++cc) {
          int cx, cy, cz;
          st_off<D>(cc, cx, cy, cz);
          const int dx = 2 * ox + cx - ax, dy = 2 * oy + cy - ay, dz = 2 * oz + cz - az;
          if (abs(dx) > 1 || abs(dy) > 1 || abs(dz) > 1) continue;
          const int gx = 2 * JX + cx, gy = 2 * JY + cy, gz = 2 * JZ + cz;
          if (!f.in(gx, gy, gz)) continue;
          const int64_t j = f.id(gx, gy, gz);
          const int kk = (dx + 1) + 3 * (dy + 1) + (D == 3 ? 9 * (dz + 1) : 0);
          const double w = wa * pw(cx) * pw(cy) * pw(cz);
          const double* s = Sf + (i * NST + kk) * B * B;
#pragma unroll
          for (int p = 0; p < B; ++p)
#pragma unroll
            for (int q = 0; q < B; ++q)
              if (!dec_f[i * B + p] && !dec_f[j * B + q]) acc[p][q] = fma(w, s[p * B + q], acc[p][q]);
        }
      }
#pragma unroll
      for (int q = 0; q < B; ++q)
        if (dec_c[J * B + q])
#pragma unroll
          for (int p = 0; p < B; ++p) acc[p][q] = 0.0;
    }
#pragma unroll
    for (int p = 0; p < B; ++p) {
      const bool dp = dec_c[I * B + p];
#pragma unroll
      for (int q = 0; q < B; ++q) Sc[(I * NST + k) * B * B + p * B + q] = dp ? ((k == NST / 2 && p == q) ? diag_c[I * B + p] : 0.0) : acc[p][q];
    }
  }
}

// 1 / diagonal of a stencil level
template <int B, int D>
__global__ void mg_dinv_kernel(int64_t nn, const double* __restrict__ S, double* __restrict__ dinv) {
  constexpr int NST = D == 3 ? 27 : 9;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nn * B; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = r / B;
    const int p = (int)(r - i * B);
    dinv[r] = 1.0 / S[(i * NST + NST / 2) * B * B + p * B + p];
  }
}

// dense image of the coarsest stencil (D zeroed before)
template <int B, int D>
__global__ void mg_dense_kernel(Grid cg, const double* __restrict__ S, double* __restrict__ Dm, int64_t n) {
  constexpr int NST = D == 3 ? 27 : 9;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cg.nodes() * NST; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tn = t / NST;
    const int k = (int)(t - tn * NST);
    int X, Y, Z, ox, oy, oz;
    cg.lex(tn, X, Y, Z);
    st_off<D>(k, ox, oy, oz);
    if (!cg.in(X + ox, Y + oy, Z + oz)) continue;
    const int64_t I = cg.id(X, Y, Z), J = cg.id(X + ox, Y + oy, Z + oz);
    for (int p = 0; p < B; ++p)
      for (int q = 0; q < B; ++q) Dm[(I * B + p) * n + J * B + q] = S[(I * NST + k) * B * B + p * B + q];
  }
}

// ---- cycle kernels: thread per node, its B components in registers -----------------------------------------------------------

template <int B, int D>
__device__ __forceinline__ void stencil_row(const Grid& g, const double* __restrict__ S, const double* __restrict__ x, int X, int Y, int Z,
                                            int64_t I, double (&y)[B]) {
  constexpr int NST = D == 3 ? 27 : 9;
#pragma unroll
  for (int p = 0; p < B; ++p) y[p] = 0.0;
  const double* s = S + I * NST * B * B;
#pragma unroll
  for (int k = 0; k < NST; ++k) {
    int ox, oy, oz;
    st_off<D>(k, ox, oy, oz);
    if (!g.in(X + ox, Y + oy, Z + oz)) continue;
    const int64_t J = g.id(X + ox, Y + oy, Z + oz);
    double xj[B];
#pragma unroll
    for (int q = 0; q < B; ++q) xj[q] = x[J * B + q];
#pragma unroll
    for (int p = 0; p < B; ++p)
#pragma unroll
      for (int q = 0; q < B; ++q) y[p] = fma(s[(k * B + p) * B + q], xj[q], y[p]);
  }
}

// y = S x
template <int B, int D>
__global__ void __launch_bounds__(256) mg_apply_kernel(Grid g, const double* __restrict__ S, const double* __restrict__ x, double* __restrict__ y) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int X, Y, Z;
    g.lex(t, X, Y, Z);
    const int64_t I = g.id(X, Y, Z);
    double v[B];
    stencil_row<B, D>(g, S, x, X, Y, Z, I, v);
#pragma unroll
    for (int p = 0; p < B; ++p) y[I * B + p] = v[p];
  }
}

// one Chebyshev step fused with the stencil product: t = r - S zin (zin = 0 when zero_in), d = c1 d + c2 D^-1 t, zout = zin + d;
// decoupled rows: zout = r / a_ii
template <int B, int D>
__global__ void __launch_bounds__(256) mg_cheb_kernel(Grid g, const double* __restrict__ S, const double* __restrict__ r,
                                                      const double* __restrict__ zin, double* __restrict__ zout, double* __restrict__ d,
                                                      const double* __restrict__ dinv, const uint8_t* __restrict__ dec,
                                                      const double* __restrict__ diag, double c1, double c2, int zero_in) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int X, Y, Z;
    g.lex(t, X, Y, Z);
    const int64_t I = g.id(X, Y, Z);
    double az[B];
    if (zero_in) {
#pragma unroll
      for (int p = 0; p < B; ++p) az[p] = 0.0;
    } else {
      stencil_row<B, D>(g, S, zin, X, Y, Z, I, az);
    }
#pragma unroll
    for (int p = 0; p < B; ++p) {
      const int64_t e = I * B + p;
      const double dn = fma(c2 * dinv[e], r[e] - az[p], zero_in ? 0.0 : c1 * d[e]);
      d[e] = dn;
      zout[e] = dec[e] ? r[e] / diag[e] : (zero_in ? dn : zin[e] + dn);
    }
  }
}

// level 0 (product supplied by the caller): t = r - Az (Az null: z = 0), d = c1 d + c2 D^-1 t, z += d; decoupled rows z = r / a_ii
__global__ void __launch_bounds__(256) mg_cheb0_kernel(const double* __restrict__ r, const double* __restrict__ Az, double* __restrict__ z,
                                                       double* __restrict__ d, const double* __restrict__ dinv, const uint8_t* __restrict__ dec,
                                                       const double* __restrict__ diag, double c1, double c2, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const double t = Az ? r[e] - Az[e] : r[e];
    const double dn = fma(c2 * dinv[e], t, Az ? c1 * d[e] : 0.0);
    d[e] = dn;
    z[e] = dec[e] ? r[e] / diag[e] : (Az ? z[e] + dn : dn);
  }
}

// r_c = P^T (r_f - A_f z_f): one thread per coarse node; the fine residuals come from the stencil (S_f non-null) or, on level 0,
// from the caller's product (Az_f)
template <int B, int D>
__global__ void __launch_bounds__(256) mg_restrict_kernel(Grid f, Grid cg, const double* __restrict__ Sf, const double* __restrict__ rf,
                                                          const double* __restrict__ zf, const double* __restrict__ Azf,
                                                          const uint8_t* __restrict__ dec_f, const uint8_t* __restrict__ dec_c,
                                                          double* __restrict__ rc) {
  constexpr int NST = D == 3 ? 27 : 9;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cg.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int X, Y, Z;
    cg.lex(t, X, Y, Z);
    const int64_t I = cg.id(X, Y, Z);
    double acc[B] = {};
    for (int a = 0; a < NST; ++a) {
      int ax, ay, az;
      st_off<D>(a, ax, ay, az);
      const int fx = 2 * X + ax, fy = 2 * Y + ay, fz = 2 * Z + az;
      if (!f.in(fx, fy, fz)) continue;
      const int64_t i = f.id(fx, fy, fz);
      double res[B];
      if (Sf) {
        stencil_row<B, D>(f, Sf, zf, fx, fy, fz, i, res);
#pragma unroll
        for (int p = 0; p < B; ++p) res[p] = rf[i * B + p] - res[p];
      } else {
#pragma unroll
        for (int p = 0; p < B; ++p) res[p] = rf[i * B + p] - Azf[i * B + p];
      }
      const double w = pw(ax) * pw(ay) * pw(az);
#pragma unroll
      for (int p = 0; p < B; ++p)
        if (!dec_f[i * B + p]) acc[p] = fma(w, res[p], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < B; ++p) rc[I * B + p] = dec_c[I * B + p] ? 0.0 : acc[p];
  }
}

// z_f += P e_c: one thread per fine node, its (up to 2^d) coarse parents
template <int B, int D>
__global__ void __launch_bounds__(256) mg_prolong_kernel(Grid f, Grid cg, const double* __restrict__ ec, const uint8_t* __restrict__ dec_f,
                                                         const uint8_t* __restrict__ dec_c, double* __restrict__ zf) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < f.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int x, y, z;
    f.lex(t, x, y, z);
    const int64_t i = f.id(x, y, z);
    double acc[B] = {};
    const int x0 = x >> 1, y0 = y >> 1, z0 = z >> 1;
    const int nxp = (x & 1) + 1, nyp = (y & 1) + 1, nzp = (z & 1) + 1;
    const double w = (nxp == 2 ? 0.5 : 1.0) * (nyp == 2 ? 0.5 : 1.0) * (nzp == 2 ? 0.5 : 1.0);
    for (int cz = 0; cz < nzp; ++cz)
      for (int cy = 0; cy < nyp; ++cy)
        for (int cx = 0; cx < nxp; ++cx) {
          const int64_t J = cg.id(x0 + cx, y0 + cy, z0 + cz);
#pragma unroll
          for (int p = 0; p < B; ++p)
            if (!dec_c[J * B + p]) acc[p] = fma(w, ec[J * B + p], acc[p]);
        }
#pragma unroll
    for (int p = 0; p < B; ++p)
      if (!dec_f[i * B + p]) zf[i * B + p] += acc[p];
  }
}

// ---- level 0 of order ngl >= 4: transfers between the GLL node lattice (M = ngl - 1 intervals per cell) and the Q1 lattice of the
// same cells.  1-D rule: fine node x = M e + i of cell e takes (1 - xi_i) / 2 of coarse node e and (1 + xi_i) / 2 of e + 1, i.e. the
// hat of coarse node X at fine node M X + t is hat[M + t], |t| < M, with hat[M + i] = (1 - xi_i) / 2 and hat[i] = (1 + xi_i) / 2
// (2 M + 1 doubles, copied to LDS by every workgroup; hat[0] = hat[2 M] = 0 are never used: a cell vertex has one parent).

// One axis of r_c = P0^T (r - A z), P0 a tensor product: out[ou][X][il] = sum_{|t| < M} hat[M + t] in[ou][M X + t][il], a thread per
// output node with its B components, the 2 M - 1 terms in ascending t.  FIRST (the x axis): `in` is r - Az at the level-0 node ids,
// decoupled fine DOFs left out.  LAST: decoupled coarse DOFs give 0.  No atomics: the same bits every time.
template <int B, int D, int M, bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) mg_ho_restrict_kernel(Grid f, const double* __restrict__ hatg, const double* __restrict__ in,
                                                             const double* __restrict__ Az, const uint8_t* __restrict__ dec_f,
                                                             const uint8_t* __restrict__ dec_c, double* __restrict__ out, int64_t ni,
                                                             int n, int N, int64_t total) {
  __shared__ double hat[2 * M + 1];
  if (threadIdx.x < 2 * M + 1) hat[threadIdx.x] = hatg[threadIdx.x];
  __syncthreads();
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t il = t % ni, q = t / ni;
    const int X = (int)(q % N);
    const int64_t ou = q / N;
    double acc[B] = {};
#pragma unroll
    for (int dt = -(M - 1); dt <= M - 1; ++dt) {
      const int a = M * X + dt;
      if (a < 0 || a >= n) continue;
      const double w = hat[M + dt];
      if (FIRST) {   // ni == 1: ou = y + ny z
        const int64_t i = f.id(a, (int)(ou % f.ny), (int)(ou / f.ny));
#pragma unroll
        for (int p = 0; p < B; ++p)
          if (!dec_f[i * B + p]) acc[p] = fma(w, Az ? in[i * B + p] - Az[i * B + p] : in[i * B + p], acc[p]);
      } else {
        const double* v = in + ((ou * n + a) * ni + il) * B;
#pragma unroll
        for (int p = 0; p < B; ++p) acc[p] = fma(w, v[p], acc[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < B; ++p) out[t * B + p] = (LAST && dec_c[t * B + p]) ? 0.0 : acc[p];
  }
}

// z_f += P0 e_c: one thread per fine node, its (up to 2^d) coarse parents, masked like mg_prolong_kernel
template <int B, int D, int M>
__global__ void __launch_bounds__(256) mg_ho_prolong_kernel(Grid f, Grid cg, const double* __restrict__ hatg, const double* __restrict__ ec,
                                                            const uint8_t* __restrict__ dec_f, const uint8_t* __restrict__ dec_c,
                                                            double* __restrict__ zf) {
  __shared__ double hat[2 * M + 1];
  if (threadIdx.x < 2 * M + 1) hat[threadIdx.x] = hatg[threadIdx.x];
  __syncthreads();
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < f.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int c[3];
    f.lex(t, c[0], c[1], c[2]);
    const int64_t i = f.id(c[0], c[1], c[2]);
    const int nc[3] = {cg.nx, cg.ny, cg.nz};
    int p0[3], np[3];        // first parent and parent count per axis
    double w[3][2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p0[a] = 0;
      np[a] = 1;
      w[a][0] = 1.0;
      w[a][1] = 0.0;
      if (a >= D) continue;
      const int e = min(c[a] / M, nc[a] - 2), k = c[a] - e * M;   // cell and local node 0 .. M (M: the far end of the last cell)
      p0[a] = k == M ? e + 1 : e;
      if (k != 0 && k != M) {
        np[a] = 2;
        w[a][0] = hat[M + k];
        w[a][1] = hat[k];
      }
    }
    double acc[B] = {};
#pragma unroll
    for (int cz = 0; cz < (D == 3 ? 2 : 1); ++cz)
#pragma unroll
      for (int cy = 0; cy < 2; ++cy)
#pragma unroll
        for (int cx = 0; cx < 2; ++cx) {
          if (cx >= np[0] || cy >= np[1] || cz >= np[2]) continue;
          const int64_t J = cg.id(p0[0] + cx, p0[1] + cy, p0[2] + cz);
          const double ww = w[0][cx] * w[1][cy] * w[2][cz];
#pragma unroll
          for (int p = 0; p < B; ++p)
            if (!dec_c[J * B + p]) acc[p] = fma(ww, ec[J * B + p], acc[p]);
        }
#pragma unroll
    for (int p = 0; p < B; ++p)
      if (!dec_f[i * B + p]) zf[i * B + p] += acc[p];
  }
}

// probing S1 = P0^T A P0 through the product: the unit vectors of one colour (coarse index mod 3 per axis) and component q ...
__global__ void mg_ho_seed_kernel(Grid cg, int b, int colour, int q, double* __restrict__ ec) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cg.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int x, y, z;
    cg.lex(t, x, y, z);
    const bool on = x % 3 == colour % 3 && y % 3 == (colour / 3) % 3 && (cg.dim == 2 || z % 3 == colour / 9);
    for (int p = 0; p < b; ++p) ec[cg.id(x, y, z) * b + p] = (on && p == q) ? 1.0 : 0.0;
  }
}

// ... and column q of the one stencil block of every coarse row that points at a node of that colour (S zeroed before: blocks that
// point outside the lattice stay zero); decoupled coarse rows are the coincident fine diagonal
__global__ void mg_ho_probe_store_kernel(Grid cg, int b, int colour, int q, const double* __restrict__ rc, const uint8_t* __restrict__ dec_c,
                                         const double* __restrict__ diag_c, double* __restrict__ S) {
  const int nst = cg.dim == 3 ? 27 : 9;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < cg.nodes(); t += (int64_t)gridDim.x * blockDim.x) {
    int x, y, z;
    cg.lex(t, x, y, z);
    const int col[3] = {colour % 3, (colour / 3) % 3, colour / 9}, c[3] = {x, y, z};
    int o[3] = {0, 0, 0};
    for (int a = 0; a < cg.dim; ++a) {
      const int d = (col[a] - c[a] % 3 + 3) % 3;
      o[a] = d == 2 ? -1 : d;
    }
    if (!cg.in(x + o[0], y + o[1], z + o[2])) continue;
    const int k = (o[0] + 1) + 3 * (o[1] + 1) + (cg.dim == 3 ? 9 * (o[2] + 1) : 0);
    const int64_t I = cg.id(x, y, z);
    for (int p = 0; p < b; ++p)
      S[((I * nst + k) * b + p) * b + q] = dec_c[I * b + p] ? ((k == nst / 2 && p == q) ? diag_c[I * b + p] : 0.0) : rc[I * b + p];
  }
}

// ---- eigenvalue estimate (CG with Jacobi, Lanczos coefficients) ------------------------------------------------------------
__global__ void __launch_bounds__(256) mg_dot_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n, double* __restrict__ part) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc = fma(x[i], y[i], acc);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// r -= alpha Ap ; z = dinv r  (alpha null: z = dinv r only)
__global__ void mg_eig_update_kernel(double* __restrict__ r, const double* __restrict__ Ap, const double* __restrict__ dinv, double* __restrict__ z,
                                     double alpha, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double ri = Ap ? r[i] - alpha * Ap[i] : r[i];
    r[i] = ri;
    z[i] = dinv[i] * ri;
  }
}

__global__ void mg_xpby_kernel(double* __restrict__ p, const double* __restrict__ z, double beta, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = z[i] + beta * p[i];
}

// largest eigenvalue of the symmetric tridiagonal (a, b) by Sturm-sequence bisection
double tridiag_max_eig(const std::vector<double>& a, const std::vector<double>& b) {
  const int m = (int)a.size();
  double lo = 0.0, hi = 0.0;
  for (int i = 0; i < m; ++i) {
    const double rad = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i + 1 < m ? fabs(b[i]) : 0.0);
    hi = std::max(hi, a[i] + rad);
    lo = std::min(lo, a[i] - rad);
  }
  auto count_below = [&](double x) {   // eigenvalues < x
    int cnt = 0;
    double q = 1.0;
    for (int i = 0; i < m; ++i) {
      q = a[i] - x - (i > 0 ? b[i - 1] * b[i - 1] / q : 0.0);
      if (q == 0.0) q = -1e-300;
      if (q < 0) ++cnt;
    }
    return cnt;
  };
  for (int it = 0; it < 200 && hi - lo > 1e-14 * std::max(1.0, fabs(hi)); ++it) {
    const double mid = 0.5 * (lo + hi);
    if (count_below(mid) >= m) hi = mid;
    else lo = mid;
  }
  return hi;
}

}  // namespace

// ---- hierarchy -----------------------------------------------------------------------------------------------------------------
struct MgLevel {
  int nx = 0, ny = 0, nz = 0;
  int64_t nn = 0;                // nodes
  DevBuf<int32_t> P;             // [planes]
  DevBuf<int32_t> invP;          // [planes]
  DevBuf<double> S;              // stencil (levels >= 1)
  DevBuf<double> dinv;           // levels >= 1 (level 0: the matrix's own DMat::dinv)
  DevBuf<double> diag;           // a_ii [nn b]
  DevBuf<uint8_t> dec;           // decoupled DOF [nn b]
  DevBuf<double> b;              // right-hand side of the level's cycle (levels >= 1)
  DevBuf<double> z[2];           // ping-pong iterates (levels >= 1); z[0] also the product scratch of level 0
  DevBuf<double> d;              // Chebyshev direction
  double lam = 0.0;              // lambda_max(D^-1 A) estimate
};

struct MgHier {
  pyn_mg_opts opts{};
  int dim = 0, b = 0, nlev = 0;
  MgLevel L[PYN_MG_MAX_LEVELS];
  DevBuf<double> lu;
  DevBuf<int> piv;
  int64_t lu_n = 0;
  double setup_ms = 0.0;
  int builds = 0;
  // level 0 of order ngl >= 4 (ho_m = ngl - 1 > 0): level 1 is the Q1 lattice of the same cells, the 0 <-> 1 transfers are the
  // mg_ho kernels; 0: every step halves (kinds 1, 2, 3)
  int ho_m = 0;
  DevBuf<double> ho_hat;         // [2 ho_m + 1] 1-D weights
  DevBuf<double> ho_tmp[2];      // stages of the axis-by-axis restriction
  void free_levels() {           // a rebuild keeps the options and the counters
    ho_hat.reset();
    ho_tmp[0].reset();
    ho_tmp[1].reset();
    ho_m = 0;
    for (auto& l : L) l = MgLevel();
    lu.reset();
    piv.reset();
    lu_n = 0;
    nlev = 0;
  }
};

void MgHierDelete::operator()(MgHier* h) const { delete h; }

static pyn_mg_opts mg_defaults(const pyn_mg_opts* in) {
  pyn_mg_opts o{};
  if (in) o = *in;
  if (o.max_levels <= 0) o.max_levels = PYN_MG_MAX_LEVELS;
  if (o.smooth_degree <= 0) o.smooth_degree = 2;
  if (o.coarse_max_rows <= 0) o.coarse_max_rows = 4096;
  if (o.esteig_its <= 0) o.esteig_its = 10;
  if (o.esteig_min <= 0.0) o.esteig_min = 0.1;
  if (o.esteig_max <= 0.0) o.esteig_max = 1.1;
  return o;
}

static bool same_opts(const pyn_mg_opts& a, const pyn_mg_opts& b) {
  return a.max_levels == b.max_levels && a.smooth_degree == b.smooth_degree && a.coarse_max_rows == b.coarse_max_rows &&
         a.esteig_its == b.esteig_its && a.esteig_min == b.esteig_min && a.esteig_max == b.esteig_max;
}

static Grid grid_of(const MgHier& H, int l) {
  const MgLevel& L = H.L[l];
  return Grid{H.dim, L.nx, L.ny, L.nz, L.P, L.invP};
}

#define PYN_MG_DISPATCH(B, D, CALL)                                         \
  do {                                                                      \
    if ((D) == 2) {                                                         \
      if ((B) == 1) { constexpr int B_ = 1, D_ = 2; CALL; }                 \
      else if ((B) == 2) { constexpr int B_ = 2, D_ = 2; CALL; }            \
      else { constexpr int B_ = 3, D_ = 2; CALL; }                          \
    } else {                                                                \
      if ((B) == 1) { constexpr int B_ = 1, D_ = 3; CALL; }                 \
      else if ((B) == 2) { constexpr int B_ = 2, D_ = 3; CALL; }            \
      else { constexpr int B_ = 3, D_ = 3; CALL; }                          \
    }                                                                       \
  } while (0)

// the same with the order of a high-order level 0: M_ = ngl - 1 (the orders of pyn_ho_matfree_max_ngl)
#define PYN_MG_HO_CASE(B, D, M, CALL) case M: PYN_MG_DISPATCH_D(B, D, M, CALL); break;
#define PYN_MG_DISPATCH_D(B, D, M, CALL)                                    \
  do {                                                                      \
    constexpr int M_ = M;                                                   \
    if ((B) == 1) { constexpr int B_ = 1, D_ = D; CALL; }                   \
    else if ((B) == 2) { constexpr int B_ = 2, D_ = D; CALL; }              \
    else { constexpr int B_ = 3, D_ = D; CALL; }                            \
  } while (0)
#define PYN_MG_HO_DISPATCH(B, D, M, CALL)                                   \
  do {                                                                      \
    static_assert(PYN_HO_MAX_NGL_2D == 12 && PYN_HO_MAX_NGL_3D == 8, "orders of the transfer kernels"); \
    if ((D) == 2) switch (M) {                                              \
        PYN_MG_HO_CASE(B, 2, 3, CALL) PYN_MG_HO_CASE(B, 2, 4, CALL) PYN_MG_HO_CASE(B, 2, 5, CALL) PYN_MG_HO_CASE(B, 2, 6, CALL) \
        PYN_MG_HO_CASE(B, 2, 7, CALL) PYN_MG_HO_CASE(B, 2, 8, CALL) PYN_MG_HO_CASE(B, 2, 9, CALL) PYN_MG_HO_CASE(B, 2, 10, CALL) \
        PYN_MG_HO_CASE(B, 2, 11, CALL)                                      \
      }                                                                     \
    else switch (M) {                                                       \
        PYN_MG_HO_CASE(B, 3, 3, CALL) PYN_MG_HO_CASE(B, 3, 4, CALL) PYN_MG_HO_CASE(B, 3, 5, CALL) PYN_MG_HO_CASE(B, 3, 6, CALL) \
        PYN_MG_HO_CASE(B, 3, 7, CALL)                                       \
      }                                                                     \
  } while (0)

// r_c = P0^T (in - Az) (Az null: P0^T in), axis by axis: x into ho_tmp[0], y into rc (2-D) or ho_tmp[1], z into rc
static int mg_ho_restrict(pyn_ctx* c, MgHier& H, const double* in, const double* Az, double* rc) {
  const MgLevel &F = H.L[0], &C = H.L[1];
  const Grid gf = grid_of(H, 0);
  hipStream_t s = c->stream;
  const int b = H.b, dim = H.dim, m = H.ho_m;
  const int64_t t0 = (int64_t)C.nx * F.ny * F.nz, t1 = (int64_t)C.nx * C.ny * F.nz, t2 = (int64_t)C.nx * C.ny * C.nz;
  PYN_MG_HO_DISPATCH(b, dim, m, (mg_ho_restrict_kernel<B_, D_, M_, true, false><<<grid_for(t0), 256, 0, s>>>(
                                    gf, H.ho_hat, in, Az, F.dec, nullptr, H.ho_tmp[0], 1, F.nx, C.nx, t0)));
  if (dim == 2) {
    PYN_MG_HO_DISPATCH(b, dim, m, (mg_ho_restrict_kernel<B_, D_, M_, false, true><<<grid_for(t1), 256, 0, s>>>(
                                      gf, H.ho_hat, H.ho_tmp[0], nullptr, nullptr, C.dec, rc, C.nx, F.ny, C.ny, t1)));
  } else {
    PYN_MG_HO_DISPATCH(b, dim, m, (mg_ho_restrict_kernel<B_, D_, M_, false, false><<<grid_for(t1), 256, 0, s>>>(
                                      gf, H.ho_hat, H.ho_tmp[0], nullptr, nullptr, nullptr, H.ho_tmp[1], C.nx, F.ny, C.ny, t1)));
    PYN_MG_HO_DISPATCH(b, dim, m, (mg_ho_restrict_kernel<B_, D_, M_, false, true><<<grid_for(t2), 256, 0, s>>>(
                                      gf, H.ho_hat, H.ho_tmp[1], nullptr, nullptr, C.dec, rc, (int64_t)C.nx * C.ny, F.nz, C.nz, t2)));
  }
  return PYN_OK;
}

// z_f += P0 e_c
static int mg_ho_prolong(pyn_ctx* c, MgHier& H, const double* ec, double* zf) {
  const MgLevel &F = H.L[0], &C = H.L[1];
  const Grid gf = grid_of(H, 0), gc = grid_of(H, 1);
  PYN_MG_HO_DISPATCH(H.b, H.dim, H.ho_m, (mg_ho_prolong_kernel<B_, D_, M_><<<grid_for(F.nn), 256, 0, c->stream>>>(gf, gc, H.ho_hat, ec, F.dec,
                                                                                                                 C.dec, zf)));
  return PYN_OK;
}

// the level-0 product of the set-up: the assembled matrix, through the image the CG loop uses
static int mg_assembled_product(pyn_ctx* c, DMat& A, const double* x, double* y) {
  LinOp op;
  PYN_TRY(op.init(c, A, PYN_MATFREE_OFF));
  return op.apply(x, y);
}

static int mg_dot(pyn_ctx* c, const double* x, const double* y, int64_t n, double* out) {
  const int g = (int)std::max<int64_t>(1, std::min<int64_t>((n + 511) / 512, PYN_MAX_PARTIALS));
  mg_dot_kernel<<<g, 256, 0, c->stream>>>(x, y, n, c->d_part);
  return pyn_reduce_host(c, 1, g, 0, out);
}

// lambda_max(D^-1 A) of level l from `its` CG steps on a seeded random right-hand side (the Lanczos matrix of the CG coefficients)
static int mg_estimate(pyn_ctx* c, DMat& A, MgHier& H, int l, double* lam) {
  MgLevel& L = H.L[l];
  const int64_t n = L.nn * H.b;
  DevTmp tmp;
  PYN_HIP(tmp.alloc((size_t)4 * n * sizeof(double)));
  double *r = tmp.as<double>(), *z = r + n, *p = z + n, *Ap = p + n;
  std::vector<double> h(n);
  uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)(l + 1);
  for (int64_t i = 0; i < n; ++i) {   // splitmix64 -> uniform [-1, 1)
    uint64_t v = (s += 0x9E3779B97F4A7C15ull);
    v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
    v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
    v ^= v >> 31;
    h[i] = (double)(v >> 11) * (2.0 / 9007199254740992.0) - 1.0;
  }
  PYN_HIP(hipMemcpyAsync(r, h.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const double* dinv = l == 0 ? A.dinv.get() : L.dinv.get();
  const Grid g = grid_of(H, l);
  mg_eig_update_kernel<<<grid_for(n), 256, 0, c->stream>>>(r, nullptr, dinv, z, 0.0, n);
  PYN_HIP(hipMemcpyAsync(p, z, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  double rz = 0.0;
  PYN_TRY(mg_dot(c, r, z, n, &rz));
  std::vector<double> alpha, beta;
  for (int j = 0; j < H.opts.esteig_its && rz > 0.0; ++j) {
    if (l == 0) PYN_TRY(mg_assembled_product(c, A, p, Ap));
    else PYN_MG_DISPATCH(H.b, H.dim, (mg_apply_kernel<B_, D_><<<grid_for(L.nn), 256, 0, c->stream>>>(g, L.S, p, Ap)));
    double pap = 0.0;
    PYN_TRY(mg_dot(c, p, Ap, n, &pap));
    if (!(pap > 0.0)) break;
    const double a = rz / pap;
    mg_eig_update_kernel<<<grid_for(n), 256, 0, c->stream>>>(r, Ap, dinv, z, a, n);
    double rz1 = 0.0;
    PYN_TRY(mg_dot(c, r, z, n, &rz1));
    const double bt = rz1 / rz;
    alpha.push_back(a);
    beta.push_back(bt);
    rz = rz1;
    mg_xpby_kernel<<<grid_for(n), 256, 0, c->stream>>>(p, z, bt, n);
  }
  PYN_HIP(hipGetLastError());
  PYN_CHECK(!alpha.empty(), "multigrid: the eigenvalue estimate of level %d found no positive curvature (is the matrix SPD?)", l);
  const int m = (int)alpha.size();
  std::vector<double> ta(m), tb(std::max(0, m - 1));
  for (int j = 0; j < m; ++j) {
    ta[j] = 1.0 / alpha[j] + (j > 0 ? beta[j - 1] / alpha[j - 1] : 0.0);
    if (j + 1 < m) tb[j] = sqrt(beta[j]) / alpha[j];
  }
  *lam = tridiag_max_eig(ta, tb);
  return PYN_OK;
}

// S1 = P0^T A P0 of a high-order level 0, probed through the assembled product: a fine row reaches the nodes of its own cells, so
// coarse nodes couple at +-1 per axis and the unit vectors of one colour (index mod 3 per axis) and one component do not overlap.
// 3^dim b products per build; every kernel of the chain has a fixed summation order, so two builds give the same bits.
static int mg_ho_probe(pyn_ctx* c, DMat& A, MgHier& H) {
  MgLevel &F = H.L[0], &C = H.L[1];
  hipStream_t s = c->stream;
  const int b = H.b, nst = H.dim == 3 ? 27 : 9;
  const Grid gc = grid_of(H, 1);
  const size_t nf = (size_t)F.nn * b * sizeof(double);
  double *v = F.z[0], *y = F.d, *ec = C.z[0], *rc = C.b;   // free until the first cycle
  LinOp op;
  PYN_TRY(op.init(c, A, PYN_MATFREE_OFF));
  PYN_HIP(hipMemsetAsync(C.S, 0, (size_t)C.nn * nst * b * b * sizeof(double), s));
  for (int colour = 0; colour < nst; ++colour)
    for (int q = 0; q < b; ++q) {
      mg_ho_seed_kernel<<<grid_for(C.nn), 256, 0, s>>>(gc, b, colour, q, ec);
      PYN_HIP(hipMemsetAsync(v, 0, nf, s));
      PYN_TRY(mg_ho_prolong(c, H, ec, v));
      PYN_TRY(op.apply(v, y));
      PYN_TRY(mg_ho_restrict(c, H, y, nullptr, rc));
      mg_ho_probe_store_kernel<<<grid_for(C.nn), 256, 0, s>>>(gc, b, colour, q, rc, C.dec, C.diag, C.S);
    }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

static int mg_build(pyn_ctx* c, DMat& A, const pyn_mg_opts& o) {
  PYN_CHECK(c->nranks == 1 && c->n_ghost == 0, "multigrid: the preconditioner runs on one rank without ghost nodes (%d ranks, %lld ghosts)",
            c->nranks, (long long)c->n_ghost);
  PYN_CHECK(A.br == A.bc, "multigrid: the matrix must have square blocks (%d x %d)", A.br, A.bc);
  PYN_CHECK(A.br >= 1 && A.br <= 3, "multigrid: block size %d (1, 2 or 3 DOFs per node)", A.br);
  PYN_CHECK(!A.rhs_compact, "multigrid: a compact imposed-column matrix (pyn_mat_create_rhs) is not a system matrix");
  // the node lattice of level 0: pyn_mesh_topology's kinds 1, 2 and 3, or a box lattice of order ngl >= 4 (kind 0, pyn_ctx::ho_valid)
  const BoxLattice& B = c->box;
  const int ho_m = (!pyn_lattice_kind(c) && c->ho_valid) ? B.ngl - 1 : 0;
  const int dim = (pyn_lattice_kind(c) || ho_m) ? B.dim : 0, nx = B.NX, ny = B.ny(), nz = B.nz();
  const std::vector<int32_t>& P = B.P;
  PYN_CHECK(dim > 0, "multigrid: needs a structured lattice mesh (pyn_mesh_topology kind 1, 2 or 3); this mesh has general connectivity (kind 0)");
  const int planes = B.npl;
  const int64_t plane = B.plane();
  PYN_CHECK((int64_t)planes * plane == c->n_owned && (int)P.size() == planes, "multigrid: the lattice (%d x %d x %d) does not cover the %lld owned nodes",
            nx, ny, nz, (long long)c->n_owned);
  std::vector<int32_t> invP(planes, -1);
  for (int j = 0; j < planes; ++j) {
    PYN_CHECK(P[j] % plane == 0 && P[j] / plane < planes && invP[P[j] / plane] < 0, "multigrid: lattice planes are not whole blocks of node ids");
    invP[P[j] / plane] = j;
  }
  // levels
  const int b = A.br;
  int dims[PYN_MG_MAX_LEVELS][3];
  dims[0][0] = nx;
  dims[0][1] = ny;
  dims[0][2] = nz;
  int nlev = 1;
  auto rows = [&](int l) { return (int64_t)dims[l][0] * dims[l][1] * dims[l][2] * b; };
  while (nlev < std::min(o.max_levels, PYN_MG_MAX_LEVELS) && rows(nlev - 1) > o.coarse_max_rows) {
    const int* d = dims[nlev - 1];
    const int m = (nlev == 1 && ho_m) ? ho_m : 2;   // order ngl >= 4: the first step goes to the Q1 lattice of the same cells, whatever their count
    bool even = true;
    for (int a = 0; a < dim; ++a) even = even && d[a] > 1 && (d[a] - 1) % m == 0;
    if (!even) break;
    for (int a = 0; a < 3; ++a) dims[nlev][a] = a < dim ? (d[a] - 1) / m + 1 : 1;
    ++nlev;
  }
  PYN_CHECK(nlev >= 2, "multigrid: fewer than 2 levels possible (lattice %d x %d x %d nodes, %lld rows; coarse_max_rows %d, max_levels %d: "
            "coarsening needs an even number of cells on every axis and more rows than coarse_max_rows)",
            nx, ny, nz, (long long)rows(0), o.coarse_max_rows, o.max_levels);
  PYN_CHECK(rows(nlev - 1) <= pyn_direct_max_rows(), "multigrid: the coarsest level (%d x %d x %d nodes) has %lld rows, above the dense LU limit "
            "of %d (an odd cell count stops the coarsening; raise max_levels or lower coarse_max_rows)",
            dims[nlev - 1][0], dims[nlev - 1][1], dims[nlev - 1][2], (long long)rows(nlev - 1), pyn_direct_max_rows());

  const auto t0 = std::chrono::steady_clock::now();
  if (!A.mg) A.mg.reset(new MgHier());
  MgHier& H = *A.mg;
  H.free_levels();
  A.mg_valid = false;
  H.opts = o;
  H.dim = dim;
  H.b = b;
  H.nlev = nlev;
  H.ho_m = ho_m;
  hipStream_t s = c->stream;
  if (ho_m) {   // the 1-D weights from the library's own Lobatto nodes; the stage buffers of the restriction
    std::vector<double> xi(ho_m + 1), hat(2 * ho_m + 1);
    PYN_TRY(pyn_ho_tables_1d(ho_m + 1, xi.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    for (int i = 0; i <= ho_m; ++i) {
      hat[ho_m + i] = 0.5 * (1.0 - xi[i]);
      hat[i] = 0.5 * (1.0 + xi[i]);
    }
    PYN_HIP(H.ho_hat.alloc(hat.size()));
    PYN_HIP(hipMemcpy(H.ho_hat, hat.data(), hat.size() * sizeof(double), hipMemcpyHostToDevice));
    PYN_HIP(H.ho_tmp[0].alloc((size_t)dims[1][0] * ny * nz * b));
    if (dim == 3) PYN_HIP(H.ho_tmp[1].alloc((size_t)dims[1][0] * dims[1][1] * nz * b));
  }
  for (int l = 0; l < nlev; ++l) {
    MgLevel& L = H.L[l];
    L.nx = dims[l][0];
    L.ny = dims[l][1];
    L.nz = dims[l][2];
    L.nn = (int64_t)L.nx * L.ny * L.nz;
    const int pl = dim == 3 ? L.nz : L.ny;
    const int64_t pls = dim == 3 ? (int64_t)L.nx * L.ny : L.nx;
    std::vector<int32_t> lp(pl), li(pl);
    for (int j = 0; j < pl; ++j) {
      lp[j] = l == 0 ? P[j] : (int32_t)(j * pls);
      li[j] = l == 0 ? invP[j] : j;
    }
    const int64_t n = L.nn * b;
    PYN_HIP(L.P.alloc(pl));
    PYN_HIP(L.invP.alloc(pl));
    PYN_HIP(hipMemcpy(L.P, lp.data(), pl * sizeof(int32_t), hipMemcpyHostToDevice));
    PYN_HIP(hipMemcpy(L.invP, li.data(), pl * sizeof(int32_t), hipMemcpyHostToDevice));
    PYN_HIP(L.diag.alloc(n));
    PYN_HIP(L.dec.alloc(n));
    PYN_HIP(L.z[0].alloc(n));
    PYN_HIP(L.d.alloc(n));
    if (l > 0) {
      const int nst = dim == 3 ? 27 : 9;
      PYN_HIP(L.S.alloc((size_t)L.nn * nst * b * b));
      PYN_HIP(L.dinv.alloc(n));
      PYN_HIP(L.b.alloc(n));
      PYN_HIP(L.z[1].alloc(n));
    }
  }
  PYN_TRY(pyn_dinv_ensure(c, A));
  mg_decouple0_kernel<<<grid_for(c->n_owned * b), 256, 0, s>>>(c->d_rowptr, c->d_colidx, A.val, c->n_owned, b, H.L[0].dec, H.L[0].diag);
  DevTmp dbad;
  PYN_HIP(dbad.alloc(sizeof(int)));
  PYN_HIP(hipMemsetAsync(dbad.get(), 0, sizeof(int), s));
  for (int l = 1; l < nlev; ++l) {
    MgLevel &F = H.L[l - 1], &C = H.L[l];
    const Grid gf = grid_of(H, l - 1), gc = grid_of(H, l);
    mg_coarse_dec_kernel<<<grid_for(C.nn), 256, 0, s>>>(gf, gc, b, (l == 1 && ho_m) ? ho_m : 2, F.dec, F.diag, C.dec, C.diag);
    if (l == 1 && ho_m)
      PYN_TRY(mg_ho_probe(c, A, H));
    else if (l == 1)
      PYN_MG_DISPATCH(b, dim, (mg_galerkin0_kernel<B_, D_><<<(int)std::min<int64_t>(C.nn, 1 << 20), 64, 0, s>>>(
                                  gf, gc, c->d_rowptr, c->d_colidx, A.val, F.dec, C.dec, C.diag, C.S, dbad.as<int>())));
    else
      PYN_MG_DISPATCH(b, dim, (mg_galerkin_kernel<B_, D_><<<grid_for(C.nn * (dim == 3 ? 27 : 9)), 256, 0, s>>>(gf, gc, F.S, F.dec, C.dec, C.diag, C.S)));
    PYN_MG_DISPATCH(b, dim, (mg_dinv_kernel<B_, D_><<<grid_for(C.nn * b), 256, 0, s>>>(C.nn, C.S, C.dinv)));
  }
  int bad = 0;
  PYN_HIP(hipMemcpyAsync(&bad, dbad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  PYN_HIP(hipStreamSynchronize(s));
  PYN_HIP(hipGetLastError());
  PYN_CHECK(!bad, "multigrid: a row of the matrix reaches further than 2 lattice nodes (not a Q1 / ngl 3 lattice operator)");
  // coarsest: dense LU
  {
    MgLevel& C = H.L[nlev - 1];
    const int64_t n = C.nn * b;
    PYN_HIP(H.lu.alloc((size_t)n * n));
    PYN_HIP(H.piv.alloc((size_t)(2 * n + 1)));
    H.lu_n = n;
    PYN_HIP(hipMemsetAsync(H.lu, 0, (size_t)n * n * sizeof(double), s));
    const Grid gc = grid_of(H, nlev - 1);
    PYN_MG_DISPATCH(b, dim, (mg_dense_kernel<B_, D_><<<grid_for(C.nn * (dim == 3 ? 27 : 9)), 256, 0, s>>>(gc, C.S, H.lu, n)));
    PYN_TRY(pyn_dense_lu_factor(c, H.lu, H.piv, n));
  }
  for (int l = 0; l + 1 < nlev; ++l) PYN_TRY(mg_estimate(c, A, H, l, &H.L[l].lam));
  PYN_HIP(hipStreamSynchronize(s));
  H.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  H.builds++;
  A.mg_valid = true;
  return PYN_OK;
}

int pyn_mg_ensure(pyn_ctx* c, DMat& A) {
  if (A.mg_valid && A.mg) return PYN_OK;
  return mg_build(c, A, mg_defaults(A.mg ? &A.mg->opts : nullptr));
}

// Chebyshev coefficients of step j (j = 0: the first, c2 = 1 / theta)
static void cheb_coef(const MgHier& H, double lam, int j, double* rho, double* c1, double* c2) {
  const double emin = H.opts.esteig_min * lam, emax = H.opts.esteig_max * lam;
  const double theta = 0.5 * (emax + emin), delta = 0.5 * (emax - emin), sigma = theta / delta;
  if (j == 0) {
    *rho = 1.0 / sigma;
    *c1 = 0.0;
    *c2 = 1.0 / theta;
    return;
  }
  const double rn = 1.0 / (2.0 * sigma - *rho);
  *c1 = rn * *rho;
  *c2 = 2.0 * rn / delta;
  *rho = rn;
}

// V-cycle on level l >= 1: the right-hand side is L.b, the result is left in *out (one of L.z)
static int vcycle_level(pyn_ctx* c, MgHier& H, int l, double** out) {
  MgLevel& L = H.L[l];
  hipStream_t s = c->stream;
  const int b = H.b, dim = H.dim;
  if (l == H.nlev - 1) {
    PYN_TRY(pyn_dense_lu_solve(c, H.lu, H.piv, H.lu_n, L.b, L.z[0], L.d));
    *out = L.z[0];
    return PYN_OK;
  }
  const Grid g = grid_of(H, l), gc = grid_of(H, l + 1);
  const int k = H.opts.smooth_degree, gn = grid_for(L.nn);
  int cur = 0;
  double rho = 0, c1 = 0, c2 = 0;
  // pre-smoothing from zero
  for (int j = 0; j < k; ++j) {
    cheb_coef(H, L.lam, j, &rho, &c1, &c2);
    PYN_MG_DISPATCH(b, dim, (mg_cheb_kernel<B_, D_><<<gn, 256, 0, s>>>(g, L.S, L.b, L.z[cur], L.z[cur ^ (j > 0)], L.d, L.dinv, L.dec, L.diag, c1,
                                                                       c2, j == 0)));
    if (j > 0) cur ^= 1;
  }
  // residual -> coarse right-hand side, coarse correction, prolongation
  MgLevel& C = H.L[l + 1];
  PYN_MG_DISPATCH(b, dim, (mg_restrict_kernel<B_, D_><<<grid_for(C.nn), 256, 0, s>>>(g, gc, L.S, L.b, L.z[cur], nullptr, L.dec, C.dec, C.b)));
  double* ec = nullptr;
  PYN_TRY(vcycle_level(c, H, l + 1, &ec));
  PYN_MG_DISPATCH(b, dim, (mg_prolong_kernel<B_, D_><<<gn, 256, 0, s>>>(g, gc, ec, L.dec, C.dec, L.z[cur])));
  // post-smoothing: z += S (r - A z), the same polynomial
  for (int j = 0; j < k; ++j) {
    cheb_coef(H, L.lam, j, &rho, &c1, &c2);
    PYN_MG_DISPATCH(b, dim, (mg_cheb_kernel<B_, D_><<<gn, 256, 0, s>>>(g, L.S, L.b, L.z[cur], L.z[cur ^ 1], L.d, L.dinv, L.dec, L.diag,
                                                                       j == 0 ? 0.0 : c1, c2, 0)));
    cur ^= 1;
  }
  *out = L.z[cur];
  return PYN_OK;
}

int pyn_mg_vcycle(pyn_ctx* c, DMat& A, const double* r, double* z, const LinOp& prod0) {
  MgHier& H = *A.mg;
  MgLevel& L = H.L[0];
  hipStream_t s = c->stream;
  const int b = H.b, dim = H.dim;
  const int64_t n = L.nn * b;
  const int gv = grid_for(n), k = H.opts.smooth_degree;
  double* Az = L.z[0];
  double rho = 0, c1 = 0, c2 = 0;
  for (int j = 0; j < k; ++j) {   // pre-smoothing from zero
    cheb_coef(H, L.lam, j, &rho, &c1, &c2);
    if (j > 0) PYN_TRY(prod0.apply(z, Az));
    mg_cheb0_kernel<<<gv, 256, 0, s>>>(r, j > 0 ? Az : nullptr, z, L.d, A.dinv, L.dec, L.diag, c1, c2, n);
  }
  const Grid g = grid_of(H, 0), gc = grid_of(H, 1);
  MgLevel& C = H.L[1];
  PYN_TRY(prod0.apply(z, Az));
  if (H.ho_m)
    PYN_TRY(mg_ho_restrict(c, H, r, Az, C.b));
  else
    PYN_MG_DISPATCH(b, dim, (mg_restrict_kernel<B_, D_><<<grid_for(C.nn), 256, 0, s>>>(g, gc, nullptr, r, nullptr, Az, L.dec, C.dec, C.b)));
  double* ec = nullptr;
  PYN_TRY(vcycle_level(c, H, 1, &ec));
  if (H.ho_m)
    PYN_TRY(mg_ho_prolong(c, H, ec, z));
  else
    PYN_MG_DISPATCH(b, dim, (mg_prolong_kernel<B_, D_><<<grid_for(L.nn), 256, 0, s>>>(g, gc, ec, L.dec, C.dec, z)));
  for (int j = 0; j < k; ++j) {   // post-smoothing
    cheb_coef(H, L.lam, j, &rho, &c1, &c2);
    PYN_TRY(prod0.apply(z, Az));
    // the first post step starts a new polynomial: d = D^-1 t / theta (c1 = 0), z += d
    mg_cheb0_kernel<<<gv, 256, 0, s>>>(r, Az, z, L.d, A.dinv, L.dec, L.diag, j == 0 ? 0.0 : c1, c2, n);
  }
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" int pyn_mg_setup(pyn_ctx* c, int mat_id, const pyn_mg_opts* opts) {
  PYN_TRY(pyn_check_mat(c, mat_id, "pyn_mg_setup"));
  DMat& A = c->mats[mat_id];
  const pyn_mg_opts o = mg_defaults(opts);
  PYN_CHECK(o.esteig_min < o.esteig_max, "multigrid: esteig bounds must satisfy min < max (%g, %g)", o.esteig_min, o.esteig_max);
  PYN_HIP(hipSetDevice(c->device));
  if (A.mg_valid && A.mg && same_opts(A.mg->opts, o)) return PYN_OK;
  return mg_build(c, A, o);
}

extern "C" int pyn_mg_info(pyn_ctx* c, int mat_id, int* nlevels, int64_t* rows, double* lam, double* setup_ms, int* builds) {
  PYN_TRY(pyn_check_mat(c, mat_id, "pyn_mg_info"));
  DMat& A = c->mats[mat_id];
  PYN_CHECK(A.mg && A.mg_valid, "multigrid: no hierarchy for the current values of matrix %d (pyn_mg_setup or a PYN_PC_MG solve first)", mat_id);
  const MgHier& H = *A.mg;
  if (nlevels) *nlevels = H.nlev;
  for (int l = 0; l < PYN_MG_MAX_LEVELS; ++l) {
    if (rows) rows[l] = l < H.nlev ? H.L[l].nn * H.b : 0;
    if (lam) lam[l] = l < H.nlev ? H.L[l].lam : 0.0;
  }
  if (setup_ms) *setup_ms = H.setup_ms;
  if (builds) *builds = H.builds;
  return PYN_OK;
}

extern "C" int pyn_mg_apply(pyn_ctx* c, int mat_id, int rv, int zv) {
  PYN_TRY(pyn_check_mat(c, mat_id, "pyn_mg_apply"));
  PYN_TRY(pyn_check_vec(c, rv, "pyn_mg_apply r"));
  PYN_TRY(pyn_check_vec(c, zv, "pyn_mg_apply z"));
  PYN_CHECK(rv != zv, "r and z must differ");
  DMat& A = c->mats[mat_id];
  PYN_CHECK(c->vecs[rv].bs == A.br && c->vecs[zv].bs == A.br, "vector block size mismatch");
  PYN_HIP(hipSetDevice(c->device));
  PYN_TRY(pyn_mg_ensure(c, A));
  PYN_TRY(pyn_dinv_ensure(c, A));
  LinOp op;
  PYN_TRY(op.init(c, A, PYN_MATFREE_OFF));
  PYN_TRY(pyn_mg_vcycle(c, A, c->vecs[rv].d, c->vecs[zv].d, op));
  PYN_HIP(hipStreamSynchronize(c->stream));
  PYN_HIP(hipGetLastError());
  return PYN_OK;
}

extern "C" int pyn_mg_level_get(pyn_ctx* c, int mat_id, int level, double* out) {
  PYN_TRY(pyn_check_mat(c, mat_id, "pyn_mg_level_get"));
  PYN_CHECK(out, "NULL argument");
  DMat& A = c->mats[mat_id];
  PYN_CHECK(A.mg && A.mg_valid, "multigrid: no hierarchy for the current values of matrix %d", mat_id);
  const MgHier& H = *A.mg;
  PYN_CHECK(level >= 1 && level < H.nlev, "multigrid: level %d is not a coarse level (1 .. %d)", level, H.nlev - 1);
  const MgLevel& L = H.L[level];
  const size_t cnt = (size_t)L.nn * (H.dim == 3 ? 27 : 9) * H.b * H.b;
  PYN_HIP(hipMemcpyAsync(out, L.S, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PYN_HIP(hipStreamSynchronize(c->stream));
  return PYN_OK;
}
