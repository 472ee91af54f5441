// Internal declarations shared by the translation units of libpynama_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/pynama_hip.h"

void pyn_set_error(const char* fmt, ...);

#define PYN_HIP(call)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      pyn_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_));      \
      return PYN_EHIP;                                                                        \
    }                                                                                         \
  } while (0)

#define PYN_NCCL(call)                                                                        \
  do {                                                                                        \
    ncclResult_t r_ = (call);                                                                 \
    if (r_ != ncclSuccess) {                                                                  \
      pyn_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, ncclGetErrorString(r_));     \
      return PYN_ENCCL;                                                                       \
    }                                                                                         \
  } while (0)

#define PYN_CHECK(cond, ...)                                                                  \
  do {                                                                                        \
    if (!(cond)) {                                                                            \
      pyn_set_error(__VA_ARGS__);                                                             \
      return PYN_EINVAL;                                                                      \
    }                                                                                         \
  } while (0)

#define PYN_TRY(call)                                                                         \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != PYN_OK) return rc_;                                                            \
  } while (0)

// ---- device memory ownership ---------------------------------------------------------------------------------------------------
// Every device (and pinned host) allocation of the library is held by one Buf: move-only, freed by its destructor, and the only
// caller of the allocator.  Set-up routines build into local Bufs and move them into the object after the last step that can fail.
// The two process-wide counters (pyn_alloc_live) make "every buffer has an owner" an equality a test can check.
inline std::atomic<int64_t> pyn_live_buffers{0}, pyn_live_bytes{0};

template <typename T, bool PINNED = false>
class Buf {
  T* p_ = nullptr;
  size_t n_ = 0;

 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  ~Buf() { reset(); }
  hipError_t alloc(size_t n) {   // frees what it holds, then n elements (uninitialised); n == 0: empty.  Empty on failure.
    reset();
    if (n == 0) return hipSuccess;
    void* p = nullptr;
    const hipError_t e = PINNED ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    n_ = n;
    pyn_live_buffers += 1;
    pyn_live_bytes += (int64_t)(n * sizeof(T));
    return hipSuccess;
  }
  hipError_t grow(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }   // at least n elements; contents are not kept
  void reset() {
    if (!p_) return;
    (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
    pyn_live_buffers -= 1;
    pyn_live_bytes -= (int64_t)(n_ * sizeof(T));
    p_ = nullptr;
    n_ = 0;
  }
  size_t size() const { return n_; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
};
template <typename T>
using DevBuf = Buf<T, false>;
template <typename T>
using PinBuf = Buf<T, true>;   // pinned host memory

// scratch bytes of a set-up routine
struct DevTmp : DevBuf<unsigned char> {
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(get());
  }
};

// n elements of `src` (null: left uninitialised) in a fresh allocation of `dst`, stream ordered
template <typename T>
inline int dev_upload(DevBuf<T>& dst, const T* src, size_t n, hipStream_t s) {
  PYN_HIP(dst.alloc(n));
  if (n && src) PYN_HIP(hipMemcpyAsync(dst.get(), src, n * sizeof(T), hipMemcpyHostToDevice, s));
  return PYN_OK;
}

struct QuadTab {
  int ngp = 0;
  DevBuf<double> w;          // [ngp]
  DevBuf<double> H;          // [ngp][nn]
  DevBuf<double> Hrs;        // [ngp][dim][nn]
  DevBuf<double> HrsCoo;     // [ngp][dim][nc]
  // host facts about the tables (set by pyn_elem_tables_set)
  double wsum = 0.0;         // sum of the weights
  bool const_grad = false;   // Hrs and HrsCoo identical at every point and to each other (affine simplex)
};

// How one assembled matrix is multiplied: the kernel family (the codes pyn_product_last reports) and what its launches need beyond the
// matrix.  Filled by pyn_sell_ensure (pyn_sell.hip), the one place that chooses and the one reader of the product knobs.
enum ProductKind { PK_NONE = 0, PK_RAW = 1, PK_SELL = 2, PK_SELLP = 3, PK_SELLB_X = 4, PK_SELLB_D = 5, PK_CSRL = 6, PK_CSRLB = 7, PK_BCSR = 8 };
struct ProductPlan {
  ProductKind kind = PK_NONE;
  int W = 0;                  // PK_CSRL (27 / 32), PK_CSRLB (18 / 32 / 50): staging width the kernel is instantiated for
  int lg = 0, unroll = 0;     // PK_BCSR: log2(lanes per node row), entries per lane and trip
  size_t lds = 0;             // dynamic LDS bytes of a launch
  int wg_cap = -1;            // most workgroups of a persistent launch (256 per CU x workgroups per CU); -1: the kernel's occupancy
  int max_grid = INT32_MAX;   // PYNAMA_SPMV_MAX_GRID
};

// complete only in pyn_mg.hip / pyn_ibm.hip, where the deleters are defined
struct MgHier;
struct IbmState;
struct MgHierDelete { void operator()(MgHier* h) const; };
struct IbmStateDelete { void operator()(IbmState* s) const; };

struct DMat {
  int br = 0, bc = 0;
  DevBuf<double> val;     // [nnzb*br*bc], layout in pynama_hip.h
  DevBuf<double> sell_val;     // SELL-64 image of `val` (the PK_SELL* kinds); it outlives a plan: a one-off block-CSR product keeps it
  bool sell_valid = false;     // the image holds the current values
  ProductPlan plan;            // how the current values are multiplied (pyn_sell_ensure); PK_NONE: not resolved yet
  DevBuf<double> dinv;         // 1 / diagonal per scalar row (Jacobi), written by the lattice assemblies in their store
  bool dinv_valid = false;     // phase, else extracted once per matrix version (pyn_dinv_ensure)
  DevBuf<double> lu;           // dense LU factors of small systems (pyn_direct.hip), [n][n] row-major, multipliers in place
  DevBuf<int> lu_piv;          // [n] row interchanges + [1] singular-column flag + [n] the same as a gather
  int64_t lu_n = 0;            // order the two buffers were sized for
  bool lu_valid = false;
  DevBuf<double> band;         // banded LU factors (pyn_direct_band.hip): [n][2 kl + ku + 64] row-major, layout there
  DevBuf<int> band_perm;       // per panel of 64 columns: the window's row interchanges as a gather [64 + kl], + [1] singular-column flag
  int64_t band_n = 0, band_kl = 0, band_ku = 0;   // shape the two buffers were sized for
  bool band_valid = false;
  std::unique_ptr<MgHier, MgHierDelete> mg;   // geometric multigrid hierarchy (pyn_mg.hip): coarse stencils, diagonals, eigenvalue estimates, coarsest LU
  bool mg_valid = false;
  // "imposed-column" matrices (Krhs / Arhs of an assembly) are zero except in rows next to imposed nodes.  rhs_clean records for
  // which Dirichlet set (pyn_ctx::bc_stamp) the stored values are known to be exactly that matrix -- or all zero (PYN_RHS_ANY: a fresh
  // or zeroed matrix fits every set); the lattice kernels then leave the zero blocks of tiles without imposed nodes unwritten.
  int64_t rhs_clean = -2;      // PYN_RHS_UNKNOWN
  // COMPACT imposed-column matrix (pyn_mat_create_rhs): only the node rows with an imposed node in their neighbourhood (themselves
  // included) are stored -- what the reference preallocates for Krhs (src/matrices/mat_generator.py:42-58, 91: `drhs_nnz`).  Stored rows
  // keep the graph's full column list; `val` holds c_nnzb blocks.  The selection belongs to ONE Dirichlet set (c_stamp).
  bool rhs_compact = false;
  int64_t c_stamp = -1;        // pyn_ctx::bc_stamp of the selection (-1: none yet)
  int64_t c_nr = 0, c_nnzb = 0;
  DevBuf<int32_t> c_crow;      // [n_owned] first block of the node's row in `val`, -1: row not stored
  DevBuf<int32_t> c_rsel;      // [c_nr] stored node rows, ascending
  DevBuf<int32_t> c_cptr;      // [c_nr + 1] first block of every stored row
  bool live = false;
  void touch() {               // the values are about to change
    sell_valid = dinv_valid = lu_valid = band_valid = mg_valid = false;
    plan = ProductPlan();
    rhs_clean = -2;
  }
  void release_band() {
    band.reset();
    band_perm.reset();
    band_n = band_kl = band_ku = 0;
    band_valid = false;
  }
  void release_lu() {          // both direct factorisations
    lu.reset();
    lu_piv.reset();
    lu_n = 0;
    lu_valid = false;
    release_band();
  }
};

struct PatchPlan {
  bool user = false;  // set through the C ABI (not the automatic consecutive-row plan)
  DevBuf<int32_t> rowptr, rows, eptr, elem;
  DevBuf<uint4> rowslot4, kmap4;
  int npatch = 0, maxrows = 0, maxlen = 0;
  int64_t npe = 0;
};

// The one structured-topology fact of the library: the connectivity is the reference's box mesh (src/domain/dmplex.py:8-21, 42-61) of
// order ngl >= 2, or a rank's slab of one (pyn_box_detect, pyn_box_lattice.hip: guessed on the host, every entry verified on the device).
// (ngl - 1) E + 1 nodes per axis numbered lexicographically; the slowest axis (y in 2-D, z in 3-D) is cut into "planes" (x-lines in
// 2-D) of NX * NY ids whose first node ids are P[j]: id = P[c_slow] + c_y NX + c_x.  Owned rows = planes [p_own0, p_own0 + n_own)
// (ids 0 .. n_owned-1); the ghost planes of a slab have ids >= n_owned.  Cell e = ex + EX (ey + EY el) sits between planes
// (ngl - 1) el and (ngl - 1) (el + 1).  Three views admit a mesh to their kernels: Lattice, Ho3View, pyn_ctx::ho_valid.
struct BoxLattice {
  bool valid = false;
  int dim = 0, ngl = 0;
  int EX = 0, EY = 0, EL = 0;   // local cells along x, y (1 in 2-D), the slow axis
  int NX = 0, NY = 0;           // nodes per x-line; x-lines per plane (1 in 2-D)
  int npl = 0, p_own0 = 0, n_own = 0;
  DevBuf<int32_t> d_P;          // [npl]
  std::vector<int32_t> P;
  int64_t plane() const { return (int64_t)NX * NY; }
  // nodes along y and z as pyn_mesh_topology reports them (2-D: the planes are the y axis, nz = 1)
  int ny() const { return dim == 3 ? NY : npl; }
  int nz() const { return dim == 3 ? npl : 1; }
  bool slab_order() const {     // ids follow the slab numbering: owned planes, then the ghost planes below, then those above
    bool ok = true;
    for (int j = 0; j < npl && ok; ++j) ok = P[j] == (j < p_own0 ? n_own + j : (j >= p_own0 + n_own ? j : j - p_own0)) * plane();
    return ok;
  }
  bool natural() const { return p_own0 == 0 && n_own == npl && slab_order(); }   // all planes owned: id = lexicographic lattice index
};

// View of 3-D first-order boxes (pyn_assemble_lattice.hip: Q1 hexahedron tiles, matrix-free Q1 products)
struct Lattice {
  bool valid = false;
  bool std_shape = false;      // ids follow the slab numbering: owned planes, ghost planes below, ghost planes above (one rank, or a rank's slab)
  DevBuf<int32_t> d_zord;      // [npl]: count | (dz+1) codes of the z-neighbour planes sorted by node id
  int rect = -1;               // rectilinear: node (i, j, plane k) at (X[i], Y[j], Z[k]) bit for bit (-1: not checked yet)
  DevBuf<double> d_axes;       // ... its axis tables X | Y | Z, each with guard slots (lat_axis_slots, pyn_lattice.h); set iff rect == 1
  DevBuf<uint32_t> d_tilebc;   // one bit per tile of the scalar tile kernel: its node box holds an imposed node ...
  int64_t tilebc_stamp = -1;   // ... for this Dirichlet set (pyn_ctx::bc_stamp)
  int tilebc_shape = -1;       // ... and this tile shape (TX << 16 | TY << 8 | TZ)
  DevBuf<uint32_t> d_rowsmap;  // one word per owned x-line of the rows kernel's walking form: class + end flags (pyn_lattice_rows.h) ...
  int64_t rowsmap_stamp = -1;  // ... for this Dirichlet set
};

// View of orders ngl 2 and 3 (pyn_assemble_ho3.hip: row-run assembly; ngl 3, the order all of the reference's cases run,
// src/cases/*.yaml, also has the matrix-free KLE operator of pyn_matfree_ho3.hip) and what its kernels cache per mesh
struct Ho3View {
  bool valid = false;
  int affine = -1;              // every element a parallelogram / parallelepiped? (-1: not checked yet)
  int diag = 0;                 // ... and axis-aligned (J diagonal): set with `affine`
  DevBuf<double> d_geom;        // [n_elem][6 | 10]: J^-1 (row = physical axis) and det J, rewritten by every assembly
  DevBuf<uint8_t> d_nbits;      // per local node: bit p = DOF p imposed (packed copy of d_bcmask)
  int64_t nbits_stamp = -1;     // pyn_ctx::bc_stamp the packed copy belongs to
  DevBuf<uint8_t> d_runflag;    // per owned node that starts a run: does the run's node box hold an imposed DOF?
  int64_t runflag_stamp = -1;   // ... for this Dirichlet set
  int runflag_R = 0;            // ... and this run length
};

// Matrix-free KLE on second-order lattices (pyn_matfree_ho3.hip): the 1-D factors of a rule (M = sum w h h, D = sum w h' h,
// S = sum w h' h') written as B^T B, G^T B, G^T G with B, G [points][3] -- values and derivatives of the 3 nodal functions at the
// rule's points, the square root of the weight folded in -- and C with J[r] = sum_d C[r][d] E_d on an affine cell (E_d = the cell's
// edge along lattice axis d; C = the Q1 corner derivatives at a point, summed over the corners at offset 2 along d)
struct Ho3MfBasis {
  double Bf[3][3], Gf[3][3];   // full rule (Gauss 3)
  double Br[2][3], Gr[2][3];   // reduced rule (Gauss 2)
  double C[3][3];              // [reference axis][lattice axis]
  int diag = 0;                // every cell's J^-1 is diagonal (axis-aligned boxes)
};

constexpr int PYN_MATFREE_SLOTS = PYN_MATFREE_KLE_NGL3_GENERAL + 1;   // operator ids of include/pynama_hip.h
constexpr int PYN_HO_MAX_NGL_2D = 12, PYN_HO_MAX_NGL_3D = 8;   // orders the matrix-free kernels are instantiated for

struct SellShape {
  int br = 0, bc = 0, maxw = 0;
  int64_t ns = 0, total = 0;
  DevBuf<int64_t> ptr;      // [ns+1] slice offsets
  DevBuf<int> w;            // [ns] slice widths (entries per scalar row)
  DevBuf<int32_t> col;      // explicit expanded columns (only when the dictionary does not apply)
  int64_t int_begin = -1, int_end = -1;  // slices without ghost columns, when they are one contiguous range
};

struct DVec {
  int bs = 0;
  DevBuf<double> d;     // [(n_owned+n_ghost)*bs]
  bool live = false;
};

// a set of owned local nodes on the device (pyn_fields.hip): strictly increasing, range-checked when it was created
struct DNodeSet {
  DevBuf<int32_t> d;     // [n]; null when n == 0
  int64_t n = 0;
  bool live = false;
};

// a set of sample points located in the mesh (pyn_probe.hip): the cell and reference position of every point, found once at creation
struct DProbe {
  DevBuf<int32_t> cell;    // [n] cell of the point, -1: in no cell
  DevBuf<double> xi;       // [n][dim] reference position in that cell (NaN where not found)
  DevBuf<double> out;      // [n][bs] staging of pyn_probe_sample (grown on demand)
  int64_t n = 0, found = 0;
  int path = 0;            // 0 rectilinear box lattice (binary search per axis), 1 bin grid + Newton
  int max_newton = 0, max_cand = 0;
  bool live = false;
};

static_assert(!std::is_copy_constructible<DMat>::value && !std::is_copy_constructible<DVec>::value &&
                  !std::is_copy_constructible<SellShape>::value && !std::is_copy_constructible<DevBuf<double>>::value,
              "a struct that owns device memory must not be copyable");
static_assert(std::is_nothrow_move_constructible<DMat>::value && std::is_nothrow_move_constructible<DVec>::value &&
                  std::is_nothrow_move_constructible<SellShape>::value && std::is_nothrow_move_constructible<DevBuf<double>>::value,
              "std::vector must move, not copy, the owners it holds");

constexpr int64_t PYN_RHS_UNKNOWN = -2, PYN_RHS_ANY = -1;   // DMat::rhs_clean
constexpr int PYN_MAX_PARTIALS = 2048;  // grid cap of every reducing kernel

// deterministic two-stage sums (pyn_krylov.hip, pyn_ts.hip): 64-lane wave sum, then block-level sum of `acc` -> part[blockIdx.x]
// (blocks of 256 threads; a second call in the same kernel needs a __syncthreads() before it)
__device__ inline double wsum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline void block_partial(double acc, double* __restrict__ part) {
  __shared__ double sm_[4];
  acc = wsum(acc);
  if ((threadIdx.x & 63) == 0) sm_[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sm_[0] + sm_[1] + sm_[2] + sm_[3];
}

// buffers of PYN_MATFREE_KLE_GENERAL (pyn_matfree_ho_general.hip), any quadrilateral / hexahedral mesh of orders ngl >= 4; it shares
// d_ho_tab / d_ho_ye with the box-lattice operator
struct HogState {
  DevBuf<int32_t> aoft;         // [nn] local node at tensor position t (the inverse of mesh_local_lattice)
  DevBuf<int32_t> inc_ptr;      // [n_node + 1] node -> (cell, t) incidence list in CSR form ...
  DevBuf<int32_t> inc;          // ... [n_elem * nn] entries cell * nn + t, ascending within a row
};
// buffers of PYN_MATFREE_KLE_NGL3_GENERAL (pyn_matfree_ho3_general.hip), any quadrilateral / hexahedral mesh of order ngl 3
struct H3gState {
  DevBuf<double> tab;           // the 1-D tables of both rules: wf Bf Gf wr Br Gr xf xr
  DevBuf<double> ye;            // the per-cell results between the two passes [n_elem][dim][nn]
  DevBuf<int32_t> aoft, inc_ptr, inc;   // as in HogState
};

// ---- context state by lifetime -----------------------------------------------------------------------------------------------------
// Every member of the context that is DERIVED from something installed lives in one of three scopes, base structs of pyn_ctx; each
// scope is reset in exactly one place by assigning a fresh one, so a cache is dropped at the right moment by where it is declared.

// Element scope, a function of (dim, nn).  Ends when a mesh of another (dim, nn) is installed (mesh_sizes, pyn_ctx.hip).
struct CtxElement {
  QuadTab quad[3];
  bool aff_standard = false;     // the uploaded tables are those of the trilinear hexahedron in closed form
  bool aff_rw_standard = false;  // ... and so is int N_a d N_b (affine Rw path)
  bool q1_red_standard = false;    // reduced rule = the centroid, weight 8, trilinear tables (lean KLE kernel)
  bool q1_gauss_standard = false;  // ... pointwise: 2x2x2 Gauss rule, unit weights (lean general-geometry kernels)
  DevBuf<double> d_aff;     // Q1-hex affine tables: [6][36] reference matrices + [4][8] non-affine monomial signs + [3][3] S
  // reference matrices of the ngl = 3 element in tensor (lattice) order, from the uploaded tables (pyn_elem_tables_set):
  // Tf / Tr[r][s][a][b] = sum_g w Hrs_r[a] Hrs_s[b] (full / reduced rule), Uf / Ur[r][a][b] = sum_g w H[a] Hrs_r[b]
  DevBuf<double> d_ho3_tabs;
  std::vector<double> ho3_t1d_host;    // 1-D factors M, D, S of the three rules; the records are their tensor products when ho3_tens_ok
  DevBuf<double> d_ho3_t1d;
  bool ho3_tens_ok = false;
  std::vector<double> ho3_tabs_host;   // host image of the records (the three rules arrive in separate pyn_elem_tables_set calls)
  bool ho3_tabs_ok[3] = {false, false, false};   // full, reduced, nodal rule
  int ho3_tabs_nn = 0;
};

// Mesh scope, a function of the connectivity and the coordinates.  Ends when a mesh is installed (mesh_installed, pyn_ctx.hip).
struct CtxMesh {
  int mesh_affine = -1;          // every element a parallelepiped? (-1: not checked yet)
  BoxLattice box;   // structured topology, if the mesh has one, and the views of it that the kernel families admit:
  Lattice lat;      // 3-D first-order cells (pyn_assemble_lattice.hip)
  Ho3View ho3;      // ngl 2 and 3 (pyn_assemble_ho3.hip)
  bool ho_valid = false;        // 4 <= ngl <= pyn_ho_matfree_max_ngl(dim) (pyn_matfree_ho.hip); pyn_mesh_topology says kind 0 for these
  DevBuf<double> d_ho_tab;      // its matrix-free KLE operator: the 1-D tables of the order (set by pyn_matfree_set) ...
  DevBuf<double> d_ho_ye;       // ... and the per-cell results between the two passes [n_elem][dim][nn]
  HogState hog;
  H3gState h3g;
  // matrix-free operators (pyn_matfree_set), slot = PYN_MATFREE_*: the Dirichlet mask is SNAPSHOT at set time, so later
  // pyn_bc_set calls (operator assembly, other matrices) do not change the operator
  bool mf_set[PYN_MATFREE_SLOTS] = {};
  DevBuf<uint8_t> mf_mask[PYN_MATFREE_SLOTS];   // null = no imposed DOF
  double mf_alpha_d[PYN_MATFREE_SLOTS] = {}, mf_alpha_w[PYN_MATFREE_SLOTS] = {};   // penalty weights of each KLE operator's snapshot
  Ho3MfBasis mf_ho3;     // the KLE operator on a second-order lattice (pyn_matfree_ho3.hip): its 1-D point bases, set with mf_set[KLE]
  // boundary condition: [n_node * bc_ndof], so a new mesh has none until pyn_bc_set
  int bc_ndof = 0;
  DevBuf<uint8_t> d_bcmask;
  // elements with an imposed node (the only ones that feed an imposed-column matrix), per Dirichlet set
  DevBuf<int32_t> d_esel;
  int64_t n_esel = 0, esel_stamp = -1;
  // general-geometry KLE: off-diagonal element Laplacians [28][ne] between the pre-pass and the tile kernel (grown on demand)
  DevBuf<double> d_kle_lel;
  // point probes (pyn_probe.hip): the local-order table ref_local_lattice(ngl, dim) [nn][dim] ...
  DevBuf<int32_t> d_probe_loc;
  DevBuf<double> d_probe_tab;       // ... and the 1-D Lobatto nodes x[ngl] with the Lagrange denominators den[ngl], uploaded once for
  int probe_tab_ngl = 0, probe_tab_dim = 0;   // ... this order and dimension
  // mesh integrals (pyn_integrals.hip): the 1-D tables w x B G of both rules and a_of_t of this order and dimension, uploaded on first
  // use; the chunk partials (grown on demand), the result and the lowest cell with det J <= 0
  DevBuf<double> d_int_tab[2], d_int_part, d_int_out;
  DevBuf<int32_t> d_int_aoft;
  DevBuf<int> d_int_bad;
  int int_tab_ngl = 0, int_tab_dim = 0;
  std::unique_ptr<IbmState, IbmStateDelete> ibm;   // immersed-boundary marker set (pyn_ibm.hip): stencils, node-major spreading lists, A = H S and its LU
};

// Graph scope, a function of the node graph.  Ends when a mesh is installed (mesh_installed) and when pyn_csr_symbolic commits a new
// graph (pyn_symbolic.hip), which moves the new rowptr / colidx / nnzb into a fresh scope.
struct CtxGraph {
  DevBuf<int32_t> d_rowptr;
  DevBuf<int32_t> d_colidx;
  int64_t nnzb = 0;
  int lat_std_ok = -1;           // Q1 lattice: closed-form row offsets verified against this graph (-1: not checked yet)
  // patch plans of the tiled assemblies (pyn_assemble_tiled.hip): [0] scalar forms, [1] KLE (3x3 blocks)
  PatchPlan plan[2];
  bool plan_unfit[2] = {false, false};  // the automatic plan did not fit this graph
  // SELL-64 structures, one per block shape, + the node-level column-pattern dictionary (pyn_sell.hip)
  std::vector<SellShape> sell_shapes;
  DevBuf<int32_t> sell_pid;      // per-node column-pattern id (dictionary mode), else null
  DevBuf<int32_t> sell_tab;      // [npat][32] relative node offsets
  int sell_npat = 0;
  bool sell_dict_built = false;
  std::vector<DMat> mats;        // handles die with the graph: "invalid matrix handle"
};

static_assert(std::is_nothrow_move_assignable<CtxElement>::value && std::is_nothrow_move_assignable<CtxMesh>::value &&
                  std::is_nothrow_move_assignable<CtxGraph>::value && !std::is_copy_constructible<CtxElement>::value &&
                  !std::is_copy_constructible<CtxMesh>::value && !std::is_copy_constructible<CtxGraph>::value,
              "a scope is reset by move-assigning a fresh one, never by a copy");

// The context proper holds what is INSTALLED or belongs to no mesh: device, streams, communicator, halo plan, the mesh arrays and their
// sizes, handles whose ids must stay stable, scratch.  A new cache is declared in the scope whose input it is computed from
// (CtxElement / CtxMesh / CtxGraph above), never here: it is then dropped with that input, and needs no release function or reset line.
struct pyn_ctx : CtxElement, CtxMesh, CtxGraph {
  pyn_ctx() = default;
  ~pyn_ctx();   // pyn_ctx.hip: drains the streams and destroys what is not memory; the members then free themselves
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t comm_stream = nullptr;            // halo exchange overlapped with the interior SpMV rows
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_vec = nullptr, ev_halo = nullptr;  // vector ready for the exchange / ghosts have arrived
  double timers[PYN_T_COUNT] = {0};

  // communicator
  int rank = 0, nranks = 1;
  ncclComm_t comm = nullptr;            // all-reduces (main stream)
  ncclComm_t comm_halo = nullptr;       // halo exchanges (split off `comm`): either stream, never shares a communicator with an all-reduce
  struct pyn_shm_comm* shm = nullptr;   // TEST transport (pyn_comm_init_shm): host-staged exchange through POSIX shared memory, so
                                        // that several ranks can share ONE GPU (RCCL refuses that); never used by bench / product runs
  bool detached = false;  // ranks declared without a transport: ghosts are supplied by the caller
  // halo plan
  int64_t n_owned = 0, n_ghost = 0;
  std::vector<int> neigh;
  std::vector<int64_t> send_ptr, recv_ptr;
  DevBuf<int32_t> d_send_idx;
  DevBuf<double> d_send_buf;     // [n_send * max_bs]
  int64_t n_send = 0;
  bool halo_set = false;

  // mesh, as installed by pyn_mesh_set / pyn_mesh_box
  int dim = 0, nn = 0, nc = 0, ngl = 0;
  int64_t n_elem = 0, n_node = 0;
  DevBuf<int32_t> d_conn;
  DevBuf<double> d_xyz;
  int64_t bc_stamp = 0;  // bumped by every pyn_bc_set; never reset, so that no stamp stored in a cache can come round again

  int64_t prod_last[8] = {0};    // pyn_product_last: the most recent product launch (pyn_product_record)

  std::vector<DVec> vecs;           // outlive a mesh: a vector of the previous mesh is refused by its node count
  std::vector<DNodeSet> nodesets;   // ids are never reused: a released set stays dead (pyn_fields.hip)
  std::vector<DProbe> probes;       // point probes (pyn_probe.hip); ids are never reused either, and a new mesh kills every set

  // reduction / solver scratch
  DevBuf<double> d_part;       // [8][PYN_MAX_PARTIALS]
  DevBuf<double> d_scal;       // [64] device scalars
  DevBuf<int> d_flag;          // [8]  device flags (done, iters, reason ...)
  PinBuf<double> h_scal;       // pinned host mirror [64]
  PinBuf<int> h_flag;          // pinned host mirror [8]
  // CG work vectors (length n_local*bs_max), reallocated on demand
  DevBuf<double> d_work;
  std::vector<hipEvent_t> prof_ev;  // event pool for per-kernel timing
  int64_t asm_last[8] = {0};     // pyn_assemble_last: what the most recent numeric assembly launched (pyn_assemble.hip)
  int64_t asm_last_rows[2] = {0};   // pyn_assemble_last_rows: ... form and grid of the lattice rows kernel, if that is what ran
  // per-context kernel attributes (pyn_kernel_lds / pyn_kernel_occupancy): a second context on another device sets its own
  std::map<const void*, size_t> kern_lds;                      // dynamic-LDS limit this context has raised the kernel to
  std::map<std::pair<const void*, size_t>, int> kern_occ;      // workgroups per CU of (kernel, dynamic LDS)
  // element-local scratch for pyn_elem_local
  DevBuf<double> d_eloc;
};

inline int64_t n_local(const pyn_ctx* c) { return c->n_owned + c->n_ghost; }
// host-side record of a product launch for pyn_product_last (slots as documented in include/pynama_hip.h)
inline void pyn_product_record(pyn_ctx* c, ProductKind family, int p1, int p2, bool dot, int grid, int maxw) {
  int64_t* r = c->prod_last;
  r[0] = family;
  r[1] = p1;
  r[2] = p2;
  r[3] = dot ? 1 : 0;
  r[4] = grid;
  r[5] = c->sell_npat;
  r[6] = maxw;
  r[7] += 1;
}
// kind of pyn_mesh_topology: 2 second-order lattice, 3 first-order quadrilaterals (both through the row-run view), 1 first-order
// hexahedra, 0 no view that assembles (general connectivity, or order ngl >= 4)
inline int pyn_lattice_kind(const pyn_ctx* c) {
  if (c->ho3.valid && (c->box.ngl == 3 || c->box.dim == 2)) return c->box.ngl == 3 ? 2 : 3;
  return c->lat.valid ? 1 : 0;
}

// ---- cross-TU helpers ---------------------------------------------------------------------
int pyn_ensure_work(pyn_ctx* c, size_t bytes);
int pyn_halo_exchange(pyn_ctx* c, double* x, int bs);  // fills ghost part of x (stream ordered)
int pyn_halo_exchange_on(pyn_ctx* c, double* x, int bs, hipStream_t st);
int pyn_check_mat(pyn_ctx* c, int id, const char* what);
int pyn_check_vec(pyn_ctx* c, int id, const char* what);
int pyn_reduce_host(pyn_ctx* c, int nslots, int nblocks, int op, double* out);  // partials -> host, allreduced
int pyn_extract_diag_inv(pyn_ctx* c, const DMat& A, double* dinv, bool invert);
int pyn_dinv_ensure(pyn_ctx* c, DMat& A);   // A.dinv valid for the current values (one diag_kernel per matrix version at most)
// assembled products (pyn_sell.hip).  pyn_sell_ensure resolves A.plan for the current values -- solver: the product will be repeated
// (Krylov loop), not a one-off pyn_spmv -- and the launches follow a plan: y = A x over the slices [a0, a1) U [b0, b1), a1 <= b0, in ONE
// launch on stream `st` (the kernels walk the logical range with the hole [a1, b0) cut out), the fused dot partials in
// d_part[poff .. poff + grid).  No halo exchange.
int pyn_sell_ensure(pyn_ctx* c, DMat& A, bool solver = true);
int pyn_sell_spmv(pyn_ctx* c, const DMat& A, const ProductPlan& P, const double* x, double* y, bool dot, int* grid_out);
int pyn_sell_spmv_range2(pyn_ctx* c, const DMat& A, const ProductPlan& P, const double* x, double* y, bool dot, int64_t a0, int64_t a1,
                         int64_t b0, int64_t b1, int poff, int max_grid, hipStream_t st, int* grid_out);
inline const ProductPlan PYN_RAW_PLAN{PK_RAW};   // 32 lanes per scalar row from the block-CSR values: needs no pyn_sell_ensure
inline int pyn_raw_grid(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>((rows * 32 + 255) / 256, PYN_MAX_PARTIALS)); }
inline int pyn_spmv_raw(pyn_ctx* c, const DMat& A, const double* x, double* y) {
  return pyn_sell_spmv(c, A, PYN_RAW_PLAN, x, y, false, nullptr);
}
const SellShape* pyn_sell_shape(pyn_ctx* c, const DMat& A);
// compact imposed-column matrices (pyn_rhs.hip)
int pyn_rhs_ensure(pyn_ctx* c, DMat& M, bool relayout = false);   // row selection + storage (values zeroed when laid out); relayout: for the CURRENT Dirichlet set
int pyn_rhs_expand(pyn_ctx* c, const DMat& M, double* full);   // full-pattern copy of the values (zeros in the rows not stored)
int pyn_bc_elements(pyn_ctx* c);                        // c->d_esel / n_esel for the current Dirichlet set
int64_t pyn_mat_blocks(const pyn_ctx* c, const DMat& M);        // blocks stored by the matrix (graph entries, or the compact count)
// entry i of the local connectivity as the host sees it: the array handed to pyn_mesh_set, or the closed form of pyn_mesh_box
using ConnAt = std::function<int32_t(int64_t)>;
// pyn_box_lattice.hip: c->box from the connectivity; the local node offsets of the box mesh (reference position / flipped in 2-D)
int pyn_box_detect(pyn_ctx* c, const ConnAt& at);
void ref_local_lattice(int n, int dim, std::vector<int>& out);
void mesh_local_lattice(int ngl, int dim, std::vector<int>& loc);
// the three views of c->box, each next to its kernels (once per pyn_mesh_set, after pyn_box_detect)
int pyn_lattice_view(pyn_ctx* c);   // pyn_assemble_lattice.hip
bool pyn_q1_affine_tables_standard(const double* aff);
int pyn_mesh_all_affine(pyn_ctx* c, int* out);                        // pyn_assemble_tiled.hip
// collectives behind one switch: RCCL (product) or the shared-memory test transport
inline bool pyn_has_comm(const pyn_ctx* c) { return c->comm != nullptr || c->shm != nullptr; }
int pyn_allreduce_dev(pyn_ctx* c, double* dbuf, int n, int op, hipStream_t st);   // op 0 sum, 1 max; in place, device buffer
int pyn_lattice_symbolic(pyn_ctx* c, bool* done);
bool pyn_q1_mixed_tables_standard(const double* w, const double* H, const double* Hrs);
bool pyn_q1_gauss_tables_standard(const double* w, const double* H, const double* Hrs, const double* HrsCoo);   // pyn_assemble_march.hip
// second-order (ngl = 3) lattices (pyn_assemble_ho3.hip)
void pyn_ho3_view(pyn_ctx* c);
int pyn_ho3_tables(pyn_ctx* c, int which, int ngp, const double* w, const double* H, const double* Hrs);
int pyn_ho3_symbolic(pyn_ctx* c, bool* done);
int pyn_ho3_cell_facts(pyn_ctx* c, bool* affine, bool* diag, double (*hc)[8]);   // every cell affine / axis-aligned; corner derivatives
// box lattices of order ngl >= 4 (pyn_matfree_ho.hip)
void pyn_ho_view(pyn_ctx* c);
// dense LU shared by the direct solve, the coarsest multigrid level and the immersed-boundary force solve (pyn_direct.hip): piv holds 2 n + 1 ints
int pyn_dense_lu_factor(pyn_ctx* c, double* D, int* piv, int64_t n);
int pyn_dense_lu_solve(pyn_ctx* c, const double* D, const int* piv, int64_t n, const double* b, double* x, double* z);
// A matrix-free backend: the mesh family whose kernels apply the shell operators (PYN_MATFREE_*).  One static record per family, next
// to its kernels: second-order lattices (pyn_matfree_ho3.hip), meshes of order ngl >= 4 (pyn_matfree_ho.hip: box lattices of affine
// cells, and PYN_MATFREE_KLE_GENERAL on any mesh through pyn_matfree_ho_general.hip), Q1 lattices (pyn_assemble_lattice.hip).
// PYN_MATFREE_KLE_NGL3_GENERAL has a backend of its own (pyn_matfree_ho3_general.hip) that is chosen by the operator id, not by the
// mesh: a bent second-order lattice is owned by the ngl 3 backend, an imported ngl 3 mesh by none.
struct MfBackend {
  bool (*owns)(const pyn_ctx* c);
  int (*set)(pyn_ctx* c, int op);        // the checks and tables of pyn_matfree_set
  int (*bs)(const pyn_ctx* c, int op);   // DOFs per node of the operator
  int (*spmv)(pyn_ctx* c, int op, const double* x, double* y, bool dot, int* grid_out);   // dot: fused x.y partials into c->d_part
  // tiles without (zsel 1) / with (zsel 2) ghost planes, for the halo overlap; null: the backend has no interior / boundary split
  int (*part)(pyn_ctx* c, int op, const double* x, double* y, bool dot, int zsel, int part_off, int max_grid, hipStream_t st, int* grid_out);
};
const MfBackend* pyn_mf_ho3();
const MfBackend* pyn_mf_ho();
const MfBackend* pyn_mf_q1();
const MfBackend* pyn_mf_h3g();
inline const MfBackend* pyn_matfree_backend(const pyn_ctx* c) { return pyn_mf_ho3()->owns(c) ? pyn_mf_ho3() : pyn_mf_ho()->owns(c) ? pyn_mf_ho() : pyn_mf_q1(); }

// "apply A" of one solve (pyn_krylov.hip): the matrix-free shell or the matrix's product plan, resolved once by init.  No halo
// exchange; products run on c->stream.
// IF_READY reads no knob: it launches from the plan an earlier resolve stored, that resolve's grid clamp and workgroup cap included
// (the exit check of a matrix-free solve: the plan of the last pyn_spmv, else the raw product).
struct LinOp {
  enum Ensure { SOLVER, ONCE, IF_READY };   // pyn_sell_ensure for a repeated product / for a one-off pyn_spmv / not at all: the stored plan
  pyn_ctx* c = nullptr;
  DMat* A = nullptr;
  const MfBackend* mf = nullptr;   // the shell's backend (matfree != PYN_MATFREE_OFF)
  int op = PYN_MATFREE_OFF;
  const ProductPlan* plan = nullptr;   // without a shell: A's plan (IF_READY and none stored: the raw product)
  const SellShape* S = nullptr;
  int init(pyn_ctx* c, DMat& A, int matfree, Ensure e = SOLVER);
  int apply(const double* x, double* y) const;
  int apply_dot(const double* x, double* y, int* grid) const;   // + the x.y partials in c->d_part[0 .. *grid), skipped once F_DONE is up
  bool can_split() const { return mf ? mf->part != nullptr : (S && S->int_begin >= 0); }
  // apply_dot in two parts: the rows that read no ghost, then -- after c->ev_halo -- the others (partials [0, *grid) all the same)
  int apply_split(const double* x, double* y, int* grid) const;
};

// geometric multigrid (pyn_mg.hip): the hierarchy for the current values (built with the last options, or the defaults), and one
// V-cycle z = M^-1 r whose level-0 products are prod0 (the assembled product or the matrix-free shell)
int pyn_mg_ensure(pyn_ctx* c, DMat& A);
int pyn_mg_vcycle(pyn_ctx* c, DMat& A, const double* r, double* z, const LinOp& prod0);

// ---- numeric assembly: request -> knobs, facts -> plan -> launch (pyn_assemble.hip) -------------------------------------------
// Every entry point describes what it was asked for (AsmRequest), reads the environment once (asm_knobs), gathers what the choice
// depends on (asm_facts), resolves the kernel family in one pure host function (asm_choose, exported as pyn_assemble_choose) and
// launches from the plan through one switch (asm_run), which records what ran for pyn_assemble_last.
enum AssemblyKind { AK_NONE = 0, AK_GENERIC = 1, AK_P1 = 2, AK_PATCH = 3, AK_LATTICE = 4, AK_MARCH = 5, AK_KLE_LATTICE = 6, AK_ROWRUN = 7 };
constexpr int PYN_HO3_MAX_TERMS = 32;   // operator terms the row-run kernels carry in their arguments

// The PYNAMA_* switches that steer the numeric assembly, read per assembly call (tests set them between calls).  F: flag, set or
// not; I: integer with the value that stands for "not set".  The switches that act when a mesh or a graph is installed are read
// there (DESIGN.md lists both groups).
// PYN_LAT_FILL_KNOBS: the ones behind the lattice checks and argument fill, all that a matrix-free Q1 product reads (lat_fill_knobs).
#define PYN_LAT_FILL_KNOBS(F, I)                                                                                                 \
  F(no_affine, "PYNAMA_NO_AFFINE") F(no_lean, "PYNAMA_NO_LEAN") F(no_std_lattice, "PYNAMA_NO_STD_LATTICE")                       \
  I(lattice_ablate, "PYNAMA_LATTICE_ABLATE", 0)
#define PYN_ASM_KNOBS(F, I)                                                                                                      \
  PYN_LAT_FILL_KNOBS(F, I) F(no_lean_plan, "PYNAMA_NO_LEAN_PLAN") F(no_p1, "PYNAMA_NO_P1")                                       \
  F(no_p1_tiled, "PYNAMA_NO_P1_TILED") F(no_ho, "PYNAMA_NO_HO") F(no_ho_mfma, "PYNAMA_NO_HO_MFMA")                               \
  F(no_dinv, "PYNAMA_NO_ASM_DINV") F(rhs_full_write, "PYNAMA_RHS_FULL_WRITE")                                                    \
  F(no_kle_lattice, "PYNAMA_NO_KLE_LATTICE") F(no_kle_general, "PYNAMA_NO_KLE_GENERAL") F(no_march, "PYNAMA_NO_MARCH")           \
  F(no_ho3_lattice, "PYNAMA_NO_HO3_LATTICE") F(no_ho3_operator, "PYNAMA_NO_HO3_OPERATOR") F(ho3_require, "PYNAMA_HO3_REQUIRE")   \
  F(ho3_no_diag, "PYNAMA_HO3_NO_DIAG") F(ho3_no_pstd, "PYNAMA_HO3_NO_PSTD") F(march_stamps, "PYNAMA_MARCH_STAMPS")               \
  I(lattice_tile, "PYNAMA_LATTICE_TILE", -1) I(march_tile, "PYNAMA_MARCH_TILE", -1)                                             \
  I(kle_lattice_tile, "PYNAMA_KLE_LATTICE_TILE", -1) I(march_zlen, "PYNAMA_MARCH_ZLEN", -1) I(ho3_run, "PYNAMA_HO3_RUN", 0)     \
  I(ho3_wgs_per_cu, "PYNAMA_HO3_WGS_PER_CU", -1) I(ho3_grid, "PYNAMA_HO3_GRID", -1) I(kle_ablate, "PYNAMA_KLE_ABLATE", 0)       \
  I(tiled_ablate, "PYNAMA_TILED_ABLATE", 0) I(ho3_ablate, "PYNAMA_HO3_ABLATE", 0)
// PYN_ASM_LAUNCH_KNOBS: switches of a launcher that asm_choose never sees (the variant is decided inside the launcher, as AFF is), so
// they are read with the others but are no part of the exported chooser's knob array (pyn_assemble_choose_layout).
#define PYN_ASM_LAUNCH_KNOBS(F, I) F(no_lattice_axes, "PYNAMA_NO_LATTICE_AXES") F(lattice_axes_require, "PYNAMA_LATTICE_AXES_REQUIRE") \
  F(no_lattice_tilebc, "PYNAMA_NO_LATTICE_TILEBC") F(no_lattice_rows, "PYNAMA_NO_LATTICE_ROWS")                                      \
  F(lattice_rows_require, "PYNAMA_LATTICE_ROWS_REQUIRE") I(lattice_rows_lines, "PYNAMA_LATTICE_ROWS_LINES", 0)               \
  I(lattice_rows_threads, "PYNAMA_LATTICE_ROWS_THREADS", 0) F(lattice_rows_oneshot, "PYNAMA_LATTICE_ROWS_ONESHOT")                      \
  I(lattice_rows_max_grid, "PYNAMA_LATTICE_ROWS_MAX_GRID", 0) F(lattice_rows_no_classes, "PYNAMA_LATTICE_ROWS_NO_CLASSES")
struct AsmKnobs {
#define PYN_F(f, e) bool f = false;
#define PYN_I(f, e, d) int f = d;
  PYN_ASM_KNOBS(PYN_F, PYN_I)
  PYN_ASM_LAUNCH_KNOBS(PYN_F, PYN_I)
#undef PYN_F
#undef PYN_I
};
AsmKnobs asm_knobs();        // the one reader of the switches above ...
AsmKnobs lat_fill_knobs();   // ... and of the four a matrix-free Q1 product reads, per product (the rest at their defaults)

// What the choice depends on beyond the request (asm_facts fills it; the ones that cost device work only for the family that reads
// them: mesh_affine, lat_std_ok, ho3_affine stay -1 "not checked" otherwise)
#define PYN_ASM_FACTS(X)                                                                                                         \
  X(dim) X(nn) X(nc) X(ngl) X(ngp0) X(ngp1) X(ngp2) X(const_grad) X(q1_gauss_standard) X(q1_red_standard) X(aff_standard)        \
  X(aff_rw_standard) X(mesh_affine) X(lat_valid) X(lat_std_ok) X(ho3_valid) X(ho3_affine) X(ho3_tabs_nn) X(ho3_tabs_ok0)         \
  X(ho3_tabs_ok1) X(ho3_tabs_ok2) X(plan0_present) X(plan0_user) X(plan0_unfit) X(plan1_present) X(plan1_user) X(plan1_unfit)
struct AsmFacts {
#define PYN_X(f) int f = 0;
  PYN_ASM_FACTS(PYN_X)
#undef PYN_X
  // this assembly has run the row-run geometry pre-pass (asm_facts launches it once) / tried the automatic patch plan, which left none
  bool geom_done = false, plan_declined = false;
};

// What an entry point was asked for, handed by reference to the launchers, + what they report back
struct AsmRequest {
  int form = 0, variant = 1;
  double alpha_d = 0.0, alpha_w = 0.0;
  double *K = nullptr, *Krhs = nullptr, *Rw = nullptr, *Rd = nullptr;   // value targets (scalar forms: K = A, Krhs = Arhs; operators: K = M)
  const int32_t* rcrow = nullptr;   // the Krhs target is COMPACT: first block of every owned node row in it (-1: not stored), else null
  int64_t krhs_blocks = 0;          // blocks it stores
  bool rhs_clean = false;           // the Krhs target holds zeros wherever this Dirichlet set leaves zeros
  double* dinv = nullptr;           // 1 / diagonal target (the K matrix's DMat::dinv), null: not wanted
  int op_rule = 0, op_br = 0, op_bc = 0, op_nterms = 0;   // PYN_FORM_OPERATOR
  const int32_t* op_terms = nullptr;                      // host copies [nterms][3], [nterms]
  const double* op_coef = nullptr;
  // results
  bool dinv_written = false;        // a kernel filled dinv
  bool krhs_completed = false;      // the compact Krhs was left to the completion pass (generic kernel over the imposed elements)
  int generic = 0;                  // sub-variant of the last generic launch
  int rows_form = 0, rows_grid = 0; // the lattice rows kernel ran: 1 the one-shot form, 2 the walking form (a class per line); its workgroups
};

struct AsmPlan {
  AssemblyKind kind = AK_GENERIC;
  int shape = 0;        // tile / shape id as the PYNAMA_*_TILE tables number it (ids they do not number: 0, the default arm); AK_ROWRUN: rows per run
  bool k_closed = false, rw_closed = false;   // the K / Rw target takes the affine closed forms (false: quadrature, or no such target)
  bool kle_general = false;   // AK_KLE_LATTICE: the general-geometry kernel (closed form of the 2x2x2 rule), not the parallelepipeds'
  int generic = 0;      // AK_GENERIC: 1 64 threads, 2 256 threads with the points in LDS, 3 ... in global scratch, 4 staged high order, 5 MFMA
  bool krhs_pending = false;   // the family cannot address the compact Krhs: the completion pass fills it
  bool dinv = false;    // 1 / diagonal leaves with the store phase
  // rowrun_candidate: the request is one the row-run view is tried for (PYNAMA_HO3_REQUIRE); want_plan: the patch kernels' turn on a
  // graph without a plan -- the actor builds the automatic one and asks again
  bool rowrun_candidate = false, want_plan = false;
};
AsmPlan asm_choose(const AsmRequest& rq, const AsmFacts& f, const AsmKnobs& k);
int asm_facts(pyn_ctx* c, const AsmRequest& rq, const AsmKnobs& k, AsmFacts* f);
// the launchers behind the plan, each next to its kernels; called only when chosen
int pyn_assemble_ho3_lattice(pyn_ctx* c, const AsmRequest& rq, const AsmKnobs& k, const AsmPlan& P);    // AK_ROWRUN, operators included
int pyn_assemble_lattice(pyn_ctx* c, AsmRequest& rq, const AsmKnobs& k, const AsmPlan& P);              // AK_LATTICE, AK_MARCH
int pyn_assemble_lattice_march(pyn_ctx* c, const AsmKnobs& k, void* lat_args, int shape);               // pyn_assemble_march.hip
int pyn_assemble_kle_lattice(pyn_ctx* c, const AsmRequest& rq, const AsmKnobs& k, const AsmPlan& P);    // AK_KLE_LATTICE
int pyn_assemble_patch(pyn_ctx* c, const AsmRequest& rq, const AsmKnobs& k, const AsmPlan& P);          // AK_PATCH
int pyn_patch_plan_default(pyn_ctx* c, int kind);   // the automatic plan of a graph without one; leaves none where it does not apply or fit
int pyn_lattice_checks(pyn_ctx* c, const AsmKnobs& k);   // c->mesh_affine, c->lat_std_ok (once per mesh / graph)
int pyn_ho3_prepare(pyn_ctx* c);                         // geometry pre-pass of a row-run assembly (+ c->ho3.affine / diag, once per mesh)
int pyn_ho3_run_length(int dim, int ngl, bool op, int knob);   // rows per run of the row-run kernels
// per-context kernel attributes (pyn_ctx.hip): raise fn's dynamic-LDS limit unless this context already set at least `bytes` (kernels
// of one fixed size only); workgroups per CU of (fn, lds), asked once
int pyn_kernel_lds(pyn_ctx* c, const void* fn, size_t bytes);
int pyn_kernel_occupancy(pyn_ctx* c, const void* fn, int threads, size_t lds, int* per_cu);
template <typename F>
inline int pyn_kernel_lds(pyn_ctx* c, F* fn, size_t bytes) { return pyn_kernel_lds(c, reinterpret_cast<const void*>(fn), bytes); }
