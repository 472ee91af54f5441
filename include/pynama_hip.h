/* pynama_hip.h -- C ABI of libpynama_hip.so: the MI355X (gfx950) implementation of the
 * Pynama finite/spectral-element hot path (element quadrature + global scatter + Krylov solve).
 *
 * Plain C: opaque context, plain pointers and sizes, int32 indices, float64 values.  No
 * PyTorch / C++ types cross this boundary.  Every function returns 0 on success and a
 * negative PYN_E* code on failure; the message is available from pyn_last_error().
 * Host arrays are caller-owned, C-contiguous, borrowed for the duration of the call.
 * Device memory is owned by the context.  A context is bound to ONE GPU and ONE process
 * (one process per GPU; ranks are tied together with pyn_comm_init over RCCL).  A context is
 * not re-entrant.
 *
 * Each entry point names the reference interface (file:line under /root/reference/) whose
 * work it takes over.  The reference has no FFI: the boundary sits behind its Python classes
 * (Spectral, DMPlexDom, Mat, KspSolver, FreeSlip); pynama_amd/ mirrors those classes on top of
 * this header with ctypes.
 */
#ifndef PYNAMA_HIP_H
#define PYNAMA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pyn_ctx pyn_ctx;

enum {
  PYN_OK = 0,
  PYN_EINVAL = -1,   /* bad argument / wrong call order */
  PYN_EHIP = -2,     /* HIP runtime error */
  PYN_ENCCL = -3,    /* RCCL error */
  PYN_ENOTCONV = -4, /* reserved */
  PYN_ENOGPU = -5    /* no gfx950 device visible */
};

/* quadrature table slots -- src/elements/spectral.py:45-61 (H/Hrs/gps, HRed/..., HOp/...) */
enum { PYN_Q_FULL = 0, PYN_Q_RED = 1, PYN_Q_NODAL = 2 };

/* scalar forms for pyn_assemble_scalar / pyn_elem_local */
enum {
  PYN_FORM_LAPLACE = 0,   /* L_e = sum_full w detJ G^T G          spectral.py:125,131 (one component) */
  PYN_FORM_MASS_NODAL = 1,/* M_e = sum_nodal w detJ H H^T         spectral.py:215 (elWeigMat)         */
  PYN_FORM_MASS_FULL = 2, /* same on the full rule (consistent mass)                                   */
  PYN_FORM_KLE = 3,       /* K_e, Rw_e, Rd_e                       spectral.py:89-157                  */
  PYN_FORM_OPERATOR = 4   /* first-order operator blocks (internal to pyn_assemble_operator)            */
};

/* Krylov method / preconditioner / norm (PETSc option names in comments) */
enum { PYN_KSP_CG = 0, PYN_KSP_GMRES = 1 };                 /* -ksp_type cg | gmres            */
enum { PYN_PC_NONE = 0, PYN_PC_JACOBI = 1, PYN_PC_MG = 2 };  /* -pc_type none | jacobi | mg     */
enum { PYN_NORM_PRECONDITIONED = 0, PYN_NORM_UNPRECONDITIONED = 1, PYN_NORM_NATURAL = 2 };
/* converged reasons, numbered as PETSc's KSPConvergedReason */
enum { PYN_CONVERGED_RTOL = 2, PYN_CONVERGED_ATOL = 3, PYN_CONVERGED_ITS = 4,
       PYN_DIVERGED_ITS = -3, PYN_DIVERGED_DTOL = -4, PYN_DIVERGED_BREAKDOWN = -5,
       PYN_DIVERGED_NANORINF = -9 };

const char* pyn_last_error(void);
int pyn_version(void);
const char* pyn_source_hash(void);   /* first 16 hex digits of the sha256 of the kernel sources this library was built from */
int pyn_device_count(int* count);
/* device and pinned-host allocations the library holds right now, in this process: their count and their bytes (either pointer may be
 * NULL).  Needs no device and no context; equal readings before a context is created and after it is destroyed mean nothing leaked. */
int pyn_alloc_live(int64_t* buffers, int64_t* bytes);

/* ---- context -------------------------------------------------------------------------- */
int pyn_ctx_create(int device, pyn_ctx** out);
int pyn_ctx_destroy(pyn_ctx* ctx);
int pyn_sync(pyn_ctx* ctx);                       /* hipStreamSynchronize on the context stream */

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ------------------------------------
 * Replaces the MPI communicator the reference hands to PETSc (src/cases/base_problem.py:22,
 * src/matrices/mat_generator.py:95-99) and the implicit collectives inside MatAssembly /
 * KSPSolve. */
int pyn_comm_unique_id(void* out, int nbytes);    /* rank 0: nbytes >= 128 */
/* unique_id == NULL with nranks > 1 declares the ranks WITHOUT a transport ("detached"): the rank's
 * slab can be assembled and multiplied in isolation, ghost entries being supplied by the caller
 * through pyn_vec_set_local_host; collectives and pyn_solve are refused.
 * nranks == 1: unique_id == NULL means serial (no communicator, no RCCL calls); a unique id creates a
 * real one-rank RCCL communicator, so the collective code paths (and a halo plan whose neighbour is
 * the rank itself) run exactly as they do at nranks > 1. */
int pyn_comm_init(pyn_ctx* ctx, int rank, int nranks, const void* unique_id, int nbytes);
/* TEST transport: the same collectives staged through a POSIX shared-memory file (device -> host, process barrier,
 * host -> device), so that world_size > 1 can be exercised end to end by processes sharing ONE GPU, which RCCL refuses
 * (duplicate device).  `path` names a zero-filled file of at least 4096 + nranks*512 + nranks*nranks*16 + nranks*cap_bytes
 * bytes created by the launcher; cap_bytes bounds one rank's packed halo.  Never used by bench.py or the cases. */
int pyn_comm_init_shm(pyn_ctx* ctx, int rank, int nranks, const char* path, int64_t cap_bytes);
int pyn_comm_barrier(pyn_ctx* ctx);               /* device + host barrier over all ranks */
int pyn_comm_allreduce_f64(pyn_ctx* ctx, double* inout, int n, int op /*0 sum, 1 max*/);
/* Start-up self-test of the communicators (all-reduces and halo exchanges have one each): RCCL's own rank count of both, all-reduce
 * of 1 and of the rank, one halo exchange of a rank-stamped vector on the main stream, one on the communication stream (the
 * overlapped form of the CG), and one on the communication stream WHILE an all-reduce is queued on the main stream, each checked on
 * the receiver.  info[6]: ranks counted by RCCL (0: the shared-memory test transport), sum(1), sum(rank), ghosts checked (main /
 * communication stream), sum(rank + 1) of the all-reduce that ran beside an exchange, [6] 1 = the halo exchanges have a communicator of
 * their own, 2 = they share the all-reduces' (RCCL refused the split; reported on stderr).  The
 * reference's analogue is implicit: PETSc checks its communicator at KSPSetUp / MatAssemblyEnd (src/solver/ksp_solver.py:19,
 * src/matrices/mat_generator.py:14-17).  Call after pyn_halo_set. */
int pyn_comm_selftest(pyn_ctx* ctx, double* info, int ninfo);

/* Row partition + halo plan of this rank.  Local node numbering: owned nodes
 * [0, n_owned) in global order, then ghosts grouped by owning neighbour (recv order).
 *   send_idx[send_ptr[k] .. send_ptr[k+1]) : owned local node ids sent to neigh[k]
 *   ghosts from neigh[k] occupy local ids n_owned + recv_ptr[k] .. n_owned + recv_ptr[k+1]
 * Must be called BEFORE pyn_mesh_set when nranks > 1 (default: everything owned). */
int pyn_halo_set(pyn_ctx* ctx, int64_t n_owned, int64_t n_ghost, int n_neigh, const int32_t* neigh,
                 const int64_t* send_ptr, const int32_t* send_idx, const int64_t* recv_ptr);

/* ---- mesh, element tables, boundary condition ------------------------------------------- */
/* Connectivity + coordinates of the LOCAL mesh (owned + ghost nodes).  Takes over
 * DMPlexDom.getCellCornersCoords (src/domain/dmplex.py:97-104) and getGlobalNodesFromCell
 * (dmplex.py:197-200 -> src/domain/indices.py:66-88) for every cell at once:
 * conn[e*nn + a] = local node id of element-local node a (reference order; the
 * first 2^dim entries are the corners in DMPlex closure order), xyz[n*dim + d].
 * nn == dim + 1 selects linear simplices (triangles / tetrahedra; no counterpart in the reference, which
 * is tensor-product only -- BASELINE.json configs[4]): the geometry nodes are the element's own nodes,
 * HrsCoo has dim+1 columns, and every entry point below works unchanged. */
int pyn_mesh_set(pyn_ctx* ctx, int dim, int nn, int64_t n_elem, int64_t n_node,
                 const int32_t* conn, const double* xyz);
/* The reference's box mesh built where it is used: replaces PETSc.DMPlex().createBoxMesh(faces, lower, upper)
 * (src/domain/dmplex.py:16-21) + the per-cell closure / coordinate interpolation of setFemIndexing / computeFullCoordinates
 * (dmplex.py:42-95) for this rank's block of a structured mesh of ngl^dim-node cells, without a host copy of either array:
 *   nel_local[dim]  elements per axis of the block (only the slowest axis -- y in 2-D, z in 3-D -- may be cut),
 *   layer0          first global element layer of the block along the slowest axis,
 *   lattice[dim]    nodes per axis of the WHOLE mesh ((ngl-1) * elements + 1),
 *   loc[nn*dim]     lattice offset in 0..ngl-1 of local node a along axis d (the reference's local order),
 *   planes[n_planes] global slowest-axis index of local plane k: local node id = k * (nodes per plane) + in-plane id, owned planes
 *                   first (pyn_halo_set's numbering); n_planes = (ngl-1) * nel_local[slow] + 1,
 *   axes            coordinate of lattice line i of axis d, the axes one after the other (lattice[0] + lattice[1] (+ lattice[2]) doubles).
 * Everything pyn_mesh_set does afterwards (topology detection, verified against the generated connectivity) is the same. */
int pyn_mesh_box(pyn_ctx* ctx, int dim, int ngl, const int64_t* nel_local, int64_t layer0, const int64_t* lattice,
                 const int32_t* loc, int64_t n_planes, const int64_t* planes, const double* axes);
/* Host copies of the local mesh as the device holds it (either pointer may be NULL): conn[n_elem*nn], xyz[n_node*dim].
 * DMPlexDom.getCellCornersCoords / getNodesCoordinates (dmplex.py:97-104, 230-244) for a caller that wants them all. */
int pyn_mesh_get(pyn_ctx* ctx, int32_t* conn, double* xyz);
/* Topology recognised by pyn_mesh_set: kind 0 = general connectivity, 1 = structured lattice of Q1
 * hexahedra (the reference's box mesh, src/domain/dmplex.py:8-21, or a rank's z-slab of one): nx, ny =
 * nodes per x / y line, nz = node planes of the local mesh.  Lattices are assembled by a plan-free kernel.
 * kind 2 = structured mesh of SECOND-order cells (ngl = 3: 9-node quadrilaterals / 27-node hexahedra in the
 * reference's local order, src/elements/spectral.py:346-431 -- the order of every yaml file under src/cases),
 * kind 3 = structured mesh of Q1 quadrilaterals; for both nx, ny, nz count the NODES per x-line, x-lines per
 * plane and planes (2-D: nz = 1) and the atomics-free row-run kernels assemble them (pyn_assemble_ho3.hip). */
int pyn_mesh_topology(pyn_ctx* ctx, int* kind, int* nx, int* ny, int* nz);
/* Box meshes of order ngl >= 4 (the reference's box mesh, (ngl-1) nelem + 1 nodes per axis numbered lexicographically, or a rank's
 * slab of one) stay kind 0 above: the assemblies and the direct solves treat them as general meshes.  They are recognised all the
 * same (every entry of the connectivity is checked) for the matrix-free KLE operator and for multigrid; this query reports it: *ngl = the order
 * (0: not such a lattice, or an order above pyn_ho_matfree_max_ngl(dim)), nx, ny, nz as for kind 2. */
int pyn_mesh_ho_lattice(pyn_ctx* ctx, int* ngl, int* nx, int* ny, int* nz);
/* Host-side pieces of that operator (no device needed).  pyn_ho_matfree_max_ngl: the largest order with a kernel (2-D: 12, 3-D: 8).
 * pyn_ho_tables_1d: the 1-D tables of order ngl, recomputed by the library (any pointer may be NULL): xl, wl [ngl] Lobatto nodes and
 * weights; Dl [ngl][ngl], Dl[i][a] = h_a'(xl_i); xr, wr [ngl-1] Gauss points and weights; Br, Gr [ngl-1][ngl] values and derivatives
 * of the ngl Lagrange functions at the Gauss points.  pyn_ho_local_lattice: loc [ngl^dim][dim], the lattice offset of every local
 * node of a box-mesh cell in the reference's vertex / edge / face / interior order (2-D: with the x ~ -r, y ~ -s flip). */
int pyn_ho_matfree_max_ngl(int dim);
int pyn_ho_tables_1d(int ngl, double* xl, double* wl, double* Dl, double* xr, double* wr, double* Br, double* Gr);
int pyn_ho_local_lattice(int ngl, int dim, int32_t* loc);
/* One quadrature's tables -- Spectral.computeMats2D/3D output (spectral.py:220-344):
 * w[ngp], H[ngp*nn], Hrs[ngp*dim*nn], HrsCoo[ngp*dim*2^dim] (geometry basis, spectral.py:54-61). */
int pyn_elem_tables_set(pyn_ctx* ctx, int which, int ngp, const double* w, const double* H,
                        const double* Hrs, const double* HrsCoo);
/* Dirichlet mask per LOCAL velocity DOF (node*ndof + d): 1 = value imposed.  Takes over the
 * set algebra of FreeSlip.buildKLEMats (src/cases/base_problem.py:512-528).  ndof = dim for the
 * KLE forms, 1 for scalar forms.  mask == NULL clears it. */
int pyn_bc_set(pyn_ctx* ctx, int ndof, const uint8_t* mask);

/* ---- symbolic phase ----------------------------------------------------------------------
 * Node adjacency graph -> CSR row pointers / column indices on the device (rows = owned
 * nodes, columns = local node ids, sorted).  Takes over DMPlexDom.getMatIndices
 * (dmplex.py:305-333) and the nnz preallocation of Mat.createEmptyKLEMats
 * (src/matrices/mat_generator.py:32-99).  All matrices share this one graph; a matrix with
 * block shape (br, bc) stores, for node-row i and component p, the scalar row
 * [(i,p) ; (col_k, q)] contiguously:  val[(rowptr[i]*br + p*len_i + k)*bc + q]. */
int pyn_csr_symbolic(pyn_ctx* ctx);
int pyn_csr_info(pyn_ctx* ctx, int64_t* n_rows, int64_t* nnz_blocks);
int pyn_csr_get(pyn_ctx* ctx, int32_t* rowptr, int32_t* colidx);

/* Optional patch plan for the atomics-free tiled assembly (Q1 hexahedra): a partition of the owned
 * rows into patches of <= 352 rows, patch p owning patch_rows[patch_ptr[p] .. patch_ptr[p+1]).  One
 * workgroup per patch integrates every element touching its rows, accumulates in LDS and writes each
 * CSR row once (no HBM atomics, no zero fill).  Built on the device from the connectivity; call after
 * pyn_csr_symbolic.  n_patch == 0 removes the plan.  Meshes without a plan use the generic kernel. */
int pyn_patch_plan_set(pyn_ctx* ctx, int n_patch, const int32_t* patch_ptr, const int32_t* patch_rows);
/* kind 0: the plan of the scalar forms (<= 352 rows per patch); kind 1: the plan of the tiled KLE
 * assembly (3x3 blocks: <= 36 rows per patch, e.g. 4x3x3 node tiles).  Both may coexist. */
int pyn_patch_plan_set_kind(pyn_ctx* ctx, int kind, int n_patch, const int32_t* patch_ptr, const int32_t* patch_rows);
/* The plan in use (the caller's, or the automatic one an assembly built): info[4] = patches, longest patch (rows), longest
 * row of the graph (entries), (patch, element) pairs -- pairs / elements is the factor by which elements on patch borders are
 * integrated more than once (diagnostics; no counterpart in the reference). */
int pyn_patch_plan_info(pyn_ctx* ctx, int kind, int64_t* info);

/* ---- matrices and vectors (device resident) ---------------------------------------------
 * Handles are small non-negative ints.  A vector with block size b has (n_owned+n_ghost)*b
 * entries; only the owned part is meaningful to the caller. */
int pyn_mat_create(pyn_ctx* ctx, int br, int bc, int* mat_id);      /* mat_generator.py:95-99 */
/* Krhs / Krhsfs / Arhs ("imposed-column" matrices: -K_e[free, bc] and the unit diagonal of the imposed DOFs, zero elsewhere) in COMPACT
 * form: only the node rows with an imposed node in their neighbourhood are stored -- the preallocation the reference makes for Krhs
 * (src/matrices/mat_generator.py:42-58, 91: `drhs_nnz` counts the Dirichlet columns of a row).  Laid out for the Dirichlet set current
 * at creation (pyn_bc_set first); an assembly under another set lays it out again.  Valid as the Krhs / Krhsfs / Arhs argument of the
 * assemblies, in pyn_spmv (rows that are not stored are zero rows), pyn_mat_add_values (entries in stored rows), pyn_mat_zero,
 * pyn_mat_get_values (the graph's full layout is returned) and pyn_mat_destroy; not a system matrix for pyn_solve.  A matrix made by
 * pyn_mat_create serves as Krhs as well (full pattern: 11 x the memory at 128^3, every product streams it whole). */
int pyn_mat_create_rhs(pyn_ctx* ctx, int br, int bc, int* mat_id);
/* what the matrix really stores: graph blocks (x br x bc doubles) and node rows -- Mat.getInfo() / printMatsInfo (mat_generator.py:120-130) */
int pyn_mat_stored_blocks(pyn_ctx* ctx, int mat_id, int64_t* blocks, int64_t* node_rows);
int pyn_mat_destroy(pyn_ctx* ctx, int mat_id);                      /* Mat.destroy(): values, solver image and Jacobi data are released, the handle dies */
int pyn_mat_zero(pyn_ctx* ctx, int mat_id);
/* Host insertion path, Mat.setValues(rows, cols, vals, addv) (src/cases/base_problem.py:531-547, src/matrices/mat_generator.py:
 * 113-118, 157-170): scalar DOF indices (node * block + component, LOCAL numbering), vals row-major [nrows][ncols];
 * insert != 0: INSERT_VALUES.  Entries outside the node graph are an error; rows of other ranks are dropped. */
int pyn_mat_add_values(pyn_ctx* ctx, int mat_id, int nrows, const int32_t* rows, int ncols, const int32_t* cols, const double* vals,
                       int insert);
int pyn_mat_get_values(pyn_ctx* ctx, int mat_id, double* val);      /* layout above */
int pyn_mat_get_diagonal(pyn_ctx* ctx, int mat_id, int vec_id);
int pyn_mat_axpy(pyn_ctx* ctx, int y_mat, double a, int x_mat);     /* Y += a X (base_problem.py:318) */
int pyn_mat_row_scale(pyn_ctx* ctx, int mat_id, int vec_id);        /* diagonalScale(L=) mat_generator.py:176; a vector of block size 1
                                                                      * holds one factor per NODE for all of its rows (the lumped weights) */
int pyn_vec_create(pyn_ctx* ctx, int bs, int* vec_id);
int pyn_vec_destroy(pyn_ctx* ctx, int vec_id);
int pyn_vec_set_host(pyn_ctx* ctx, int vec_id, const double* src);  /* owned part, n_owned*bs */
int pyn_vec_set_local_host(pyn_ctx* ctx, int vec_id, const double* src); /* owned + ghost, (n_owned+n_ghost)*bs */
int pyn_vec_get_host(pyn_ctx* ctx, int vec_id, double* dst);
int pyn_vec_fill(pyn_ctx* ctx, int vec_id, double value);
int pyn_vec_scatter_host(pyn_ctx* ctx, int vec_id, int64_t n, const int32_t* idx, const double* vals,
                         int add);                                   /* Vec.setValues */
/* w = a*x + b*y (x,y,w may alias) ; w = x.*y ; w = 1./x ; reductions over owned entries,
 * all-reduced across ranks */
int pyn_vec_axpby(pyn_ctx* ctx, int w, double a, int x, double b, int y);
int pyn_vec_pointwise_mult(pyn_ctx* ctx, int w, int x, int y);
int pyn_vec_reciprocal(pyn_ctx* ctx, int x);
int pyn_vec_vtensv(pyn_ctx* ctx, int v, int out);   /* v (x) v, BaseProblem.computeVtensV (base_problem.py:234-252) */
int pyn_vec_dot(pyn_ctx* ctx, int x, int y, double* out);
/* A NaN entry makes every norm of this rank NaN, type 3 included (its max keeps NaN, as PETSc's NORM_INFINITY does).  Across ranks
 * the all-reduce's max decides what a NaN of ONE rank becomes: it may be dropped there. */
int pyn_vec_norm(pyn_ctx* ctx, int x, int type /*1, 2, 3=inf (PETSc NormType)*/, double* out);

/* ---- explicit Runge-Kutta (TsSolver, pynama_amd/solver/ts_solver.py; pyn_ts.hip) ------------
 * Owned entries only (n_owned*bs; ghosts untouched), on the context stream.  ids[m] are vectors of x's block size,
 * 0 <= m <= PYN_TS_MAX_STAGES. */
#define PYN_TS_MAX_STAGES 8
/* y = x + sum_j w[j] * V[ids[j]], one pass, fixed j order (PETSc VecMAXPY after VecCopy: the stage vector of TSStep_RK, and
 * the roll-back of a rejected step with w = -h b, TSRollBack_RK).  y may be x. */
int pyn_vec_maxpy(pyn_ctx* ctx, int y, int x, int m, const int* ids, const double* w);
/* x += sum_j hb[j] * K[ids[j]] in place (TSEvaluateStep_RK).  wnorm != NULL: also the weighted RMS norm of the embedded error
 * d = sum_j hd[j] * K[ids[j]], sqrt( sum_i (|d_i| / (atol + rtol max(|x_i|, |x_i + d_i|)))^2 / N ) over the UPDATED x and all
 * ranks' entries N (TSErrorWeightedNorm2 with scalar tolerances); hd may be NULL when wnorm is.  No id may be x. */
int pyn_ts_step_finish(pyn_ctx* ctx, int x, int m, const int* ids, const double* hb, const double* hd, double atol, double rtol,
                       double* wnorm);

/* ---- analytic fields and constant values on node sets (pyn_fields.hip) ------------------------
 * What the reference does per node on the host -- DMPlexDom.applyFunctionVecToVec / applyValuesToVec (src/domain/dmplex.py:
 * 262-296) with the closed-form fields of src/cases/custom_func.py (:173-310) -- as one stream-ordered launch: no host loop over
 * nodes, no host-to-device copy, no synchronise. */
/* A set of OWNED local nodes kept on the device: nodes[n] strictly increasing, each in [0, n_owned) (checked here, once; n = 0 is
 * a valid empty set, nodes may then be NULL) -- the `nodes` argument of dmplex.py's apply*ToVec helpers (dmplex.py:262-296), which
 * the reference rebuilds per call.  Sets belong to the mesh: pyn_mesh_set / pyn_mesh_box release them all, like the immersed-
 * boundary markers; a released id is never handed out again. */
int pyn_nodeset_create(pyn_ctx* ctx, int64_t n, const int32_t* nodes, int* set_id);
int pyn_nodeset_destroy(pyn_ctx* ctx, int set_id);
/* The closed-form fields of src/cases/custom_func.py: Taylor-Green 2-D (:173-193), Taylor-Green 3-D on the unit box (:196-272), the
 * sinusoidal field of the operator study (:276-310).  Every factor that does not depend on the coordinates is computed by the
 * caller and travels in params; the kernel computes the phases k x_d, one sincos per axis it needs, and multiplies left to right
 * as the Python expressions do (no exp; one rounding per operation: contraction into fused multiply-adds is off for these kernels).  With k = 2 pi, e the decay exp(...) of the field at (nu, t):
 *   field                    dim bs  params                                  value
 *   TG2D_VEL                  2  2   k, e                                    cos x sin y e ; -sin x cos y e
 *   TG2D_VORT                 2  1   k, c = -2 pi (1/Lx + 1/Ly), e           c cos x cos y e
 *   TG3D_VEL                  3  3   k, e                                    cos x sin y sin z e ; sin x cos y sin z e ; -2 sin x sin y cos z e
 *   TG3D_VORT                 3  3   k, q = 2 pi e                           -3 q sin x cos y cos z ; 3 q cos x sin y cos z ; 0
 *   TG3D_CONV                 3  3   k, a = 6 (2 pi e)^2                     -a sin y cos y sin z cos z ; a sin x cos x sin z cos z ; 0
 *   TG3D_DIFF                 3  3   k, a = 9 nu e (2 pi)^3                  a sin x cos y cos z ; -a cos x sin y cos z ; 0
 *   SEN2D_VEL                 2  2   k                                       sin(k y) ; sin(2k x)
 *   SEN2D_VORT                2  1   k                                       2k cos(2k x) - k cos(k y)
 *   SEN2D_CONV                2  1   k, c = (2 pi)^2 - (4 pi)^2              c sin(k y) sin(2k x)
 *   SEN2D_DIFF                2  1   k, nu, a = (2 pi)^3, b = (4 pi)^3       nu (a cos(k y) - b cos(2k x))
 * (x, y, z in the Taylor-Green rows are the phases k x_d; 2k is exact, so 4 pi needs no slot of its own.) */
enum {
  PYN_FIELD_TG2D_VEL = 0, PYN_FIELD_TG2D_VORT = 1,
  PYN_FIELD_TG3D_VEL = 2, PYN_FIELD_TG3D_VORT = 3, PYN_FIELD_TG3D_CONV = 4, PYN_FIELD_TG3D_DIFF = 5,
  PYN_FIELD_SEN2D_VEL = 6, PYN_FIELD_SEN2D_VORT = 7, PYN_FIELD_SEN2D_CONV = 8, PYN_FIELD_SEN2D_DIFF = 9,
  PYN_FIELD_COUNT = 10
};
#define PYN_FIELD_MAX_PARAMS 4
/* dimension, block size and parameter count of a field (host only: no context; any pointer may be NULL) */
int pyn_field_info(int field, int* dim, int* bs, int* nparams);
/* vec[node*bs + k] = field_k(xyz[node]) for every node of the set (set_id -1: every owned node); other entries, ghosts included,
 * are untouched -- DMPlexDom.applyFunctionVecToVec (dmplex.py:262-275) for a custom_func.py field.  Stream-ordered: no copy, no
 * synchronise; params travel by value in the kernel arguments.  Refused with a message, before any launch: an unknown field, a
 * field whose dimension is not the mesh's, a vector whose block size is not the field's, nparams that is not the field's, a set id
 * that is dead or was never handed out by this context. */
int pyn_field_eval(pyn_ctx* ctx, int field, const double* params, int nparams, int set_id, int vec_id);
/* vec[node*bs + k] = values[k] for the nodes of the set (-1: every owned node) and the components with dofs[k] != 0 (dofs NULL:
 * all); values[nvalues], nvalues == bs, by value in the kernel arguments -- DMPlexDom.applyValuesToVec (dmplex.py:287-296) and the
 * per-wall Vec.setValues of src/cases/cavity.py:56-75.  Stream-ordered like pyn_field_eval. */
int pyn_vec_set_nodes(pyn_ctx* ctx, int vec_id, int set_id, const double* values, int nvalues, const uint8_t* dofs);

/* ---- numeric phase (HOT LOOP 1) -----------------------------------------------------------
 * One device pass over all local elements: quadrature (spectral.py:89-157) + scatter-add with
 * Dirichlet elimination (base_problem.py:499-552) + unit diagonal on imposed DOFs
 * (mat_generator.py:113-118).  Matrices are zeroed first.  Any id may be -1 (skipped).
 *   K   [dim,dim]  += K_e[free,free]         Krhs[dim,dim] += -K_e[free,bc]
 *   Rw  [dim,dim_w]+= Rw_e[free,:]           Rd  [dim,1]   += Rd_e[free,:]
 * variant: 0 = workgroup-per-element + FP64 atomics (any mesh, any ngl), 1 = auto: the tiled atomics-free
 * kernels for Q1 hexahedra (with the caller's patch plan, else patches of consecutive rows), else 0. */
int pyn_assemble_kle(pyn_ctx* ctx, double alpha_d, double alpha_w, int K, int Krhs, int Rw, int Rd,
                     int variant);
/* No-slip / free-slip split of the same pass (NoSlipFreeSlip.buildKLEMats, src/cases/base_problem.py:
 * 329-454; MatNS, src/matrices/mat_ns.py:17-121).  pyn_bc_set(dim, cls) holds a CLASS per velocity DOF:
 * 0 free, 1 tangential DOF at a no-slip wall (free in the free-slip solve, imposed in the final one),
 * 2 imposed in both.  mat_ids[8] = K, Krhs, Rw, Rd, Kfs, Krhsfs, Rwfs, Rdfs (-1 = skipped):
 *   K[0,0] += v        Krhs[0,{1,2}] += -v       Rw[0,:], Rd[0,:]          unit diagonal on classes 1, 2
 *   Kfs[1,{0,1}] , Kfs[0,1] += v  (diag -1 on class 1)      Krhsfs[{0,1},2] += -v  (diag 1 on class 2)
 *   Rwfs[1,:], Rdfs[1,:] */
int pyn_assemble_kle_noslip(pyn_ctx* ctx, double alpha_d, double alpha_w, const int* mat_ids);
/* Scalar forms with the same elimination rule: A[1,1] += A_e[free,free], Arhs += -A_e[free,bc]. */
int pyn_assemble_scalar(pyn_ctx* ctx, int form, int A, int Arhs, int variant);
/* Single-element entry used for fixture parity: runs the SAME device element routine on one
 * element given by its corner coordinates and returns dense row-major matrices
 * (spectral.py:89-157 signature: coords -> K_e, Rw_e, Rd_e; any of the outputs may be NULL).
 * PYN_FORM_KLE: out0 = K_e[dim nn, dim nn], out1 = Rw_e[dim nn, dim_w nn], out2 = Rd_e[dim nn, nn];
 * scalar forms: out0 = A_e[nn, nn]. */
int pyn_elem_local(pyn_ctx* ctx, int form, double alpha_d, double alpha_w, const double* corners,
                   double* out0, double* out1, double* out2);

/* First-order operator blocks of Spectral.getElemKLEOperators (src/elements/spectral.py:159-218:
 * SrT, DivSrT, Curl) and their global scatter (Operators.setValues, src/matrices/mat_generator.py:
 * 157-170).  With G_g = J^-1 Hrs the physical gradients at point g of quadrature `rule`, c_g = w detJ:
 *   M[(a,p),(b,q)] = sum_g c_g H_g[a] * sum_t [row_t == p and col_t == q] coef_t * G_g[der_t][b]
 * terms[t] = (row component, column component, derivative axis); the block shape is the matrix's.
 * No Dirichlet elimination (the reference applies none to the operators). */
int pyn_assemble_operator(pyn_ctx* ctx, int rule, int nterms, const int32_t* terms, const double* coef, int mat_id);
/* single element, dense row-major out[br*nn][bc*nn] (fixture parity) */
int pyn_elem_operator_local(pyn_ctx* ctx, int rule, int br, int bc, int nterms, const int32_t* terms,
                            const double* coef, const double* corners, double* out);

/* ---- SpMV and Krylov solve (HOT LOOP 2) ---------------------------------------------------
 * y = A x with halo exchange of x over RCCL when nranks > 1 (PETSc MatMult,
 * base_problem.py:481 "Rw*vort + Krhs*vel"). */
int pyn_spmv(pyn_ctx* ctx, int mat_id, int x_vec, int y_vec);
/* Which product kernel the context launched last (pyn_spmv, the products inside pyn_solve, ...): a host-side record, for tests and
 * diagnostics (no counterpart in the reference).  info[8]:
 *   [0] family, the library's ProductKind: 0 PK_NONE none yet, 1 PK_RAW 32-lane block CSR (spmv_kernel), 2 PK_SELL sell_spmv (image,
 *       explicit columns), 3 PK_SELLP sellp_spmv (image, column dictionary), 4 PK_SELLB_X sellb_spmv with explicit columns,
 *       5 PK_SELLB_D sellb_spmv with the dictionary, 6 PK_CSRL csrl_spmv, 7 PK_CSRLB csrlb_spmv, 8 PK_BCSR bcsr_spmv
 *   [1] staging width W of PK_CSRL and PK_CSRLB; lanes per node row G of PK_BCSR; block columns BC of PK_SELLB_X / _D; else 0
 *   [2] entries per lane and trip U of PK_BCSR, else 0
 *   [3] 1 when the launch carried the fused dot x.Ax
 *   [4] grid (workgroups)
 *   [5] patterns of the column dictionary (0: none)
 *   [6] longest scalar row of the matrix's block shape (0 for PK_RAW)
 *   [7] product launches of this context so far (a product split around a halo exchange counts 2) */
int pyn_product_last(pyn_ctx* ctx, int64_t* info);
/* The rule that picks the family (host only: no context, no device) -- what the library applies whenever it resolves the product of a
 * matrix, i.e. on every pyn_spmv and once per solve.  Facts: block shape br x bc; npat patterns of the node-level column dictionary
 * (0: none); maxw longest scalar row; nnzb, n_owned of the graph; rhs_compact (pyn_mat_create_rhs); solver 1: the product will be
 * repeated (Krylov loop), 0: a one-off pyn_spmv; image 1: the matrix holds a SELL image of its current values.  Knobs, as the
 * environment variables of the same names would set them: sell_image, block_sell, no_csrlb, no_sell 0 / 1; bcsr_min_avg, bcsr_lanes,
 * bcsr_unroll negative = not set.  Out: *kind as [0] above (0: no product for this block shape), *W of PK_CSRL / PK_CSRLB, *lanes and
 * *unroll of PK_BCSR, 0 where they do not apply. */
int pyn_product_choose(int br, int bc, int npat, int maxw, int64_t nnzb, int64_t n_owned, int rhs_compact, int solver, int image,
                       int sell_image, int block_sell, int no_csrlb, int no_sell, double bcsr_min_avg, int bcsr_lanes, int bcsr_unroll,
                       int* kind, int* W, int* lanes, int* unroll);
/* Which kernel family the context's most recent numeric assembly ran (pyn_assemble_kle, pyn_assemble_kle_noslip, pyn_assemble_scalar,
 * pyn_assemble_operator): a host-side record of what was launched, for tests and diagnostics (no counterpart in the reference).
 * info[8]:
 *   [0] kind, the library's AssemblyKind: 0 AK_NONE nothing assembled yet, 1 AK_GENERIC assemble_generic_kernel and its high-order
 *       staged / MFMA variants, 2 AK_P1 assemble_p1_laplace_kernel, 3 AK_PATCH the patch-plan kernels (Q1 hex scalar, P1 tets, KLE
 *       tiled, and their affine forms), 4 AK_LATTICE assemble_q1_hex_lattice_kernel, 5 AK_MARCH assemble_q1_hex_march_kernel,
 *       6 AK_KLE_LATTICE assemble_q1_hex_kle_lattice_kernel, 7 AK_ROWRUN assemble_ho3_lattice_kernel (K, Rw, Laplacian, operators)
 *   [1] tile / shape id as PYNAMA_LATTICE_TILE (0..9), PYNAMA_MARCH_TILE (0..14), PYNAMA_KLE_LATTICE_TILE (0..4) number them (an id
 *       the table does not number: 0, its default shape; the general-geometry KLE lattice kernel has one shape, 0); rows per run
 *       of AK_ROWRUN; else 0
 *   [2] 1: the K target (A of a scalar form, M of an operator) took the closed forms of affine cells; 0: quadrature, or no K target
 *   [3] the same for the Rw target
 *   [4] AK_GENERIC: 1 64 threads per element, 2 256 threads with the point data in LDS, 3 ... in global scratch, 4 ... and the Gauss
 *       points staged through LDS, 5 the FP64 matrix cores; else 0
 *   [5] 1 when a compact Krhs / Arhs was completed through the generic kernel over the elements with an imposed node
 *   [6] 1 when 1 / diagonal was written with the rows
 *   [7] assemblies of this context so far */
int pyn_assemble_last(pyn_ctx* ctx, int64_t* info);
/* ... and, when that assembly ran the rows kernel of rectilinear Q1 lattices (AK_LATTICE, shape 0, closed form), which form of it:
 * info[2]: [0] 0: another kernel, 1: one workgroup per x-line (PYNAMA_LATTICE_ROWS_ONESHOT), 2: the persistent form;
 *          [1] the workgroups it launched */
int pyn_assemble_last_rows(pyn_ctx* ctx, int64_t* info);
/* What the geometry pre-pass of the row-run kernels (lattices of order ngl 2 in 2-D and ngl 3) found on the current mesh, and the
 * form the matrix-free KLE operator of a second-order lattice took from it.  info[3]:
 *   [0] 1: every cell is a parallelogram / parallelepiped, 0: some cell is not, -1: the pass has not run on this mesh
 *   [1] 1: ... and axis-aligned, so the kernels take the diagonal forms of J^-1 (unless PYNAMA_HO3_NO_DIAG); 0: full J^-1; -1 as [0]
 *   [2] 1 / 0: the matrix-free KLE operator set on a second-order lattice uses the diagonal / the full form; -1: none is set */
int pyn_ho3_geometry(pyn_ctx* ctx, int64_t* info);
/* The rule that picks the family (host only: no context, no device, no environment) -- what every assembly applies, once, to its
 * request, the facts of the context and the PYNAMA_* switches of the moment.  The three arrays hold plain integers in the order
 * pyn_assemble_choose_layout writes into buf ("request:a,b,..;facts:..;knobs:.."): request = form, variant, which of K / Krhs / Rw /
 * Rd are asked for, whether Krhs is compact, rule and term count of an operator; facts = mesh, tables, views and patch plans
 * (mesh_affine, lat_std_ok, ho3_affine: 1 yes, 0 no, -1 not checked); knobs = flags 0 / 1 and integers, negative = not set.
 * out[8]: [0]..[3] as pyn_assemble_last, [4] the generic sub-variant, [5] 1: a compact Krhs is left to the completion pass,
 * [6] 1: 1 / diagonal is emitted, [7] 1: the request is one PYNAMA_HO3_REQUIRE insists on AK_ROWRUN for. */
int pyn_assemble_choose(const int64_t* request, const int64_t* facts, const int64_t* knobs, int64_t* out);
int pyn_assemble_choose_layout(char* buf, int len);
/* Matrix-free operators: y = A x WITHOUT an assembled matrix (PETSc analogue: a MATSHELL).  Element matrices are recomputed
 * on the fly (Spectral.getElemKLEMatrices, spectral.py:120-153) and applied per element; needs a structured mesh, errors otherwise:
 *   Q1 hexahedra (pyn_mesh_topology == lattice)            both operators
 *   second-order lattices (lattice-ngl3), 2-D and 3-D      PYN_MATFREE_KLE only, and only when every cell is affine
 *                                                          (parallelograms / parallelepipeds; sum-factorised, pyn_matfree_ho3.hip)
 *   box lattices of order ngl >= 4 (pyn_mesh_ho_lattice)   PYN_MATFREE_KLE only, affine cells only, ngl <= 12 in 2-D and <= 8 in 3-D
 *                                                          (lane per node, two passes, pyn_matfree_ho.hip).  Refused with a message:
 *                                                          a cell that is not affine, PYN_MATFREE_LAPLACE, an order above the limit,
 *                                                          a connectivity that is not the lexicographic box lattice (imported /
 *                                                          renumbered meshes), tables that are not the Lobatto(ngl) / Gauss(ngl-1) rules
 *   ANY quadrilateral / hexahedral mesh of order ngl >= 4   PYN_MATFREE_KLE_GENERAL only: bent (bilinear / trilinear) cells, any node
 *                                                          numbering, cell order, cell orientation and vertex valence (imported Gmsh
 *                                                          meshes), ngl <= 12 in 2-D and <= 8 in 3-D, ONE rank (lane per node with the
 *                                                          Jacobian formed at every point from the cell's corners, a gather pass over
 *                                                          a node -> cell incidence list; pyn_matfree_ho_general.hip).  Refused with a
 *                                                          message: an order outside 4..limit (ngl <= 3 meshes included), several ranks
 *                                                          or ghost nodes, n_elem * nn >= 2^31, tables that are not those rules or
 *                                                          whose geometry tables are not the multilinear corner basis, a cell with
 *                                                          det J <= 0 at a point of either rule ("non-positive Jacobian")
 *   ANY quadrilateral / hexahedral mesh of order ngl 3      PYN_MATFREE_KLE_NGL3_GENERAL only: second-order lattices with bent cells and
 *                                                          imported Gmsh meshes lifted to ngl 3 (any node numbering, cell order,
 *                                                          orientation-preserving cell orientation and vertex valence), ONE rank (lane
 *                                                          per tensor position = point of the Gauss(3) full rule, both rules by
 *                                                          interpolation with the Jacobian formed at every point from the cell's
 *                                                          corners, the gather pass of the general operator;
 *                                                          pyn_matfree_ho3_general.hip).  Refused with a message: an order other than
 *                                                          ngl 3 (ngl >= 4: PYN_MATFREE_KLE_GENERAL), several ranks or ghost nodes,
 *                                                          n_elem * nn >= 2^31, tables that are not the Gauss(3) / Gauss(2) rules on the
 *                                                          Lobatto(3) nodes or whose geometry tables are not the multilinear corner
 *                                                          basis, a cell with det J <= 0 at a point of either rule ("non-positive
 *                                                          Jacobian"), PYN_PC_MG in pyn_solve (the V-cycle keeps the assembled product)
 *   PYN_MATFREE_LAPLACE  the scalar Laplacian pyn_assemble_scalar(PYN_FORM_LAPLACE) builds (1 DOF per node)
 *   PYN_MATFREE_KLE      the K of pyn_assemble_kle (dim DOFs per node: 3 on Q1 hexahedra, 2 / 3 on second- and higher-order meshes);
 *                        alpha_d / alpha_w are that call's penalty weights (1e3 / 1e2 in the reference, spectral.py:152-153)
 *   PYN_MATFREE_KLE_GENERAL  the same K; its own operator id with its own snapshot (mask, alpha_d, alpha_w): on a box lattice of
 *                        affine cells both ids may be set on one context and stay independent
 *   PYN_MATFREE_KLE_NGL3_GENERAL  the same K at order ngl 3; again an id and a snapshot of its own, next to PYN_MATFREE_KLE on a
 *                        second-order lattice of affine cells.  The backend is chosen by the id, not by the mesh
 * pyn_matfree_set defines the operator from the mesh, the element tables and a SNAPSHOT of the current Dirichlet mask
 * (imposed rows identity, imposed columns eliminated, base_problem.py:531-549): call it next to the assembly it mirrors;
 * later pyn_bc_set calls do not change it. */
enum { PYN_MATFREE_OFF = 0, PYN_MATFREE_LAPLACE = 1, PYN_MATFREE_KLE = 2, PYN_MATFREE_KLE_GENERAL = 3,
       PYN_MATFREE_KLE_NGL3_GENERAL = 4 };
int pyn_matfree_set(pyn_ctx* ctx, int op, double alpha_d, double alpha_w);
int pyn_matfree_apply(pyn_ctx* ctx, int op, int x_vec, int y_vec);
typedef struct pyn_solve_opts {
  int method;        /* PYN_KSP_*  */
  int pc;            /* PYN_PC_*   */
  int norm_type;     /* PYN_NORM_* */
  int maxit;         /* PETSc default 10000 */
  int restart;       /* GMRES(m), PETSc default 30 */
  int fixed_iters;   /* >0: run exactly this many iterations, no convergence exit (benchmarking) */
  int profile;       /* !=0: bracket every SpMV launch with HIP events (first 256 iterations) */
  int cg_variant;    /* 0 auto, 1 standard PCG, 2 single-reduction PCG (Chronopoulos-Gear; default for nranks>1) */
  int gmres_orthog;  /* 0 classical Gram-Schmidt + one refinement pass (-ksp_gmres_cgs_refinement_type refine_always),
                        1 classical without refinement (refine_never, PETSc's own default), 2 modified Gram-Schmidt
                        (-ksp_gmres_modifiedgramschmidt) */
  int matfree;       /* PYN_MATFREE_*: CG / GMRES multiply with the matrix-free operator instead of the assembled matrix, which
                        then only supplies the Jacobi diagonal and the exit check (KSPSetOperators(Amat = shell, Pmat =
                        assembled)); pyn_solve first verifies on b that both operators agree */
  double rtol, atol, dtol;   /* PETSc defaults 1e-5, 1e-50, 1e5 */
} pyn_solve_opts;
typedef struct pyn_solve_info {
  int iters;
  int reason;
  double rnorm;       /* last residual norm in the solver's norm type */
  double rnorm0;
  double true_resid;  /* ||b - A x||_2 / ||b||_2 recomputed at exit; -1 (not computed) when opts.fixed_iters > 0 */
  double solve_ms;    /* device time of the iteration loop (HIP events) */
  double spmv_ms;     /* mean device time of one SpMV launch (profile != 0), else 0 */
  int spmv_launches;  /* launches averaged in spmv_ms */
  double reduce_ms;   /* single-reduction CG with profile != 0: mean device time from the end of the product to the scalars being
                         ready (partial sums + all-reduce + scalar step), else 0 */
  double halo_ms;     /* same runs, overlapped exchange: mean device time of pack + grouped send/recv on the communication
                         stream (hidden behind the interior rows when shorter than their product), else 0 */
} pyn_solve_info;
/* Solve A x = b (x0 = 0).  Takes over KspSolver.createSolver + KSP.__call__
 * (src/solver/ksp_solver.py:9-19, call site base_problem.py:481). */
int pyn_solve(pyn_ctx* ctx, int mat_id, int b_vec, int x_vec, const pyn_solve_opts* opts,
              pyn_solve_info* info);
/* Direct solve of a SMALL system: blocked dense LU with partial pivoting, the factors cached in the matrix until its values change.
 * Stands for the reference's hard-wired `-ksp_type preonly -pc_type lu` (src/solver/ksp_solver.py:13-16, makefile:7: PETSc
 * factors at KSPSetUp, every later call is two triangular solves) at the sizes the reference's own tests use it
 * (src/tests/test_solver.py).  One rank, rows <= pyn_direct_max_rows(); info->iters = 1 and info->reason =
 * PYN_CONVERGED_ITS as PETSc reports for preonly; info->true_resid as in pyn_solve.  A zero pivot is PYN_EINVAL. */
int pyn_direct_max_rows(void);
int pyn_solve_direct(pyn_ctx* ctx, int mat_id, int b_vec, int x_vec, pyn_solve_info* info);
/* Direct solve of a BANDED system above the dense limit: LU with partial pivoting in band storage (LAPACK gbtrf / gbtrs semantics),
 * in the existing numbering (no reordering).  Stands for the same `-ksp_type preonly -pc_type lu` (src/solver/ksp_solver.py:13-16)
 * on structured meshes, whose stiffness is narrowly banded in the lattice numbering.  pyn_direct_band_info: the scalar
 * half-bandwidths kl, ku of the matrix (from the node graph: (max node distance) b + b - 1) and the bytes its factors would take;
 * nothing is allocated.  pyn_solve_direct_band: factors cached in the matrix until its values change (refactored after), then
 * permuted forward / backward banded substitution; info as pyn_solve_direct (iters = 1, PYN_CONVERGED_ITS, true_resid).  One rank,
 * no ghost nodes, br == bc, not a compact pyn_mat_create_rhs matrix; factors above max_bytes or above the free device memory, and
 * a zero pivot, are PYN_EINVAL. */
int pyn_direct_band_info(pyn_ctx* ctx, int mat_id, int64_t* kl, int64_t* ku, int64_t* bytes);
int pyn_solve_direct_band(pyn_ctx* ctx, int mat_id, int b_vec, int x_vec, int64_t max_bytes, pyn_solve_info* info);

/* Geometric multigrid preconditioner for CG (PETSc's -pc_type mg) on structured lattice meshes: pyn_solve with PYN_KSP_CG and
 * PYN_PC_MG runs PCG with one V-cycle per iteration.  One rank, no ghost nodes, pyn_mesh_topology kinds 1 (Q1 hexahedra), 2 (ngl 3,
 * 2-D / 3-D) and 3 (Q1 quadrilaterals), square blocks of 1..3 DOFs per node, not a compact pyn_mat_create_rhs matrix.  Level 0 is the
 * matrix; every coarser level halves the cells of every axis (ngl 3 -> Q1 on the same node lattice first) while all cell counts are
 * even, the level has more than coarse_max_rows rows and fewer than max_levels levels exist.  A_c = P^T A P with P the tensor-product
 * linear interpolation per component, zero in decoupled fine rows (rows whose only non-zero is the diagonal: the Dirichlet rows) and
 * in decoupled coarse columns (a coarse DOF is decoupled when its coincident fine DOF is; its row is that fine diagonal).  Smoother:
 * Chebyshev of degree smooth_degree with Jacobi scaling on [esteig_min, esteig_max] x lambda, lambda estimating lambda_max(D^-1 A)
 * from esteig_its seeded CG steps; the same polynomial before and after the coarse correction (symmetric V-cycle), decoupled rows
 * z = r / a_ii.  Coarsest level: dense LU (at most pyn_direct_max_rows() rows).  The hierarchy is cached in the matrix until its
 * values change; pyn_solve builds it with the last options (the defaults when there are none).  A zero field takes its default.
 * Box lattices of order ngl >= 4 (pyn_mesh_ho_lattice reports ngl > 0; kind 0, one rank) are accepted as well.  Their first step
 * needs no even cell count: level 1 is the Q1 lattice of the same cells, E + 1 nodes per axis, coarse node I at fine node (ngl-1) I,
 * and every later level halves as above.  P0 is, per component, the tensor product over the axes of the 1-D rule: fine node i of
 * cell e takes (1 - xi_i) / 2 of coarse node e and (1 + xi_i) / 2 of e + 1, xi the Lobatto(ngl) nodes of pyn_ho_tables_1d (a cell
 * vertex: its one coincident coarse node, weight 1), masked by the decoupled DOFs as P is.  Level 1 = P0^T A P0 in the same stencil
 * format, found through 3^dim b products with the assembled matrix per build.  With matfree = PYN_MATFREE_KLE, CG and level 0 of the
 * V-cycle multiply with the ngl >= 4 shell.  Any other kind 0 mesh is refused ("general connectivity"). */
#define PYN_MG_MAX_LEVELS 16
typedef struct pyn_mg_opts {
  int max_levels;        /* -pc_mg_levels: levels including the matrix itself (default PYN_MG_MAX_LEVELS) */
  int smooth_degree;     /* -mg_levels_ksp_max_it: Chebyshev degree (default 2) */
  int coarse_max_rows;   /* stop coarsening at this many rows (default 4096) */
  int esteig_its;        /* CG steps of the eigenvalue estimate (default 10) */
  double esteig_min, esteig_max;   /* Chebyshev interval as factors of the estimate (defaults 0.1, 1.1) */
} pyn_mg_opts;
/* builds the hierarchy (again only when the options or the matrix values changed since the last build) */
int pyn_mg_setup(pyn_ctx* ctx, int mat_id, const pyn_mg_opts* opts);
/* levels; rows[PYN_MG_MAX_LEVELS] per level; lambda[PYN_MG_MAX_LEVELS] per smoothed level (0 on the coarsest); host time of the last
 * build (ms); number of builds so far (any pointer may be NULL) */
int pyn_mg_info(pyn_ctx* ctx, int mat_id, int* nlevels, int64_t* rows, double* lambda, double* setup_ms, int* builds);
/* z = M^-1 r: one V-cycle with the assembled matrix at level 0 */
int pyn_mg_apply(pyn_ctx* ctx, int mat_id, int r_vec, int z_vec);
/* stencil of coarse level `level` (1 .. nlevels-1): [node][3^dim][b][b] doubles, nodes lexicographic (x fastest), stencil entry
 * k = sum_a (o_a + 1) 3^a for the node offset o in {-1, 0, 1}^dim (x first) */
int pyn_mg_level_get(pyn_ctx* ctx, int mat_id, int level, double* out);

/* ---- immersed boundary (pyn_ibm.hip) ---------------------------------------------------------
 * One set of Lagrangian markers per context, on a UNIFORM node lattice (structured box mesh of ngl 2 or 3, pyn_mesh_topology kind
 * 1, 2 or 3; nodes lower + i h, x fastest).  With W_kj = prod_d phi((x_jd - X_kd) / h_d): interpolation (H u)_k = sum_j W_kj u_j,
 * spreading (S q)_j = sum_k W_kj c_k q_k with c_k = dl_k / prod_d h_d, and A = H S (n x n, the same for every component).
 * Velocity vectors have block size dim; marker arrays on the host are [marker][component].  Every sum has a fixed order (no
 * atomics): repeated calls give identical bits.  Every entry but pyn_ibm_set is PYN_EINVAL before a successful pyn_ibm_set. */
/* Uploads the markers and builds, for this position, the stencils, the node-major spreading lists, A and its dense LU factors --
 * ImmersedBoundaryStatic.buildIBMMatrix (src/cases/immersed_boundary.py) with the marker loops of src/domain/immersed_body.py.
 * kernel 0: Peskin's 4-point delta (the reference's fourGrid), 1: Roma's 3-point delta (threeGrid).  X[n*dim], dl[n] (arc-length /
 * area element), lower[dim], h[dim].  Refused with a message, before any kernel touches the markers: more than one rank or ghost
 * nodes; a mesh of kind 0; nodes that are not lower + i h to 1e-12 of the box extent (checked on the device); a stencil line outside
 * 1 .. n_d - 2 on any axis (imposed boundary nodes are never altered); n = 0 or n > pyn_direct_max_rows(); non-finite X or dl.
 * A refused call leaves no marker set. */
int pyn_ibm_set(pyn_ctx* ctx, int kernel, int dim, int64_t n, const double* X, const double* dl, const double* lower, const double* h);
/* out[n*dim] = H u -- the interpolation loop of computeVelocityCorrection */
int pyn_ibm_interp(pyn_ctx* ctx, int u_vec, double* out);
/* u += S q, q[n*dim] -- the spreading loop of computeVelocityCorrection */
int pyn_ibm_spread(pyn_ctx* ctx, const double* q, int u_vec);
/* The whole of computeVelocityCorrection in one call: r = ub - H u stays on the device, A q = r per component with the cached
 * factors, u += S q; q_out[n*dim] is the only device -> host copy.  Afterwards H u = ub. */
int pyn_ibm_correct(pyn_ctx* ctx, int u_vec, const double* ub, double* q_out);
/* A[n*n] row-major (the reference's H S product, for condition numbers and tests) */
int pyn_ibm_matrix_get(pyn_ctx* ctx, double* A);
/* info[4]: markers, stencil width per axis (4 or 3), affected lattice nodes, pyn_ibm_set builds since the set was created */
int pyn_ibm_info(pyn_ctx* ctx, int64_t* info);
/* drops the marker set (pyn_mesh_set / pyn_mesh_box and pyn_ctx_destroy do the same) */
int pyn_ibm_clear(pyn_ctx* ctx);

/* ---- point probes (pyn_probe.hip) ------------------------------------------------------------
 * The finite-element interpolant of a nodal vector at arbitrary points of any quadrilateral / hexahedral mesh of order
 * ngl <= pyn_ho_matfree_max_ngl(dim), on one rank.  Several probe sets live side by side (ids as for node sets, never reused);
 * pyn_mesh_set / pyn_mesh_box end every set, and a dead id is PYN_EINVAL with a message.
 * A point's cell e and reference position xi solve x(xi) = sum_c N_c(xi) X_c over the 2^dim corners (the first 2^dim entries of the
 * connectivity row; corner c sits at reference position pyn_ho_local_lattice's unflipped table of order 2).  The sampled value is
 * sum_a phi_a(xi) u[conn[e][a]], phi_a the tensor product of the Lagrange functions of the ascending Lobatto(ngl) nodes at the
 * reference position of local node a.  No floating-point atomics: two calls on the same state give identical bits. */
/* Uploads X[n*dim] and locates every point on the device, once.  Path 0, a box lattice whose nodes are the tensor product of
 * per-axis lines bit for bit (checked on the device): binary search over the cell edges per axis, xi in closed form, a point on an
 * interior cell face goes to the lower cell.  Path 1, every other mesh: a uniform bin grid of the cells' corner bounding boxes, Newton
 * from xi = 0 on each candidate (at most 16 steps, until |d xi|_inf < 1e-13), accepted at |xi|_inf <= 1 + 1e-10 (then clipped to
 * [-1, 1]); the lowest accepting cell index wins; a cell with det J <= 0 at an iterate is skipped.  A point in no cell is not an
 * error: cell -1, NaN samples.  Refused with a message: simplices; several ranks or ghost nodes; ngl above
 * pyn_ho_matfree_max_ngl(dim); nn that is not ngl^dim; n < 1; a coordinate that is NaN or infinite. */
int pyn_probe_create(pyn_ctx* ctx, int64_t n, const double* X, int* probe_id);
/* info[5]: points, points found, path (0 rectilinear, 1 search), most Newton steps of an accepted cell, most candidates of a point */
int pyn_probe_info(pyn_ctx* ctx, int probe_id, int64_t* info);
/* cell[n] (-1: not found) and xi[n*dim] (NaN where not found); either pointer may be NULL */
int pyn_probe_get(pyn_ctx* ctx, int probe_id, int32_t* cell, double* xi);
/* out[n*bs]: all bs components of the vector at every point in one pass (bs 1 .. 6), NaN where the point was not found.  Refused:
 * a vector whose node count is not the mesh's */
int pyn_probe_sample(pyn_ctx* ctx, int probe_id, int vec_id, double* out);
int pyn_probe_destroy(pyn_ctx* ctx, int probe_id);

/* ---- mesh integrals (pyn_integrals.hip) -------------------------------------------------------
 * The moments of a nodal field over any quadrilateral / hexahedral mesh of order 2 <= ngl <= pyn_ho_matfree_max_ngl(dim), on one
 * rank, in one pass over the cells: u = a, or u = a - b when vec_b >= 0 (the difference is formed per node, with one rounding,
 * before anything else).  The field of a cell is its tensor Lagrange interpolant on the Lobatto(ngl) nodes; the geometry is the
 * multilinear image of the cell's 2^dim corners (the first 2^dim entries of the connectivity row, as for the probes), its Jacobian
 * formed at every quadrature point.
 * rule: PYN_RULE_NODAL, the Lobatto(ngl) nodes themselves (collocation: the reference's lumped nodal weights); PYN_RULE_GAUSS,
 * Gauss-Legendre with ngl + 1 points per axis: volume, value and square are exact on every multilinear cell, the gradient moments
 * on affine cells.
 * out, with bs the block size of the vector (1 .. 6) and dim_w = 1 (2-D) / 3 (3-D):
 *   volume          int 1
 *   value[bs]       int u_c
 *   square[bs]      int u_c^2
 *   grad2[bs]       int |grad u_c|^2              with_grad
 *   div2            int (div u)^2                 with_grad and bs == dim
 *   curl2[dim_w]    int (curl u)_k^2              with_grad and bs == dim; 2-D: d u_1 / dx - d u_0 / dy, 3-D: the usual three
 * n_out = pyn_integrate_len(dim, bs, with_grad) entries (0 for a dim or bs that has none).
 * No floating-point atomics: a cell's sums depend on the cell alone, a fixed number of consecutive cells is accumulated in cell
 * order into one partial, a one-workgroup kernel sums the partials in a fixed order.  The result is a function of the mesh, the
 * vectors and the source constants; PYNAMA_INTEGRATE_MAX_GRID (read at every call) caps the grid and does not change a bit of it.
 * A NaN in the field gives NaN moments (volume stays), not an error.  Refused with a message: simplices; several ranks or ghost
 * nodes; nn that is not ngl^dim; ngl above the limit; a vector whose node count is not the mesh's; vec_b of another block size; an
 * unknown rule; det J <= 0 at a quadrature point (the message names the lowest such cell).  pyn_timers_get: PYN_T_INTEGRATE. */
enum { PYN_RULE_NODAL = 0, PYN_RULE_GAUSS = 1 };
int pyn_integrate(pyn_ctx* ctx, int rule, int with_grad, int vec_a, int vec_b /* -1: none */, double* out, int* n_out);
int pyn_integrate_len(int dim, int bs, int with_grad);

/* ---- timers -------------------------------------------------------------------------------
 * Device time (HIP events on the context stream) of the last call of each phase, in ms.
 * Replaces the tic/toc log of src/run_case.py:156-162. */
enum { PYN_T_SYMBOLIC = 0, PYN_T_ASSEMBLE = 1, PYN_T_SPMV = 2, PYN_T_SOLVE = 3, PYN_T_INTEGRATE = 4, PYN_T_COUNT = 8 };
int pyn_timers_get(pyn_ctx* ctx, double* ms, int n);

#ifdef __cplusplus
}
#endif
#endif /* PYNAMA_HIP_H */
