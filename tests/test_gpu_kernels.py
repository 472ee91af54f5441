"""GPU parity tests (run on a real MI355X with `-m gpu`): every result of the HIP path, called
through the C ABI (pynama_amd._lib.Context == include/pynama_hip.h), is compared with the CPU
oracle (oracle/fem_oracle.py) and with the reference's golden vectors (tests/golden)."""
import os

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.util import assert_assembled, mat_to_scipy, rel_err, sp_rel_err

pytestmark = pytest.mark.gpu

FP_TOL = 2e-13      # relative, FP64 with atomics (summation order differs from numpy)


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


def tile_plan(mesh, tile=(7, 7, 7)):
    """patch plan of the product's structured domain for the same box (same node numbering)"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    dom = DMPlexDom(boxMesh={'nelem': list(mesh.nelem), 'lower': [0.0] * mesh.dim, 'upper': [1.0] * mesh.dim}, comm=Comm())
    dom.setFemIndexing(mesh.ngl)
    return dom.patchPlan(tile)


def make_ctx(lib, mesh, ngl, bc_ndof=None, bc_nodes=None):
    from pynama_amd.elements.spectral import Spectral
    ctx = lib.Context(0)
    ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
    sp = Spectral(ngl, mesh.dim)
    for t in sp.deviceTables():
        ctx.tables_set(*t)
    if bc_ndof:
        mask = np.zeros((mesh.n_node, bc_ndof), np.uint8)
        mask[bc_nodes] = 1
        ctx.bc_set(bc_ndof, mask)
    ctx.csr_symbolic()
    return ctx


# ---- element level vs the reference's golden vectors ------------------------------------------
@pytest.mark.parametrize("dim,ngl", [(2, 2), (2, 3), (2, 5), (3, 2), (3, 3)])
def test_elem_local_vs_reference_golden(lib, golden, dim, ngl):
    from pynama_amd.elements.spectral import Spectral
    g = golden["g3_elem"]
    sp = Spectral(ngl, dim)
    for case in ("unit", "reftest", "brick128", "stretched", "jitter"):
        key = f"d{dim}_n{ngl}_{case}"
        K, Rw, Rd = sp.getElemKLEMatrices(g[key + "_coords"].copy())
        assert rel_err(K, g[key + "_K"]) < FP_TOL, (case, "K")
        assert rel_err(Rw, g[key + "_Rw"]) < FP_TOL, (case, "Rw")
        assert rel_err(Rd, g[key + "_Rd"]) < FP_TOL, (case, "Rd")


@pytest.mark.parametrize("dim,ngl", [(2, 2), (3, 2), (2, 4), (3, 3)])
def test_elem_scalar_forms_vs_oracle(lib, golden, dim, ngl):
    from pynama_amd.elements.spectral import Spectral
    c = golden["g3_elem"][f"d{dim}_n2_jitter_coords"]
    sp = Spectral(ngl, dim)
    tb = fo.Tables(ngl, dim)
    assert rel_err(sp.getElemLaplace(c), fo.elem_laplace(tb, c)[0]) < FP_TOL
    assert rel_err(sp.getElemMass(c, nodal=True), fo.elem_mass(tb, c, "nodal")[0]) < FP_TOL
    assert rel_err(sp.getElemMass(c, nodal=False), fo.elem_mass(tb, c, "full")[0]) < FP_TOL


# ---- symbolic phase: bit exact ------------------------------------------------------------------
@pytest.mark.parametrize("nelem,ngl", [([5, 4], 2), ([4, 3, 5], 2), ([3, 2], 4), ([2, 2, 3], 3)])
def test_csr_symbolic_bit_exact(lib, nelem, ngl):
    dim = len(nelem)
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0] * dim, ngl)
    ctx = make_ctx(lib, mesh, ngl)
    rp, ci = ctx.csr_get()
    rp_o, ci_o = fo.node_graph(mesh)
    assert np.array_equal(rp, rp_o) and np.array_equal(ci, ci_o)
    ctx.close()


def test_csr_symbolic_permuted_elements(lib):
    """element order must not matter (irregular-indexing stress)"""
    mesh = fo.box_mesh([6, 5, 4], [0, 0, 0], [1, 1, 1], 2)
    rng = np.random.default_rng(2024)
    mesh.conn = mesh.conn[rng.permutation(mesh.n_elem)]
    ctx = make_ctx(lib, mesh, 2)
    rp, ci = ctx.csr_get()
    rp_o, ci_o = fo.node_graph(mesh)
    assert np.array_equal(rp, rp_o) and np.array_equal(ci, ci_o)
    ctx.close()


# ---- numeric phase --------------------------------------------------------------------------------
@pytest.mark.parametrize("nelem,ngl,jitter,variant", [
    ([7, 6], 2, 0.2, 0), ([6, 5, 4], 2, 0.2, 0), ([6, 5, 4], 2, 0.2, 1), ([3, 4], 3, 0.0, 0),
    ([2, 3, 2], 3, 0.0, 0), ([2, 2], 6, 0.0, 0), ([16, 16, 16], 2, 0.2, 1),
    # point data beyond the LDS: Gauss points staged in chunks; nn >= 48 takes the FP64 matrix-core kernel
    ([3, 2], 8, 0.0, 0), ([2, 2], 11, 0.0, 0), ([2, 2, 2], 4, 0.0, 0), ([2, 1, 2], 5, 0.0, 0)])
def test_assemble_kle_vs_oracle(lib, nelem, ngl, jitter, variant):
    # the launch form of the generic kernel every variant-0 row is meant to reach: 1 = 64 threads, 2 = point data in LDS, 5 = matrix cores
    form = {(2, 2): 1, (3, 2): 1, (2, 3): 2, (3, 3): 2, (2, 6): 2, (2, 8): 5, (2, 11): 5, (3, 4): 5, (3, 5): 5}[(len(nelem), ngl)]
    dim = len(nelem)
    dw = 1 if dim == 2 else 3
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0, 0.8, 1.2][:dim], ngl, jitter=jitter)
    ctx = make_ctx(lib, mesh, ngl, bc_ndof=dim, bc_nodes=mesh.boundary)
    K, Krhs, Rw, Rd = (ctx.mat_create(dim, dim), ctx.mat_create(dim, dim), ctx.mat_create(dim, dw),
                       ctx.mat_create(dim, 1))
    if variant == 1 and dim == 3 and ngl == 2:
        # tiled KLE kernels (K, Krhs, Rw without HBM atomics); Rd goes through the generic kernel
        ctx.patch_plan_set(*tile_plan(mesh, (4, 3, 3)), kind=1)
        ctx.assemble_kle(1e3, 1e2, K, Krhs, Rw, -1, variant=1)
        ctx.assemble_kle(1e3, 1e2, -1, -1, -1, Rd, variant=0)
        assert_assembled(ctx, lib.AK_GENERIC, generic=form)
    else:
        ctx.assemble_kle(1e3, 1e2, K, Krhs, Rw, Rd, variant=variant)
        assert_assembled(ctx, lib.AK_GENERIC, generic=form)
    ref = fo.assemble_kle_freeslip(mesh, fo.Tables(ngl, dim), with_rd=True)
    assert sp_rel_err(mat_to_scipy(ctx, K, dim, dim), ref["K"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Krhs, dim, dim), ref["Krhs"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Rw, dim, dw), ref["Rw"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Rd, dim, 1), ref["Rd"]) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("nelem,form,variant", [([9, 7], "laplace", 0), ([6, 5, 7], "laplace", 0),
                                                ([6, 5, 7], "laplace", 1), ([6, 5, 7], "mass", 0),
                                                ([24, 16, 8], "laplace", 1)])
def test_assemble_scalar_vs_oracle(lib, nelem, form, variant):
    dim = len(nelem)
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0] * dim, 2, jitter=0.2)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    if variant == 1 and dim == 3:
        ctx.patch_plan_set(*tile_plan(mesh))
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE if form == "laplace" else lib.FORM_MASS_NODAL, A, Arhs, variant=variant)
    ref = fo.assemble_scalar(mesh, fo.Tables(2, dim), form, dirichlet=mesh.boundary)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("tile", [(7, 7, 7), (4, 5, 3), (16, 4, 4)])
def test_assemble_tiled_tiles_and_no_bc(lib, tile):
    """tiled (atomics-free) kernel == generic kernel == oracle for several tile shapes, with and
    without Dirichlet mask, with and without the Arhs output"""
    mesh = fo.box_mesh([11, 9, 10], [0, 0, 0], [1, 1, 1], 2, jitter=0.2)
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=mesh.boundary)
    ref0 = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace")
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    ctx.patch_plan_set(*tile_plan(mesh, tile))
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs, variant=1)
    assert_assembled(ctx, lib.AK_PATCH, k_closed=0, krhs_completed=0, dinv=0)     # the user plan keeps the lattice family out
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1, variant=1)
    assert_assembled(ctx, lib.AK_PATCH)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    ctx.bc_set(1, None)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1, variant=1)
    assert_assembled(ctx, lib.AK_PATCH, count=3)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref0["A"]) < FP_TOL
    ctx.close()


def test_assemble_tiled_scattered_patches(lib):
    """patches need not be lattice tiles: random row -> patch assignment and permuted elements
    (irregular-indexing stress) still give the oracle's matrix"""
    mesh = fo.box_mesh([8, 7, 6], [0, 0, 0], [1, 1, 1], 2, jitter=0.2)
    rng = np.random.default_rng(99)
    mesh.conn = mesh.conn[rng.permutation(mesh.n_elem)]
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=mesh.boundary)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    rows = rng.permutation(mesh.n_node).astype(np.int32)
    cuts = np.sort(rng.choice(np.arange(1, mesh.n_node), size=5, replace=False))
    ptr = np.concatenate([[0], cuts, [mesh.n_node]]).astype(np.int32)
    assert np.diff(ptr).max() <= 352
    ctx.patch_plan_set(ptr, rows)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs, variant=1)
    assert_assembled(ctx, lib.AK_PATCH, k_closed=0)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("kind", ["jitter", "uniform", "nobc", "partial_bc"])
def test_assemble_kle_tiled_variants(lib, kind):
    """tiled KLE kernels: general + affine geometry, no mask, per-component masks (normal DOFs only),
    K without Krhs; scattered patches"""
    mesh = fo.box_mesh([7, 6, 5], [0, 0, 0], [1.0, 0.9, 1.1], 2, jitter=0.0 if kind == "uniform" else 0.2)
    from pynama_amd.elements.spectral import Spectral
    ctx = lib.Context(0)
    ctx.mesh_set(3, mesh.conn, mesh.xyz)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    mask = np.zeros((mesh.n_node, 3), np.uint8)
    if kind in ("jitter", "uniform"):
        mask[mesh.boundary] = 1
    elif kind == "partial_bc":                       # only the normal component on each border
        for name, (d, _) in {"back": (2, 0), "front": (2, 1), "down": (1, 0), "up": (1, 1), "right": (0, 1), "left": (0, 0)}.items():
            mask[mesh.borders[name], d] = 1
    if kind != "nobc":
        ctx.bc_set(3, mask)
    ctx.csr_symbolic()
    rng = np.random.default_rng(1)
    rows = rng.permutation(mesh.n_node).astype(np.int32)
    ptr = np.arange(0, mesh.n_node + 30, 30).astype(np.int32)
    ptr[-1] = mesh.n_node
    ctx.patch_plan_set(ptr, rows, kind=1)
    K, Krhs, Rw = ctx.mat_create(3, 3), ctx.mat_create(3, 3), ctx.mat_create(3, 3)
    ctx.assemble_kle(1e3, 1e2, K, Krhs, Rw, -1, variant=1)
    closed = 1 if kind == "uniform" else 0
    assert_assembled(ctx, lib.AK_PATCH, k_closed=closed, rw_closed=closed, krhs_completed=0)
    # oracle with the same per-DOF mask
    tb = fo.Tables(2, 3)
    Ke, Rwe, _ = fo.elem_kle_matrices(tb, mesh.corners())
    import scipy.sparse as sps
    vdof = fo.dof_indices(mesh.conn, 3)
    is_bc = mask.ravel().astype(bool)
    rfree, cbc = ~is_bc[vdof], is_bc[vdof]
    R = np.broadcast_to(vdof[:, :, None], Ke.shape)
    Cc = np.broadcast_to(vdof[:, None, :], Ke.shape)
    mff = rfree[:, :, None] & rfree[:, None, :]
    mfb = rfree[:, :, None] & cbc[:, None, :]
    n3 = mesh.n_node * 3
    ident = sps.coo_matrix((np.ones(is_bc.sum()), (np.nonzero(is_bc)[0],) * 2), shape=(n3, n3)).tocsr()
    Kref = sps.coo_matrix((Ke[mff], (R[mff], Cc[mff])), shape=(n3, n3)).tocsr() + ident
    Krref = sps.coo_matrix((-Ke[mfb], (R[mfb], Cc[mfb])), shape=(n3, n3)).tocsr() + ident
    mr = np.broadcast_to(rfree[:, :, None], Rwe.shape)
    Rwref = sps.coo_matrix((Rwe[mr], (np.broadcast_to(vdof[:, :, None], Rwe.shape)[mr],
                                      np.broadcast_to(vdof[:, None, :], Rwe.shape)[mr])), shape=(n3, n3)).tocsr()
    assert sp_rel_err(mat_to_scipy(ctx, K, 3, 3), Kref) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Krhs, 3, 3), Krref) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Rw, 3, 3), Rwref) < FP_TOL
    # generic kernel agrees too (same per-DOF routing), and K alone (no Krhs / Rw) works
    K2 = ctx.mat_create(3, 3)
    ctx.assemble_kle(1e3, 1e2, K2, -1, -1, -1, variant=1)
    assert_assembled(ctx, lib.AK_PATCH, k_closed=closed, rw_closed=0)
    assert sp_rel_err(mat_to_scipy(ctx, K2, 3, 3), Kref) < FP_TOL
    ctx.assemble_kle(1e3, 1e2, K2, -1, -1, -1, variant=0)
    assert_assembled(ctx, lib.AK_GENERIC, generic=1)
    assert sp_rel_err(mat_to_scipy(ctx, K2, 3, 3), Kref) < FP_TOL
    ctx.close()


def test_assemble_empty_bc_and_idempotent(lib):
    """no Dirichlet mask -> pure scatter; assembling twice gives the same matrix (zeroed first)"""
    mesh = fo.box_mesh([5, 4, 3], [0, 0, 0], [1, 1, 1], 2)
    ctx = make_ctx(lib, mesh, 2)
    A = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    v1 = ctx.mat_values(A, 1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    v2 = ctx.mat_values(A, 1, 1)
    assert rel_err(v1, v2) < 1e-14
    S = mat_to_scipy(ctx, A, 1, 1)
    assert abs(S @ np.ones(mesh.n_node)).max() < 1e-12      # Laplacian kills constants
    ctx.close()


# ---- SpMV / vectors ----------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_spmv_and_vec_ops(lib, dim):
    dw = 1 if dim == 2 else 3
    nelem = [9, 8, 7][:dim]
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0] * dim, 2, jitter=0.1)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=dim, bc_nodes=mesh.boundary)
    K, Rw = ctx.mat_create(dim, dim), ctx.mat_create(dim, dw)
    ctx.assemble_kle(1e3, 1e2, K, -1, Rw, -1)
    rng = np.random.default_rng(7)
    xv, xw = rng.standard_normal(mesh.n_node * dim), rng.standard_normal(mesh.n_node * dw)
    vx, vw, vy = ctx.vec_create(dim), ctx.vec_create(dw), ctx.vec_create(dim)
    ctx.vec_set(vx, xv)
    ctx.vec_set(vw, xw)
    ctx.spmv(K, vx, vy)
    assert rel_err(ctx.vec_get(vy, dim), mat_to_scipy(ctx, K, dim, dim) @ xv) < 1e-13
    ctx.spmv(Rw, vw, vy)
    assert rel_err(ctx.vec_get(vy, dim), mat_to_scipy(ctx, Rw, dim, dw) @ xw) < 1e-13
    # vector algebra
    y = ctx.vec_get(vy, dim)
    assert abs(ctx.vec_dot(vx, vy) - xv @ y) < 1e-10 * abs(xv @ y)
    assert abs(ctx.vec_norm(vx, 2) - np.linalg.norm(xv)) < 1e-12 * np.linalg.norm(xv)
    assert abs(ctx.vec_norm(vx, 1) - np.abs(xv).sum()) < 1e-12 * np.abs(xv).sum()
    assert ctx.vec_norm(vx, 3) == np.abs(xv).max()
    ctx.vec_axpby(vy, 2.0, vx, -0.5, vy)
    assert rel_err(ctx.vec_get(vy, dim), 2.0 * xv - 0.5 * y) < 1e-15
    ctx.vec_scatter(vy, [0, 5], [3.0, 4.0])
    got = ctx.vec_get(vy, dim)
    assert got[0] == 3.0 and got[5] == 4.0
    ctx.close()


# ---- Krylov ------------------------------------------------------------------------------------
def _poisson(lib, nelem, jitter=0.1):
    dim = len(nelem)
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0] * dim, 2, jitter=jitter)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    A, M = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    ctx.bc_set(1, None)
    ctx.assemble_scalar(lib.FORM_MASS_FULL, M)
    f = dim * np.pi ** 2 * np.prod(np.sin(np.pi * mesh.xyz), axis=1)
    vf, vb, vx = ctx.vec_create(1), ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vf, f)
    ctx.spmv(M, vf, vb)
    b = ctx.vec_get(vb, 1)
    b[mesh.boundary] = 0.0
    ctx.vec_set(vb, b)
    return mesh, ctx, A, vb, vx, b


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("norm", [0, 1, 2])
def test_cg_matches_oracle_iterates(lib, norm, variant):
    """variant 1 = standard PCG, 2 = single-reduction (Chronopoulos-Gear) PCG used across ranks"""
    mesh, ctx, A, vb, vx, b = _poisson(lib, [12, 10, 8])
    S = mat_to_scipy(ctx, A, 1, 1)
    info = ctx.solve(A, vb, vx, method=lib.KSP_CG, pc=lib.PC_JACOBI, rtol=1e-10, norm_type=norm, cg_variant=variant)
    x_o, it_o, hist = fo.pcg(S, b, rtol=1e-10, norm_type=norm)
    assert info.reason == 2
    assert abs(info.iters - it_o) <= 1
    x = ctx.vec_get(vx, 1)
    assert rel_err(x, x_o) < 1e-8
    assert info.true_resid < 1e-8
    assert abs(info.rnorm0 - hist[0]) < 1e-12 * hist[0]
    ctx.close()


def test_cg_poisson_exact_solution(lib):
    """manufactured solution u = prod sin(pi x): discretisation error O(h^2), residual <= 1e-10"""
    mesh, ctx, A, vb, vx, b = _poisson(lib, [24, 24, 24], jitter=0.0)
    info = ctx.solve(A, vb, vx, rtol=1e-12, norm_type=lib.NORM_UNPRECONDITIONED)
    assert info.reason == 2 and info.true_resid < 1e-10
    u = ctx.vec_get(vx, 1)
    exact = np.prod(np.sin(np.pi * mesh.xyz), axis=1)
    assert np.abs(u - exact).max() < 5e-3
    ctx.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_cg_zero_rhs_and_maxit(lib, variant):
    mesh, ctx, A, vb, vx, b = _poisson(lib, [6, 6, 6])
    ctx.vec_fill(vb, 0.0)
    info = ctx.solve(A, vb, vx, cg_variant=variant)
    assert info.iters == 0 and info.reason in (2, 3)
    assert np.all(ctx.vec_get(vx, 1) == 0.0)
    ctx.vec_set(vb, b)
    info = ctx.solve(A, vb, vx, rtol=1e-14, maxit=3, cg_variant=variant)
    assert info.iters == 3 and info.reason == -3
    x3 = ctx.vec_get(vx, 1)
    info = ctx.solve(A, vb, vx, fixed_iters=3, cg_variant=variant)
    assert info.iters == 3 and info.reason == 4
    assert info.true_resid == -1.0                          # fixed-iteration runs do not pay the exit product (pynama_hip.h)
    assert rel_err(ctx.vec_get(vx, 1), x3) < 1e-12          # same 3 iterates either way
    x_o, _, _ = fo.pcg(mat_to_scipy(ctx, A, 1, 1), b, rtol=1e-30, maxit=3)
    assert rel_err(x3, x_o) < 1e-10
    ctx.close()


@pytest.mark.parametrize("orthog", [0, 1])
@pytest.mark.parametrize("restart", [1, 3, 5, 12, 40])
def test_gmres_restart_lengths_and_limits(lib, restart, orthog):
    """restart cycles run without host round trips (rotations on the device): short cycles, cycles longer than the 32
    accumulators of the projection sweep (second chunk re-reads the vector the first one produced), limits that end in
    the middle of a cycle -- iteration counts and iterates of the oracle"""
    mesh, ctx, A, vb, vx, b = _poisson(lib, [7, 6, 5])
    S = mat_to_scipy(ctx, A, 1, 1)
    kw = dict(method=lib.KSP_GMRES, pc=lib.PC_JACOBI, restart=restart, gmres_orthog=orthog)
    x_o, it_o, _ = fo.gmres(S, b, rtol=1e-10, restart=restart, maxit=3000)
    info = ctx.solve(A, vb, vx, rtol=1e-10, maxit=3000, **kw)
    assert info.reason == 2 and abs(info.iters - it_o) <= max(1, it_o // 100)
    assert rel_err(ctx.vec_get(vx, 1), x_o) < 1e-7
    lim = restart + max(1, restart // 2)                    # ends in the middle of the second cycle
    x_l, it_l, _ = fo.gmres(S, b, rtol=1e-30, restart=restart, maxit=lim)
    info = ctx.solve(A, vb, vx, rtol=1e-30, maxit=lim, **kw)
    assert info.iters == lim and info.reason == -3
    assert rel_err(ctx.vec_get(vx, 1), x_l) < 1e-9
    info = ctx.solve(A, vb, vx, fixed_iters=lim, **kw)
    assert info.iters == lim and info.reason == 4
    assert rel_err(ctx.vec_get(vx, 1), x_l) < 1e-9
    ctx.close()


@pytest.mark.parametrize("orthog", [0, 1, 2])
def test_gmres_matches_oracle(lib, orthog):
    """0: classical Gram-Schmidt + refinement (fused, default), 1: classical without refinement (PETSc's default),
    2: modified Gram-Schmidt -- all reproduce the oracle's (modified Gram-Schmidt) iteration count and solution"""
    mesh, ctx, A, vb, vx, b = _poisson(lib, [8, 7, 6])
    S = mat_to_scipy(ctx, A, 1, 1)
    info = ctx.solve(A, vb, vx, method=lib.KSP_GMRES, pc=lib.PC_JACOBI, rtol=1e-10, restart=30, gmres_orthog=orthog)
    x_o, it_o, hist = fo.gmres(S, b, rtol=1e-10, restart=30)
    assert info.reason == 2 and abs(info.iters - it_o) <= 1
    assert rel_err(ctx.vec_get(vx, 1), x_o) < 1e-7
    ctx.close()


# ---- end-to-end: the reference's analytic assertions (src/tests/test_solver.py:20-27,52-62) ----
@pytest.mark.parametrize("nelem,ngl,tol", [([10, 10], 3, 1e-12), ([3, 3, 3], 3, 2e-13)])
def test_uniform_flow_kle(lib, nelem, ngl, tol):
    dim = len(nelem)
    dw = 1 if dim == 2 else 3
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0] * dim, ngl)
    ctx = make_ctx(lib, mesh, ngl, bc_ndof=dim, bc_nodes=mesh.boundary)
    K, Krhs, Rw = ctx.mat_create(dim, dim), ctx.mat_create(dim, dim), ctx.mat_create(dim, dw)
    ctx.assemble_kle(1e3, 1e2, K, Krhs, Rw, -1)
    cte = np.array([1.0, 0.0, 0.0][:dim])
    vel = np.zeros((mesh.n_node, dim))
    vel[mesh.boundary] = cte
    vvel, vrhs, vx = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vvel, vel.ravel())
    ctx.spmv(Krhs, vvel, vrhs)                      # vort = 0 -> rhs = Krhs * vel
    # the settings of the API-level twin (KspSolver's preonly/lu substitute, tests/test_gpu_api.py:46-49): the reference's
    # own bars -- 1e-12 (2-D, test_solver.py:20-27) and 2e-13 (3-D, :52-62) -- hold at the C ABI as well
    info = ctx.solve(K, vrhs, vx, rtol=1e-14, atol=1e-300, dtol=1e8, norm_type=lib.NORM_UNPRECONDITIONED, maxit=200000)
    err = np.linalg.norm(ctx.vec_get(vx, dim) - np.tile(cte, mesh.n_node))
    assert err < tol, (err, info.iters, info.reason)
    ctx.close()


# ---- N > 1 device logic on ONE GPU: every rank's slab processed in isolation (detached comm) -----
@pytest.mark.parametrize("size,variant", [(2, 0), (3, 1)])
def test_rank_slabs_assembly_and_spmv(lib, size, variant):
    """owner-computes assembly + SpMV of each rank's slab (owned rows, ghost columns) equals the
    corresponding rows of the serial oracle; covers local numbering, ghost handling in the generic
    and tiled kernels, the SELL image and the per-entry bc bytes."""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    nelem = [6, 5, 9]
    glob = fo.box_mesh(nelem, [0, 0, 0], [1, 1, 1], 2, jitter=0.2)
    ref = fo.assemble_scalar(glob, fo.Tables(2, 3), "laplace", dirichlet=glob.boundary)
    xg = np.random.default_rng(11).standard_normal(glob.n_node)
    yg = ref["A"] @ xg
    for r in range(size):
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0, 0, 0], 'upper': [1, 1, 1]}, comm=Comm(r, size), jitter=0.2)
        dom.setFemIndexing(2)
        ctx = lib.Context(0)
        ctx.comm_init(r, size, None)                      # detached
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(3, dom.conn, dom.xyz)
        for t in Spectral(2, 3).deviceTables():
            ctx.tables_set(*t)
        ctx.bc_set(1, dom.boundaryMaskLocal())
        ctx.csr_symbolic()
        if variant == 1:
            ctx.patch_plan_set(*dom.patchPlan((7, 7, 7)))
        A, Ar = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar, variant=variant)
        cols = dom._local2global(np.arange(dom.nLocal))
        S = mat_to_scipy(ctx, A, 1, 1)
        assert sp_rel_err(S, ref["A"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Ar, 1, 1), ref["Arhs"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        vx, vy = ctx.vec_create(1), ctx.vec_create(1)
        ctx.vec_set_local(vx, xg[cols])
        ctx.spmv(A, vx, vy)
        assert rel_err(ctx.vec_get(vy, 1), yg[dom.rStart:dom.rEnd]) < 1e-13
        with pytest.raises(lib.PynamaHipError):
            ctx.solve(A, vx, vy)
        ctx.close()


def test_random_node_numbering_falls_back_to_explicit_columns(lib):
    """irregular indexing: with randomly permuted node ids the column-pattern dictionary does not
    apply (thousands of patterns) and the SpMV/CG path uses explicit column indices; results still
    match the oracle on the permuted mesh"""
    mesh = fo.box_mesh([9, 8, 7], [0, 0, 0], [1, 1, 1], 2, jitter=0.2)
    rng = np.random.default_rng(4242)
    perm = rng.permutation(mesh.n_node)                 # old id -> new id
    inv = np.argsort(perm)
    mesh.conn = perm[mesh.conn].astype(np.int32)
    mesh.xyz = mesh.xyz[inv]
    mesh.boundary = np.sort(perm[mesh.boundary])
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    assert ctx.mesh_topology()[0] == "general"
    rp, ci = ctx.csr_get()
    rp_o, ci_o = fo.node_graph(mesh)
    assert np.array_equal(rp, rp_o) and np.array_equal(ci, ci_o)
    A = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)            # variant auto: tiled kernel on the default plan
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=mesh.boundary)
    S = mat_to_scipy(ctx, A, 1, 1)
    assert sp_rel_err(S, ref["A"]) < FP_TOL
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, variant=0)  # HBM-atomic kernel
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    b = rng.standard_normal(mesh.n_node)
    b[mesh.boundary] = 0
    vb, vx, vy = ctx.vec_create(1), ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vb, b)
    ctx.spmv(A, vb, vy)
    assert rel_err(ctx.vec_get(vy, 1), ref["A"] @ b) < 1e-13
    info = ctx.solve(A, vb, vx, rtol=1e-10, norm_type=lib.NORM_UNPRECONDITIONED)
    x_o, it_o, _ = fo.pcg(ref["A"], b, rtol=1e-10, norm_type=fo.NORM_UNPRECONDITIONED)
    assert info.reason == 2 and abs(info.iters - it_o) <= 1 and rel_err(ctx.vec_get(vx, 1), x_o) < 1e-8
    ctx.close()


@pytest.mark.parametrize("kind", ["uniform", "sheared", "mixed"])
def test_assemble_tiled_affine_shortcut(lib, kind):
    """parallelepiped elements take the affine shortcut of the tiled kernel (constant Jacobian,
    precomputed reference matrices); 'mixed' jitters only the upper half of the box so that whole-wave
    affine and general quadrature paths coexist in one launch.  All equal the oracle's 8-point rule."""
    mesh = fo.box_mesh([14, 9, 16], [0, 0, 0], [1.0, 0.7, 1.3], 2)
    if kind == "sheared":
        M = np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]])
        mesh.xyz = mesh.xyz @ M.T + np.array([0.5, -1.0, 2.0])
    if kind == "mixed":
        rng = np.random.default_rng(8)
        mv = 0.15 * (1.0 / 16) * rng.uniform(-1, 1, size=mesh.xyz.shape)
        mv[mesh.xyz[:, 2] < 0.65] = 0.0
        mv[mesh.boundary] = 0.0
        mesh.xyz = mesh.xyz + mv
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=mesh.boundary)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    ctx.patch_plan_set(*tile_plan(mesh))
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs, variant=1)
    assert_assembled(ctx, lib.AK_PATCH, k_closed=0 if kind == "mixed" else 1, krhs_completed=0, dinv=0)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    ctx.close()


# ---- first-order operators (scope row f1) ------------------------------------------------------
@pytest.mark.parametrize("dim,ngl", [(2, 2), (2, 3), (2, 5), (3, 2), (3, 3)])
def test_elem_operators_vs_reference_golden(lib, golden, dim, ngl):
    """getElemKLEOperators on the GPU == the reference's own outputs (spectral.py:159-218)"""
    from pynama_amd.elements.spectral import Spectral
    g = golden["g3_elem"]
    sp = Spectral(ngl, dim)
    for case in ("unit", "reftest", "brick128", "stretched", "jitter"):
        key = f"d{dim}_n{ngl}_{case}"
        SrT, Div, Curl, wei = sp.getElemKLEOperators(g[key + "_coords"].copy())
        for name, got in (("SrT", SrT), ("DivSrT", Div), ("Curl", Curl), ("wei", wei)):
            assert rel_err(got, g[f"{key}_{name}"]) < FP_TOL, (case, name)


@pytest.mark.parametrize("nelem,ngl", [([6, 5], 2), ([5, 4, 3], 2), ([3, 2], 3)])
def test_operators_global_vs_oracle(lib, nelem, ngl):
    from pynama_amd.elements.spectral import Spectral
    dim = len(nelem)
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0, 0.8, 1.2][:dim], ngl, jitter=0.15 if ngl == 2 else 0.0)
    ref = fo.assemble_operators(mesh, fo.Tables(ngl, dim))
    ctx = make_ctx(lib, mesh, ngl)
    sp = Spectral(ngl, dim)
    ops = sp.operatorTerms()
    mass = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_MASS_NODAL, mass, -1, 0)
    vw = ctx.vec_create(1)
    ctx.mat_diagonal(mass, vw)
    w = ctx.vec_get(vw, 1)
    assert rel_err(w, ref["weights"]) < FP_TOL
    for name in ("SrT", "DivSrT", "Curl"):
        br, bc, terms, coef = ops[name]
        m = ctx.mat_create(br, bc)
        ctx.assemble_operator(lib.Q_NODAL, terms, coef, m)
        vs = ctx.vec_create(br)
        ctx.vec_set(vs, np.repeat(1.0 / w, br))
        ctx.mat_row_scale(m, vs)
        assert sp_rel_err(mat_to_scipy(ctx, m, br, bc), ref[name]) < FP_TOL, name
        # the same scaling from ONE factor per node (a vector of block size 1 serves all rows of the node: what Operators keeps on the device)
        m1 = ctx.mat_create(br, bc)
        ctx.assemble_operator(lib.Q_NODAL, terms, coef, m1)
        v1 = ctx.vec_create(1)
        ctx.vec_set(v1, 1.0 / w)
        ctx.mat_row_scale(m1, v1)
        assert rel_err(ctx.mat_values(m1, br, bc), ctx.mat_values(m, br, bc)) < 1e-14, name      # (two assemblies: LDS adds in any order)
        # SpMV through the block SELL image of the rectangular operator
        x = np.random.default_rng(2).standard_normal(mesh.n_node * bc)
        vx, vy = ctx.vec_create(bc), ctx.vec_create(br)
        ctx.vec_set(vx, x)
        ctx.spmv(m, vx, vy)
        assert rel_err(ctx.vec_get(vy, br), ref[name] @ x) < 1e-12, name
    ctx.close()


# ---- no-slip / free-slip split (scope row f2) --------------------------------------------------------
@pytest.mark.parametrize("nelem,ns,dr", [([6, 5], ["up", "down", "left", "right"], []),
                                         ([5, 4], ["up", "down"], ["left", "right"]),
                                         ([4, 3, 3], ["up", "down", "left", "right", "front", "back"], []),
                                         ([3, 3, 4], ["up", "left"], ["front"])])
def test_assemble_kle_noslip_vs_oracle(lib, nelem, ns, dr):
    dim = len(nelem)
    dw = 1 if dim == 2 else 3
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0, 0.8, 1.2][:dim], 2, jitter=0.15)
    cls = fo.noslip_classes(mesh, ns, dr)
    ref = fo.assemble_kle_noslip(mesh, fo.Tables(2, dim), cls)
    ctx = make_ctx(lib, mesh, 2)
    ctx.bc_set(dim, cls)
    shapes = [("K", dim, dim), ("Krhs", dim, dim), ("Rw", dim, dw), ("Rd", dim, 1),
              ("Kfs", dim, dim), ("Krhsfs", dim, dim), ("Rwfs", dim, dw), ("Rdfs", dim, 1)]
    ids = [ctx.mat_create(br, bc) for _, br, bc in shapes]
    ctx.assemble_kle_noslip(1e3, 1e2, ids)
    assert_assembled(ctx, lib.AK_GENERIC, generic=1, krhs_completed=0, dinv=0)
    for (name, br, bc), mid in zip(shapes, ids):
        assert sp_rel_err(mat_to_scipy(ctx, mid, br, bc), ref[name]) < FP_TOL, name
    # K + Kfs is the operator with only the doubly imposed DOFs eliminated (base_problem.py:318)
    Kff = (ref["K"] + ref["Kfs"]).toarray()
    assert np.abs(Kff - Kff.T).max() < 1e-9 * np.abs(Kff).max()
    ctx.close()


# ---- RCCL code paths on one GPU: a real one-rank communicator ---------------------------------
def test_rccl_one_rank_halo_exchange_and_collectives(lib):
    """The transport used at nranks > 1 (pack kernel + grouped ncclSend/ncclRecv into the ghost range,
    ncclAllReduce behind dot/norm/CG) exercised on one GPU: the rank is its own neighbour, its ghosts
    are copies of one node plane.  Expected values come from the oracle on the cut mesh."""
    nelem = [4, 5, 6]
    mesh = fo.box_mesh(nelem, [0, 0, 0], [1, 1, 1], 2, jitter=0.2)
    N = mesh.n_node
    per_plane = (nelem[0] + 1) * (nelem[1] + 1)
    plane = np.arange(3 * per_plane, 4 * per_plane)                     # node plane z-index 3 (lexicographic ids)
    cells_per_layer = nelem[0] * nelem[1]
    conn = mesh.conn.copy()
    upper = conn[3 * cells_per_layer:]                                  # cell layers 3.. reference ghost copies
    ghost_of = np.full(N, -1)
    ghost_of[plane] = N + np.arange(per_plane)
    hit = ghost_of[upper] >= 0
    upper[hit] = ghost_of[upper][hit]
    xyz = np.vstack([mesh.xyz, mesh.xyz[plane]])
    cut = fo.BoxMesh(3, 2, tuple(nelem), mesh.lattice, conn.astype(np.int32), xyz, mesh.boundary, mesh.borders)
    ref = fo.assemble_scalar(cut, fo.Tables(2, 3), "laplace")["A"][:N]

    ctx = lib.Context(0)
    ctx.comm_init(0, 1, lib.Context.unique_id())                        # real RCCL communicator, one rank
    ctx.halo_set(N, per_plane, [0], [0, per_plane], plane.astype(np.int32), [0, per_plane])
    ctx.mesh_set(3, cut.conn, cut.xyz)
    from pynama_amd.elements.spectral import Spectral
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    ctx.csr_symbolic()
    # start-up self-test (what bench.py --gpus N runs first): both communicators counted by RCCL, rank-stamped exchanges on either
    # stream, and an all-reduce queued on the main stream while an exchange is in flight on the communication stream
    st = ctx.comm_selftest()
    assert st["transport"] == "rccl" and st["nranks_seen_by_rccl"] == 1 and st["halo_communicator"].startswith("own")
    assert st["allreduce_sum_ones"] == 1.0 and st["allreduce_beside_exchange_sum_ranks_plus_1"] == 1.0
    assert st["halo_ghosts_checked_main_stream"] == per_plane == st["halo_ghosts_checked_comm_stream"]
    # should RCCL refuse the split, the exchanges share the first communicator (reported, not fatal): same checks pass
    os.environ["PYNAMA_NO_COMM_SPLIT"] = "1"
    try:
        c2 = lib.Context(0)
        c2.comm_init(0, 1, lib.Context.unique_id())
    finally:
        del os.environ["PYNAMA_NO_COMM_SPLIT"]
    c2.halo_set(N, per_plane, [0], [0, per_plane], plane.astype(np.int32), [0, per_plane])
    c2.mesh_set(3, cut.conn, cut.xyz)
    st2 = c2.comm_selftest()
    assert st2["halo_communicator"].startswith("shared") and st2["halo_ghosts_checked_comm_stream"] == per_plane
    c2.close()
    A = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref) < FP_TOL
    rng = np.random.default_rng(3)
    x = rng.standard_normal(N)
    vx, vy = ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vx, x)                                                  # owned entries only: ghosts arrive by RCCL
    ctx.spmv(A, vx, vy)
    assert rel_err(ctx.vec_get(vy, 1), ref @ np.concatenate([x, x[plane]])) < 1e-13
    # 3-component vectors use the same plan with block size 3
    K = ctx.mat_create(3, 3)
    ctx.assemble_kle(1e3, 1e2, K, -1, -1, -1)
    S3 = mat_to_scipy(ctx, K, 3, 3)
    x3 = rng.standard_normal(3 * N)
    v3, w3 = ctx.vec_create(3), ctx.vec_create(3)
    ctx.vec_set(v3, x3)
    ctx.spmv(K, v3, w3)
    ext = np.concatenate([x3, x3.reshape(N, 3)[plane].ravel()])
    assert rel_err(ctx.vec_get(w3, 3), S3 @ ext) < 1e-12
    # reductions through ncclAllReduce
    assert abs(ctx.vec_dot(vx, vx) - x @ x) < 1e-11 * (x @ x)
    assert abs(ctx.vec_norm(vx, 2) - np.linalg.norm(x)) < 1e-12 * np.linalg.norm(x)
    assert np.allclose(ctx.allreduce([1.5, -2.0]), [1.5, -2.0])
    assert np.allclose(ctx.allreduce([1.5, -2.0], op="max"), [1.5, -2.0])
    ctx.barrier()
    ctx.close()


@pytest.mark.parametrize("method", ["cg", "gmres"])
def test_rccl_one_rank_solve_equals_serial(lib, method):
    """with a communicator the solve takes the distributed code path (single-reduction CG, all-reduced
    scalars); one rank must reproduce the serial iterates"""
    out = []
    for with_comm in (False, True):
        mesh = fo.box_mesh([10, 9, 8], [0, 0, 0], [1, 1, 1], 2, jitter=0.1)
        ctx = lib.Context(0)
        if with_comm:
            ctx.comm_init(0, 1, lib.Context.unique_id())
        ctx.mesh_set(3, mesh.conn, mesh.xyz)
        from pynama_amd.elements.spectral import Spectral
        for t in Spectral(2, 3).deviceTables():
            ctx.tables_set(*t)
        mask = np.zeros((mesh.n_node, 1), np.uint8)
        mask[mesh.boundary] = 1
        ctx.bc_set(1, mask)
        ctx.csr_symbolic()
        A = ctx.mat_create(1, 1)
        ctx.assemble_scalar(lib.FORM_LAPLACE, A)
        b = np.random.default_rng(0).standard_normal(mesh.n_node)
        vb, vx = ctx.vec_create(1), ctx.vec_create(1)
        ctx.vec_set(vb, b)
        kw = dict(method=lib.KSP_CG, cg_variant=2) if method == "cg" else dict(method=lib.KSP_GMRES, restart=30)
        info = ctx.solve(A, vb, vx, pc=lib.PC_JACOBI, rtol=1e-10, **kw)
        out.append((info.iters, info.reason, ctx.vec_get(vx, 1)))
        if with_comm and method == "cg":                                  # default variant with a communicator
            info = ctx.solve(A, vb, vx, pc=lib.PC_JACOBI, rtol=1e-10)
            assert info.iters == out[0][0]
        ctx.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] == 2
    assert rel_err(out[1][2], out[0][2]) < 1e-12


# ---- plan-free kernel for structured topology ---------------------------------------------------
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("nelem,jitter", [([11, 9, 10], 0.2), ([17, 6, 5], 0.0), ([2, 1, 3], 0.2), ([23, 19, 17], 0.1)])
def test_assemble_lattice_kernel(lib, tile, nelem, jitter):
    """box meshes are recognised as lattices and assembled without a patch plan (index arithmetic instead
    of plan streams): every tile shape, domain sizes that are not multiples of the tile, general and affine
    geometry, with / without the Dirichlet mask and the Arhs output -- all equal the oracle and the
    plan-based kernel"""
    import os
    mesh = fo.box_mesh(nelem, [0, 0, 0], [1.0, 0.8, 1.1], 2, jitter=jitter)
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=mesh.boundary)
    ref0 = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace")
    os.environ["PYNAMA_LATTICE_TILE"] = str(tile)
    try:
        ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
        assert ctx.mesh_topology() == ("lattice", nelem[0] + 1, nelem[1] + 1, nelem[2] + 1)
        rp, ci = ctx.csr_get()                       # closed-form symbolic phase == the oracle's graph, bit for bit
        rp_o, ci_o = fo.node_graph(mesh)
        assert np.array_equal(rp, rp_o) and np.array_equal(ci, ci_o)
        A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
        general = jitter > 0 and min(nelem) >= 2          # (the jitter moves interior nodes: [2, 1, 3] has none and stays a box)
        tiles = dict(shape=tile, k_closed=0 if general else 1, dinv=1, krhs_completed=0)   # a tile request keeps the tile kernel
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
        assert_assembled(ctx, lib.AK_LATTICE, **tiles)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
        assert_assembled(ctx, lib.AK_LATTICE, **tiles)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
        ctx.bc_set(1, None)
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
        assert_assembled(ctx, lib.AK_LATTICE, **tiles)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref0["A"]) < FP_TOL
        # an interior Dirichlet node set (not the lattice boundary): the mask is data, not topology
        rng = np.random.default_rng(5)
        some = np.sort(rng.choice(mesh.n_node, size=max(1, mesh.n_node // 7), replace=False))
        mask = np.zeros((mesh.n_node, 1), np.uint8)
        mask[some] = 1
        ctx.bc_set(1, mask)
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
        assert_assembled(ctx, lib.AK_LATTICE, **tiles)
        ref2 = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=some)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref2["A"]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref2["Arhs"]) < FP_TOL
        # without a tile request: parallelepipeds take the default tile, general geometry the z-marching kernel
        del os.environ["PYNAMA_LATTICE_TILE"]
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
        assert_assembled(ctx, lib.AK_MARCH if general else lib.AK_LATTICE, shape=0, k_closed=0 if general else 1, dinv=1)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref2["A"]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref2["Arhs"]) < FP_TOL
        ctx.close()
    finally:
        os.environ.pop("PYNAMA_LATTICE_TILE", None)


@pytest.mark.parametrize("kind", ["sheared", "mixed", "stretched"])
def test_lattice_kernel_parallelepipeds(lib, kind):
    """all-parallelepiped lattices take the lean path (4 corner loads, J from the edge vectors, L_ab formed on the
    fly); one non-affine element anywhere sends the whole mesh through the quadrature path.  Both equal the oracle's
    8-point rule."""
    mesh = fo.box_mesh([14, 9, 16], [0, 0, 0], [1.0, 0.7, 1.3], 2)
    if kind == "sheared":
        M = np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]])
        mesh.xyz = mesh.xyz @ M.T + np.array([0.5, -1.0, 2.0])
    if kind == "stretched":                              # graded spacing: every cell still a brick
        mesh.xyz = mesh.xyz ** np.array([1.7, 1.0, 2.3])
    if kind == "mixed":
        mv = np.zeros_like(mesh.xyz)
        mv[mesh.n_node // 2] = [0.01, -0.008, 0.012]     # one interior node off the lattice
        mesh.xyz = mesh.xyz + mv
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=mesh.boundary)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    assert ctx.mesh_topology()[0] == "lattice"
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("size,nz", [(2, 9), (3, 9), (4, 3)])
def test_lattice_kernel_on_rank_slabs(lib, size, nz):
    """a rank's z-slab is a lattice whose ghost planes carry the LAST node ids: the z-order table of the
    plan-free kernel sorts the column blocks of interface rows accordingly"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    nelem = [6, 5, nz]                                # (4, 3): every rank owns ONE node plane, ghosts on both sides
    glob = fo.box_mesh(nelem, [0, 0, 0], [1, 1, 1], 2, jitter=0.2)
    ref = fo.assemble_scalar(glob, fo.Tables(2, 3), "laplace", dirichlet=glob.boundary)
    for r in range(size):
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0, 0, 0], 'upper': [1, 1, 1]}, comm=Comm(r, size), jitter=0.2)
        dom.setFemIndexing(2)
        ctx = lib.Context(0)
        ctx.comm_init(r, size, None)
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(3, dom.conn, dom.xyz)
        for t in Spectral(2, 3).deviceTables():
            ctx.tables_set(*t)
        ctx.bc_set(1, dom.boundaryMaskLocal())
        ctx.csr_symbolic()
        assert ctx.mesh_topology() == ("lattice", 7, 6, dom.nLocal // 42)
        rp, ci = ctx.csr_get()                       # closed-form graph of the slab == owned rows of the global graph
        rp_g, ci_g = fo.node_graph(glob)
        l2g = dom._local2global(np.arange(dom.nLocal))
        for i in (0, dom.nOwned // 2, dom.nOwned - 1):
            gi = dom.rStart + i
            assert np.array_equal(np.sort(l2g[ci[rp[i]:rp[i + 1]]]), ci_g[rp_g[gi]:rp_g[gi + 1]])
            assert np.all(np.diff(ci[rp[i]:rp[i + 1]]) > 0)
        assert rp[-1] == sum(rp_g[dom.rStart + i + 1] - rp_g[dom.rStart + i] for i in range(dom.nOwned))
        A, Ar = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)          # no plan set: lattice kernel
        cols = dom._local2global(np.arange(dom.nLocal))
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Ar, 1, 1), ref["Arhs"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        ctx.close()


def test_rccl_overlapped_halo_in_cg(lib):
    """distributed CG multiplies the rows without ghost columns while the halo exchange of the search vector is in
    flight on a second stream, then the boundary rows.  One GPU, real one-rank communicator, the rank its own
    neighbour: ghost copies of the planes next to the bottom and the top plane, so that the rows needing ghosts are
    a prefix and a suffix of the slices (as for z-slabs).  Overlapped == in-order iterates; SpMV == oracle."""
    import os
    nelem = [8, 8, 12]
    mesh = fo.box_mesh(nelem, [0, 0, 0], [1, 1, 1], 2, jitter=0.2)
    N = mesh.n_node
    pp = 81
    nzp = nelem[2] + 1
    send = np.concatenate([np.arange(pp, 2 * pp), np.arange((nzp - 2) * pp, (nzp - 1) * pp)])   # planes 1 and nz-2
    ghost_of = np.full(N, -1)
    ghost_of[send] = N + np.arange(2 * pp)
    conn = mesh.conn.copy()
    cpl = nelem[0] * nelem[1]
    for layer, plane in ((0, 1), (nelem[2] - 1, nzp - 2)):            # bottom / top cell layer -> ghost copies
        blk = conn[layer * cpl:(layer + 1) * cpl]
        hit = (blk >= plane * pp) & (blk < (plane + 1) * pp)
        blk[hit] = ghost_of[blk][hit]
    xyz = np.vstack([mesh.xyz, mesh.xyz[send]])
    cut = fo.BoxMesh(3, 2, tuple(nelem), mesh.lattice, conn.astype(np.int32), xyz, mesh.boundary, mesh.borders)
    ref = fo.assemble_scalar(cut, fo.Tables(2, 3), "laplace")["A"][:N]
    from pynama_amd.elements.spectral import Spectral
    out = {}
    for mode in ("overlap", "inorder"):
        os.environ.pop("PYNAMA_NO_OVERLAP", None)
        os.environ.pop("PYNAMA_OVERLAP_REQUIRE", None)
        os.environ["PYNAMA_NO_OVERLAP" if mode == "inorder" else "PYNAMA_OVERLAP_REQUIRE"] = "1"
        try:
            ctx = lib.Context(0)
            ctx.comm_init(0, 1, lib.Context.unique_id())
            ctx.halo_set(N, 2 * pp, [0], [0, 2 * pp], send.astype(np.int32), [0, 2 * pp])
            ctx.mesh_set(3, cut.conn, cut.xyz)
            for t in Spectral(2, 3).deviceTables():
                ctx.tables_set(*t)
            ctx.csr_symbolic()
            A = ctx.mat_create(1, 1)
            ctx.assemble_scalar(lib.FORM_LAPLACE, A)
            assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref) < FP_TOL
            b = np.random.default_rng(2).standard_normal(N)
            vb, vx = ctx.vec_create(1), ctx.vec_create(1)
            ctx.vec_set(vb, b)
            info = ctx.solve(A, vb, vx, method=lib.KSP_CG, pc=lib.PC_JACOBI, fixed_iters=6, cg_variant=2)
            out[mode] = (info.iters, ctx.vec_get(vx, 1))
            ctx.close()
        finally:
            os.environ.pop("PYNAMA_NO_OVERLAP", None)
            os.environ.pop("PYNAMA_OVERLAP_REQUIRE", None)
    assert out["overlap"][0] == out["inorder"][0] == 6
    assert rel_err(out["overlap"][1], out["inorder"][1]) < 1e-11
    # and the iterates are those of the recurrences on the folded matrix (ghost column j -> owned node send[j])
    import scipy.sparse as sps
    fold = sps.vstack([sps.identity(N, format="csr"), sps.csr_matrix((np.ones(2 * pp), (np.arange(2 * pp), send)), shape=(2 * pp, N))])
    Af = (ref @ fold).tocsr()
    x = np.zeros(N); r = b.copy(); dinv = 1.0 / Af.diagonal()
    u = dinv * r; w = Af @ u
    gamma = r @ u; delta = w @ u
    p = np.zeros(N); sv = np.zeros(N); alpha = gamma / delta; beta = 0.0
    for it in range(6):                                           # Chronopoulos-Gear recurrences
        p = u + beta * p; sv = w + beta * sv
        x = x + alpha * p; r = r - alpha * sv
        u = dinv * r; w = Af @ u
        gn = r @ u; delta = w @ u
        beta = gn / gamma; alpha = gn / (delta - beta * gn / alpha); gamma = gn
    assert rel_err(out["overlap"][1], x) < 1e-9


# ---- plan-free KLE kernels on lattices of parallelepipeds ------------------------------------------
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["uniform", "sheared", "partial_bc", "nobc", "interior_bc"])
def test_assemble_kle_lattice_kernel(lib, tile, kind):
    """box meshes of parallelepipeds are assembled by the plan-free KLE kernels (K, Krhs, Rw): every tile shape,
    ragged domain sizes, full / per-component / no / interior Dirichlet masks, K without Krhs.  All equal the
    oracle (whose blocks come from the reference-pinned formulas)."""
    import os
    import scipy.sparse as sps
    mesh = fo.box_mesh([7, 5, 8], [0, 0, 0], [1.0, 0.9, 1.1], 2)
    if kind == "sheared":
        M = np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]])
        mesh.xyz = mesh.xyz @ M.T + np.array([0.5, -1.0, 2.0])
    mask = np.zeros((mesh.n_node, 3), np.uint8)
    if kind in ("uniform", "sheared"):
        mask[mesh.boundary] = 1
    elif kind == "partial_bc":                       # only the normal component on each border
        for name, (d, _) in {"back": (2, 0), "front": (2, 1), "down": (1, 0), "up": (1, 1), "right": (0, 1), "left": (0, 0)}.items():
            mask[mesh.borders[name], d] = 1
    elif kind == "interior_bc":
        rng = np.random.default_rng(3)
        mask[rng.choice(mesh.n_node, size=mesh.n_node // 6, replace=False), rng.integers(0, 3, size=mesh.n_node // 6)] = 1
    os.environ["PYNAMA_KLE_LATTICE_TILE"] = str(tile)
    try:
        from pynama_amd.elements.spectral import Spectral
        ctx = lib.Context(0)
        ctx.mesh_set(3, mesh.conn, mesh.xyz)
        for t in Spectral(2, 3).deviceTables():
            ctx.tables_set(*t)
        if kind != "nobc":
            ctx.bc_set(3, mask)
        ctx.csr_symbolic()
        assert ctx.mesh_topology()[0] == "lattice"
        K, Krhs, Rw = ctx.mat_create(3, 3), ctx.mat_create(3, 3), ctx.mat_create(3, 3)
        ctx.assemble_kle(1e3, 1e2, K, Krhs, Rw, -1)
        assert_assembled(ctx, lib.AK_KLE_LATTICE, shape=tile, k_closed=1, rw_closed=1, krhs_completed=0)   # parallelepipeds, every kind
        K2 = ctx.mat_create(3, 3)
        ctx.assemble_kle(1e3, 1e2, K2, -1, -1, -1)
        assert_assembled(ctx, lib.AK_KLE_LATTICE, shape=tile, k_closed=1, rw_closed=0)
        tb = fo.Tables(2, 3)
        Ke, Rwe, _ = fo.elem_kle_matrices(tb, mesh.corners())
        vdof = fo.dof_indices(mesh.conn, 3)
        is_bc = mask.ravel().astype(bool)
        n3 = mesh.n_node * 3
        rfree, cbc = ~is_bc[vdof], is_bc[vdof]
        R = np.broadcast_to(vdof[:, :, None], Ke.shape)
        C = np.broadcast_to(vdof[:, None, :], Ke.shape)
        mff = rfree[:, :, None] & rfree[:, None, :]
        mfb = rfree[:, :, None] & cbc[:, None, :]
        ident = sps.coo_matrix((np.ones(is_bc.sum()), (np.nonzero(is_bc)[0], np.nonzero(is_bc)[0])), shape=(n3, n3)).tocsr()
        Kref = (sps.coo_matrix((Ke[mff], (R[mff], C[mff])), shape=(n3, n3)).tocsr() + ident).tocsr()
        Krref = (sps.coo_matrix((-Ke[mfb], (R[mfb], C[mfb])), shape=(n3, n3)).tocsr() + ident).tocsr()
        mrow = np.broadcast_to(rfree[:, :, None], Rwe.shape)
        Rwref = sps.coo_matrix((Rwe[mrow], (R[mrow], C[mrow])), shape=(n3, n3)).tocsr()
        assert sp_rel_err(mat_to_scipy(ctx, K, 3, 3), Kref) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, K2, 3, 3), Kref) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Krhs, 3, 3), Krref) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Rw, 3, 3), Rwref) < FP_TOL
        Rw2 = ctx.mat_create(3, 3)
        ctx.assemble_kle(1e3, 1e2, -1, -1, Rw2, -1)          # Rw alone
        assert_assembled(ctx, lib.AK_KLE_LATTICE, shape=tile, k_closed=0, rw_closed=1)
        assert sp_rel_err(mat_to_scipy(ctx, Rw2, 3, 3), Rwref) < FP_TOL
        # and the patch-plan kernels (explicit plan) give the same matrices
        ctx.patch_plan_set(*tile_plan(mesh, (3, 3, 3)), kind=1)
        K3, Rw3 = ctx.mat_create(3, 3), ctx.mat_create(3, 3)
        ctx.assemble_kle(1e3, 1e2, K3, -1, Rw3, -1)
        assert_assembled(ctx, lib.AK_PATCH, shape=0, k_closed=1, rw_closed=1)
        assert sp_rel_err(mat_to_scipy(ctx, K3, 3, 3), Kref) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Rw3, 3, 3), Rwref) < FP_TOL
        ctx.close()
    finally:
        del os.environ["PYNAMA_KLE_LATTICE_TILE"]


@pytest.mark.parametrize("jitter", [0.0, 0.2])
@pytest.mark.parametrize("size,nz", [(2, 9), (3, 9), (4, 3)])
def test_kle_lattice_kernel_on_rank_slabs(lib, size, nz, jitter):
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    nelem = [5, 4, nz]
    glob = fo.box_mesh(nelem, [0, 0, 0], [1, 1, 1], 2, jitter=jitter)   # 0.2: general geometry (element pre-pass over the slab incl. ghost layers)
    ref = fo.assemble_kle_freeslip(glob, fo.Tables(2, 3))
    for r in range(size):
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0, 0, 0], 'upper': [1, 1, 1]}, comm=Comm(r, size), jitter=jitter)
        dom.setFemIndexing(2)
        ctx = lib.Context(0)
        ctx.comm_init(r, size, None)
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(3, dom.conn, dom.xyz)
        for t in Spectral(2, 3).deviceTables():
            ctx.tables_set(*t)
        ctx.bc_set(3, np.repeat(dom.boundaryMaskLocal()[:, None], 3, axis=1))
        ctx.csr_symbolic()
        K, Kr, Rw = ctx.mat_create(3, 3), ctx.mat_create(3, 3), ctx.mat_create(3, 3)
        ctx.assemble_kle(1e3, 1e2, K, Kr, Rw, -1)
        closed = 0 if jitter else 1          # general geometry: the one-shape kernel with the closed form of the 2x2x2 rule
        assert_assembled(ctx, lib.AK_KLE_LATTICE, shape=0, k_closed=closed, rw_closed=closed)
        cols = dom._local2global(np.arange(dom.nLocal))
        rows3 = (np.arange(dom.rStart, dom.rEnd)[:, None] * 3 + np.arange(3)).ravel()
        cols3 = (cols[:, None] * 3 + np.arange(3)).ravel()
        for mid, name in ((K, "K"), (Kr, "Krhs"), (Rw, "Rw")):
            assert sp_rel_err(mat_to_scipy(ctx, mid, 3, 3), ref[name][rows3][:, cols3]) < FP_TOL, name
        ctx.close()


def test_lattice_kernels_fuzz_against_generic(lib):
    """seeded sweep over box sizes, geometry (uniform / sheared / jittered), Dirichlet masks, tile shapes and slab
    partitions: the plan-free scalar and KLE kernels equal the generic atomics kernel entry by entry (both on the
    device: an independent implementation with a different data path)"""
    import os
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    rng = np.random.default_rng(20240607)
    tables = Spectral(2, 3).deviceTables()
    for case in range(24):
        nelem = [int(v) for v in rng.integers(1, 15, size=3)]
        size = int(rng.choice([1, 1, 2, 3]))
        if nelem[2] + 1 < size:
            size = 1
        geom = rng.choice(["uniform", "sheared", "jitter"])
        rank = int(rng.integers(0, size))
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0, 0, 0], 'upper': [1.0, 0.7, 1.3]}, comm=Comm(rank, size),
                        jitter=0.2 if geom == "jitter" else 0.0)
        dom.setFemIndexing(2)
        xyz = dom.xyz
        if geom == "sheared":
            xyz = xyz @ np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]]).T
        os.environ["PYNAMA_LATTICE_TILE"] = str(int(rng.integers(0, 10)))
        os.environ["PYNAMA_KLE_LATTICE_TILE"] = str(int(rng.integers(0, 4)))
        try:
            ctx = lib.Context(0)
            if size > 1:
                ctx.comm_init(rank, size, None)
                ctx.halo_set(*dom._halo_plan())
            ctx.mesh_set(3, dom.conn, xyz)
            for t in tables:
                ctx.tables_set(*t)
            ctx.csr_symbolic()
            assert ctx.mesh_topology()[0] == "lattice"
            # scalar
            mask = (rng.random(dom.nLocal) < rng.choice([0.0, 0.1, 0.5])).astype(np.uint8)
            ctx.bc_set(1, mask if mask.any() else None)
            A, Ar, B, Br = (ctx.mat_create(1, 1) for _ in range(4))
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)                 # lattice kernel
            ctx.assemble_scalar(lib.FORM_LAPLACE, B, Br, variant=0)      # generic atomics kernel
            for x, y in ((A, B), (Ar, Br)):
                vx, vy = ctx.mat_values(x, 1, 1), ctx.mat_values(y, 1, 1)
                assert np.abs(vx - vy).max() <= FP_TOL * max(1e-300, np.abs(vy).max()), (case, nelem, size, rank, geom)
            # KLE (plan-free lattice kernels: closed-form blocks on parallelepipeds, the closed form of the 2x2x2 rule on jittered meshes)
            mask3 = (rng.random((dom.nLocal, 3)) < rng.choice([0.0, 0.15])).astype(np.uint8)
            ctx.bc_set(3, mask3 if mask3.any() else None)
            K, Kr, Rw, K0, Kr0, Rw0 = (ctx.mat_create(3, 3) for _ in range(6))
            ctx.assemble_kle(1e3, 1e2, K, Kr, Rw, -1)
            ctx.assemble_kle(1e3, 1e2, K0, Kr0, Rw0, -1, variant=0)
            for x, y in ((K, K0), (Kr, Kr0), (Rw, Rw0)):
                vx, vy = ctx.mat_values(x, 3, 3), ctx.mat_values(y, 3, 3)
                assert np.abs(vx - vy).max() <= FP_TOL * max(1e-300, np.abs(vy).max()), (case, nelem, size, rank, geom, "kle")
            ctx.close()
        finally:
            del os.environ["PYNAMA_LATTICE_TILE"]
            del os.environ["PYNAMA_KLE_LATTICE_TILE"]


# ---- matrix-free operator (no assembled matrix inside the CG iteration) -----------------------------------------
def _shear(mesh):
    """affine map of the whole box: every element stays a parallelepiped, none is a brick"""
    M = np.array([[1.0, 0.3, 0.1], [0.0, 0.9, 0.2], [0.05, 0.0, 1.1]])
    mesh.xyz = mesh.xyz @ M.T
    return mesh


@pytest.mark.parametrize("nelem,geom,bc", [
    ([20, 11, 13], "uniform", "boundary"), ([20, 11, 13], "shear", "left"), ([20, 11, 13], "jitter", "boundary"),
    ([5, 4, 3], "jitter", "none"), ([33, 9, 9], "uniform", "none"), ([17, 18, 10], "shear", "boundary")])
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_matfree_laplace_vs_oracle(lib, monkeypatch, nelem, geom, bc, tile):
    """y = A x without the matrix == the oracle's assembled Laplacian (Dirichlet rows identity, columns eliminated)
    applied to x; parallelepiped (closed-form L_e) and general (per-Gauss-point apply) paths, all tile shapes (6-9: the
    column-marching kernel on parallelepipeds), tiles that overhang the lattice, masks on all / one / no face"""
    monkeypatch.setenv("PYNAMA_MATFREE_TILE", str(tile))
    mesh = fo.box_mesh(nelem, [0.0] * 3, [1.0, 0.8, 1.2], 2, jitter=0.2 if geom == "jitter" else 0.0)
    if geom == "shear":
        _shear(mesh)
    nodes = {"boundary": mesh.boundary, "left": mesh.borders["left"], "none": np.zeros(0, np.int64)}[bc]
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=nodes)
    assert ctx.mesh_topology()[0] == "lattice"
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=nodes)
    x = np.random.default_rng(5).standard_normal(mesh.n_node)
    vx, vy = ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vx, x)
    with pytest.raises(lib.PynamaHipError, match="pyn_matfree_set first"):
        ctx.matfree_apply(vx, vy)
    ctx.matfree_set(lib.MATFREE_LAPLACE)
    ctx.bc_set(1, None)                       # the operator keeps the mask it was defined with
    ctx.matfree_apply(vx, vy)
    assert rel_err(ctx.vec_get(vy, 1), ref["A"] @ x) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("geom,variant", [("uniform", 1), ("jitter", 1), ("shear", 2)])
def test_matfree_cg_equals_assembled_cg(lib, geom, variant):
    """CG driven by the matrix-free operator (assembled matrix = Jacobi diagonal + exit check only) reproduces the
    assembled-matrix solve: same iteration count (+-1), same solution, true residual (computed with the ASSEMBLED
    matrix) below the bar; an assembled matrix that is not this operator is refused"""
    mesh = fo.box_mesh([18, 12, 10], [0.0] * 3, [1.0] * 3, 2, jitter=0.2 if geom == "jitter" else 0.0)
    if geom == "shear":
        _shear(mesh)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
    A, M = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    ctx.assemble_scalar(lib.FORM_MASS_NODAL, M)
    ctx.matfree_set(lib.MATFREE_LAPLACE)
    b = np.random.default_rng(9).standard_normal(mesh.n_node)
    b[mesh.boundary] = 0.0
    vb, vx = ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vb, b)
    kw = dict(rtol=1e-10, norm_type=lib.NORM_UNPRECONDITIONED, cg_variant=variant)
    i0 = ctx.solve(A, vb, vx, **kw)
    x0 = ctx.vec_get(vx, 1)
    i1 = ctx.solve(A, vb, vx, matfree=lib.MATFREE_LAPLACE, **kw)
    x1 = ctx.vec_get(vx, 1)
    assert i0.reason == 2 and i1.reason == 2 and abs(i0.iters - i1.iters) <= 1
    assert i1.true_resid < 2e-10 and rel_err(x1, x0) < 1e-8
    with pytest.raises(lib.PynamaHipError, match="differs from the assembled matrix"):
        ctx.solve(M, vb, vx, matfree=lib.MATFREE_LAPLACE, **kw)
    g0 = ctx.solve(A, vb, vx, method=lib.KSP_GMRES, rtol=1e-9)
    xg0 = ctx.vec_get(vx, 1)
    g1 = ctx.solve(A, vb, vx, method=lib.KSP_GMRES, rtol=1e-9, matfree=lib.MATFREE_LAPLACE)
    assert g0.reason == 2 and g1.reason == 2 and abs(g0.iters - g1.iters) <= 2 and rel_err(ctx.vec_get(vx, 1), xg0) < 1e-7
    ctx.close()


def test_matfree_needs_structured_topology(lib):
    mesh = fo.box_mesh([5, 4, 3], [0, 0, 0], [1, 1, 1], 2)
    perm = np.random.default_rng(1).permutation(mesh.n_node)
    mesh.conn = perm[mesh.conn].astype(np.int32)
    mesh.xyz = mesh.xyz[np.argsort(perm)]
    ctx = make_ctx(lib, mesh, 2)
    vx, vy = ctx.vec_create(1), ctx.vec_create(1)
    with pytest.raises(lib.PynamaHipError, match="structured topology"):
        ctx.matfree_set(lib.MATFREE_LAPLACE)
    ctx.close()


@pytest.mark.parametrize("size", [2, 3])
def test_matfree_on_rank_slabs(lib, size):
    """a rank's z-slab (owned planes + ghost planes, ghosts at the vector tail): matrix-free rows == serial rows"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    nelem = [6, 5, 9]
    for jitter in (0.0, 0.2):
        glob = fo.box_mesh(nelem, [0, 0, 0], [1, 1, 1], 2, jitter=jitter)
        ref = fo.assemble_scalar(glob, fo.Tables(2, 3), "laplace", dirichlet=glob.boundary)
        xg = np.random.default_rng(11).standard_normal(glob.n_node)
        yg = ref["A"] @ xg
        for r in range(size):
            dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0, 0, 0], 'upper': [1, 1, 1]}, comm=Comm(r, size), jitter=jitter)
            dom.setFemIndexing(2)
            ctx = lib.Context(0)
            ctx.comm_init(r, size, None)                      # detached
            ctx.halo_set(*dom._halo_plan())
            ctx.mesh_set(3, dom.conn, dom.xyz)
            for t in Spectral(2, 3).deviceTables():
                ctx.tables_set(*t)
            ctx.bc_set(1, dom.boundaryMaskLocal())
            ctx.csr_symbolic()
            cols = dom._local2global(np.arange(dom.nLocal))
            vx, vy = ctx.vec_create(1), ctx.vec_create(1)
            ctx.vec_set_local(vx, xg[cols])
            ctx.matfree_set(lib.MATFREE_LAPLACE)
            ctx.matfree_apply(vx, vy)
            assert rel_err(ctx.vec_get(vy, 1), yg[dom.rStart:dom.rEnd]) < FP_TOL
            ctx.close()


@pytest.mark.parametrize("nelem,geom,bc", [
    ([11, 9, 10], "uniform", "boundary"), ([11, 9, 10], "shear", "mixed"), ([11, 9, 10], "jitter", "boundary"),
    ([5, 4, 3], "jitter", "none"), ([19, 5, 5], "shear", "none")])
@pytest.mark.parametrize("tile", [0, 1, 2, 3])
def test_matfree_kle_vs_oracle(lib, monkeypatch, nelem, geom, bc, tile):
    """y = K x for the KLE stiffness without the matrix == the oracle's assembled K (per-DOF Dirichlet elimination)
    applied to x; "mixed": different components imposed on different faces"""
    monkeypatch.setenv("PYNAMA_MATFREE_TILE", str(tile))
    mesh = fo.box_mesh(nelem, [0.0] * 3, [1.0, 0.8, 1.2], 2, jitter=0.2 if geom == "jitter" else 0.0)
    if geom == "shear":
        _shear(mesh)
    mask = np.zeros((mesh.n_node, 3), np.uint8)
    if bc == "boundary":
        mask[mesh.boundary] = 1
    elif bc == "mixed":
        mask[mesh.borders["left"], 0] = 1
        mask[mesh.borders["up"], 1] = 1
        mask[mesh.borders["front"], :] = 1
    ctx = make_ctx(lib, mesh, 2)
    ctx.bc_set(3, mask)
    K = ctx.mat_create(3, 3)
    ctx.assemble_kle(1e3, 1e2, K)
    Ks = mat_to_scipy(ctx, K, 3, 3)
    if bc == "boundary":   # the oracle's free-slip assembly imposes the boundary nodes; other masks: the assembled K
        assert sp_rel_err(Ks, fo.assemble_kle_freeslip(mesh, fo.Tables(2, 3))["K"]) < FP_TOL
    x = np.random.default_rng(6).standard_normal(mesh.n_node * 3)
    vx, vy = ctx.vec_create(3), ctx.vec_create(3)
    ctx.vec_set(vx, x)
    with pytest.raises(lib.PynamaHipError, match="pyn_matfree_set first"):
        ctx.matfree_apply(vx, vy, op=lib.MATFREE_KLE)
    ctx.matfree_kle_set(1e3, 1e2)
    ctx.matfree_apply(vx, vy, op=lib.MATFREE_KLE)
    assert rel_err(ctx.vec_get(vy, 3), Ks @ x) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("geom", ["uniform", "jitter"])
def test_matfree_kle_cg_equals_assembled_cg(lib, geom):
    """the reference's solveKLE system (uniform-flow boundary data) solved with the matrix-free K: same iterates"""
    mesh = fo.box_mesh([10, 9, 8], [0.0] * 3, [1.0] * 3, 2, jitter=0.2 if geom == "jitter" else 0.0)
    ctx = make_ctx(lib, mesh, 2, bc_ndof=3, bc_nodes=mesh.boundary)
    K, Krhs = ctx.mat_create(3, 3), ctx.mat_create(3, 3)
    ctx.assemble_kle(1e3, 1e2, K, Krhs)
    vel = np.zeros((mesh.n_node, 3))
    vel[mesh.boundary] = [1.0, 0.5, -0.25]
    vv, vb, vx = ctx.vec_create(3), ctx.vec_create(3), ctx.vec_create(3)
    ctx.vec_set(vv, vel.ravel())
    ctx.spmv(Krhs, vv, vb)
    kw = dict(rtol=1e-10, norm_type=lib.NORM_UNPRECONDITIONED)
    i0 = ctx.solve(K, vb, vx, **kw)
    x0 = ctx.vec_get(vx, 3)
    ctx.matfree_kle_set(1e3, 1e2)
    i1 = ctx.solve(K, vb, vx, matfree=lib.MATFREE_KLE, **kw)
    x1 = ctx.vec_get(vx, 3)
    # penalty-weighted system (cond ~ 1e3 x Laplacian): the products differ in summation order, the stopping iteration by 2-3
    assert i0.reason == 2 and i1.reason == 2 and abs(i0.iters - i1.iters) <= max(3, i0.iters // 50)
    assert i1.true_resid < 2e-10 and rel_err(x1, x0) < 1e-8
    assert np.abs(x1.reshape(-1, 3) - [1.0, 0.5, -0.25]).max() < 1e-7       # uniform flow is the exact solution
    ctx.matfree_kle_set(1e3, 5e1)                                            # not the assembled operator
    with pytest.raises(lib.PynamaHipError, match="differs from the assembled matrix"):
        ctx.solve(K, vb, vx, matfree=lib.MATFREE_KLE, **kw)
    ctx.close()


def test_matfree_fuzz_against_assembled(lib):
    """seeded sweep over box sizes (down to one element), geometry, random per-DOF Dirichlet masks, tile shapes and slab
    partitions (detached ranks, ghost values supplied): the matrix-free scalar and KLE products equal the products with the
    matrices assembled by the generic atomics kernel (an independent data path, itself checked against the oracle)"""
    import os
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    rng = np.random.default_rng(20241004)
    tables = Spectral(2, 3).deviceTables()
    for case in range(28):
        nelem = [int(v) for v in rng.integers(1, 20, size=3)]
        size = int(rng.choice([1, 1, 2, 3]))
        if nelem[2] + 1 < size:
            size = 1
        geom = rng.choice(["uniform", "sheared", "jitter"])
        rank = int(rng.integers(0, size))
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0, 0, 0], 'upper': [1.0, 0.7, 1.3]}, comm=Comm(rank, size),
                        jitter=0.2 if geom == "jitter" else 0.0)
        dom.setFemIndexing(2)
        xyz = dom.xyz
        if geom == "sheared":
            xyz = xyz @ np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]]).T
        os.environ["PYNAMA_MATFREE_TILE"] = str(int(rng.integers(0, 10)))
        try:
            ctx = lib.Context(0)
            if size > 1:
                ctx.comm_init(rank, size, None)
                ctx.halo_set(*dom._halo_plan())
            ctx.mesh_set(3, dom.conn, xyz)
            for t in tables:
                ctx.tables_set(*t)
            ctx.csr_symbolic()
            tag = (case, nelem, size, rank, str(geom), os.environ["PYNAMA_MATFREE_TILE"])
            # scalar Laplacian
            mask = (rng.random(dom.nLocal) < rng.choice([0.0, 0.1, 0.5])).astype(np.uint8)
            ctx.bc_set(1, mask if mask.any() else None)
            A = ctx.mat_create(1, 1)
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, variant=0)
            ctx.matfree_set(lib.MATFREE_LAPLACE)
            vx, vy, vz = ctx.vec_create(1), ctx.vec_create(1), ctx.vec_create(1)
            ctx.vec_set_local(vx, rng.standard_normal(dom.nLocal))
            ctx.spmv(A, vx, vy)
            ctx.matfree_apply(vx, vz)
            assert rel_err(ctx.vec_get(vz, 1), ctx.vec_get(vy, 1)) < FP_TOL, tag
            # KLE stiffness, random per-DOF mask
            mask3 = (rng.random((dom.nLocal, 3)) < rng.choice([0.0, 0.15, 0.6])).astype(np.uint8)
            ctx.bc_set(3, mask3 if mask3.any() else None)
            K = ctx.mat_create(3, 3)
            ctx.assemble_kle(1e3, 1e2, K, variant=0)
            ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
            wx, wy, wz = ctx.vec_create(3), ctx.vec_create(3), ctx.vec_create(3)
            ctx.vec_set_local(wx, rng.standard_normal(dom.nLocal * 3))
            ctx.spmv(K, wx, wy)
            ctx.matfree_apply(wx, wz, op=lib.MATFREE_KLE)
            assert rel_err(ctx.vec_get(wz, 3), ctx.vec_get(wy, 3)) < FP_TOL, tag + ("kle",)
            ctx.close()
        finally:
            del os.environ["PYNAMA_MATFREE_TILE"]


# ---- Jacobi data written by the assembly itself (DMat::dinv): same iterates as the extracted diagonal ----------------------
@pytest.mark.parametrize("jitter,tile", [(0.0, None), (0.2, None), (0.2, "1"), (0.0, "2")])
def test_assembly_emits_jacobi_diagonal(lib, jitter, tile):
    """the lattice store phases (tile kernels, z-marching kernel, interior and boundary / Dirichlet rows) write 1 / diagonal with
    the rows; CG with that data equals CG with the diagonal extracted from the CSR values (PYNAMA_NO_ASM_DINV), iterate by
    iterate, and re-assembling a matrix refreshes it"""
    mesh = fo.box_mesh([17, 12, 19], [0, 0, 0], [1.0, 0.8, 1.1], 2, jitter=jitter)
    rng = np.random.default_rng(3)
    some = np.unique(np.concatenate([mesh.boundary, rng.choice(mesh.n_node, size=40, replace=False)]))
    b = rng.standard_normal(mesh.n_node)
    b[some] = 0.0
    xs = []
    for no_dinv in (False, True):
        if no_dinv:
            os.environ["PYNAMA_NO_ASM_DINV"] = "1"
        if tile:
            os.environ["PYNAMA_LATTICE_TILE"] = tile
        try:
            ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=some)
            A = ctx.mat_create(1, 1)
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
            assert_assembled(ctx, lib.AK_LATTICE if tile or not jitter else lib.AK_MARCH, dinv=0 if no_dinv else 1)
            vb, vx = ctx.vec_create(1), ctx.vec_create(1)
            ctx.vec_set(vb, b)
            ctx.solve(A, vb, vx, fixed_iters=25, norm_type=lib.NORM_UNPRECONDITIONED)
            x1 = ctx.vec_get(vx, 1).copy()
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)      # second version of the same matrix
            assert_assembled(ctx, lib.AK_LATTICE if tile or not jitter else lib.AK_MARCH, dinv=0 if no_dinv else 1, count=2)
            ctx.solve(A, vb, vx, fixed_iters=25, norm_type=lib.NORM_UNPRECONDITIONED)
            x2 = ctx.vec_get(vx, 1)      # (LDS atomics: the summation order of an entry, hence its last bit, varies between launches)
            assert np.abs(x1 - x2).max() <= 1e-12 * np.abs(x1).max()
            d = ctx.vec_create(1)
            ctx.mat_diagonal(A, d)
            assert np.abs(ctx.vec_get(d, 1)[some] - 1.0).max() == 0.0          # identity rows
            xs.append(x1)
            ctx.close()
        finally:
            os.environ.pop("PYNAMA_NO_ASM_DINV", None)
            os.environ.pop("PYNAMA_LATTICE_TILE", None)
    assert np.abs(xs[0] - xs[1]).max() <= 1e-13 * np.abs(xs[1]).max()


@pytest.mark.parametrize("tile", ["0", "1", "2", "5", "7", "9", "12", "13", "14"])
def test_march_kernel_shapes_vs_oracle(lib, tile):
    """every shape of the z-marching general-geometry kernel (PYNAMA_MARCH_TILE: one-wave 7x7 columns, two- to four-wave
    15x7 / 15x11 / 15x15 columns, rolled and unrolled Gauss loops) against the oracle: boundary columns, partial columns
    (the mesh is no multiple of any shape), interior Dirichlet nodes, Arhs"""
    mesh = fo.box_mesh([19, 17, 23], [0, 0, 0], [1.0, 0.9, 1.2], 2, jitter=0.25)
    rng = np.random.default_rng(17)
    some = np.unique(np.concatenate([mesh.boundary, rng.choice(mesh.n_node, size=60, replace=False)]))
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=some)
    os.environ["PYNAMA_MARCH_TILE"] = tile
    os.environ["PYNAMA_MARCH_ZLEN"] = "5"          # several z-chunks per column
    try:
        ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=some)
        A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
        assert_assembled(ctx, lib.AK_MARCH, shape=int(tile), k_closed=0, dinv=1, krhs_completed=0)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
        ctx.close()
    finally:
        os.environ.pop("PYNAMA_MARCH_TILE", None)
        os.environ.pop("PYNAMA_MARCH_ZLEN", None)


@pytest.mark.parametrize("form", ["kle", "scalar_uniform", "scalar_jitter"])
def test_imposed_column_matrices_rewritten_only_where_needed(lib, form):
    """Krhs / Arhs are zero except next to imposed nodes; the lattice kernels leave the zero rows of tiles without imposed nodes
    unwritten when the matrix is known to hold zeros there (fresh / zeroed matrix, or the last assembly used the same Dirichlet
    set: DMat::rhs_clean).  Every sequence that could leave stale entries behind -- another Dirichlet set, values added behind the
    library's back through the ABI, a matrix that served another purpose -- must still end in exactly the generic kernel's matrix."""
    kle = form == "kle"
    nd = 3 if kle else 1
    mesh = fo.box_mesh([14, 12, 13], [0, 0, 0], [1.0, 0.9, 1.1], 2, jitter=0.2 if form == "scalar_jitter" else 0.0)
    rng = np.random.default_rng(23)
    setA = np.zeros((mesh.n_node, nd), np.uint8)
    setA[mesh.boundary] = 1
    setB = np.zeros((mesh.n_node, nd), np.uint8)
    setB[rng.choice(mesh.n_node, size=40, replace=False)] = 1
    ctx = make_ctx(lib, mesh, 2)
    assert ctx.mesh_topology()[0] == "lattice"
    M, Mr, G, Gr = (ctx.mat_create(nd, nd) for _ in range(4))
    W = ctx.mat_create(3, 3) if kle else -1

    def assemble(main, rhs, variant):
        if kle:
            ctx.assemble_kle(1e3, 1e2, main, rhs, W if variant else -1, -1, variant=variant)
        else:
            ctx.assemble_scalar(lib.FORM_LAPLACE, main, rhs, variant=variant)

    def check(tag):
        assemble(M, Mr, 1)                          # lattice kernels
        assemble(G, Gr, 0)                          # generic kernel: zero fill + atomics
        a, b = ctx.mat_values(Mr, nd, nd), ctx.mat_values(Gr, nd, nd)
        assert np.abs(a - b).max() <= FP_TOL * np.abs(b).max(), tag
        a, b = ctx.mat_values(M, nd, nd), ctx.mat_values(G, nd, nd)
        assert np.abs(a - b).max() <= FP_TOL * np.abs(b).max(), tag

    ctx.bc_set(nd, setA)
    check("fresh matrix")
    check("same Dirichlet set again")
    ctx.bc_set(nd, setB)
    check("another Dirichlet set: the entries next to the old one must go")
    ctx.bc_set(nd, setA)
    check("back to the first set")
    ctx.mat_axpy(Mr, 1.0, M)                        # the matrix served another purpose
    check("after mat_axpy")
    n = mesh.n_node * nd
    mid = (n // 2 // nd) * nd
    ctx.mat_add_values(Mr, [mid], [mid], [[3.0]], insert=False)   # an entry in the middle of the box
    check("after host insertion")
    ctx.mat_zero(Mr)
    check("after mat_zero")
    os.environ["PYNAMA_RHS_FULL_WRITE"] = "1"
    try:
        check("full write forced")
    finally:
        del os.environ["PYNAMA_RHS_FULL_WRITE"]
    ctx.close()


@pytest.mark.parametrize("nelem", [[9, 8, 7], [3, 2, 2], [30, 5]])
def test_csr_product_equals_sell_image_product(lib, nelem):
    """scalar matrices that follow the column-pattern dictionary are multiplied straight from their CSR values (csrl_spmv_kernel:
    64-row runs transposed through LDS, no SELL image, nothing to refresh after an assembly); PYNAMA_SELL_IMAGE=1 keeps the
    image-based kernel.  Both equal scipy's product -- partial last slice, rows of every length (faces, edges, corners), CG on top."""
    mesh = fo.box_mesh(nelem, [0.0] * len(nelem), [1.0, 0.9, 1.2][:len(nelem)], 2, jitter=0.2)
    rng = np.random.default_rng(3)
    xin = rng.standard_normal(mesh.n_node)
    out = {}
    for mode in ("csr", "image"):
        if mode == "image":
            os.environ["PYNAMA_SELL_IMAGE"] = "1"
        try:
            ctx = make_ctx(lib, mesh, 2, bc_ndof=1, bc_nodes=mesh.boundary)
            A = ctx.mat_create(1, 1)
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
            S = mat_to_scipy(ctx, A, 1, 1)
            vx, vy, vb = ctx.vec_create(1), ctx.vec_create(1), ctx.vec_create(1)
            ctx.vec_set(vx, xin)
            b = S @ xin
            ctx.vec_set(vb, b)
            info = ctx.solve(A, vb, vy, rtol=1e-12, maxit=2000, norm_type=lib.NORM_UNPRECONDITIONED)   # the product inside CG
            assert info.reason > 0 and info.true_resid < 1e-11
            sol = ctx.vec_get(vy, 1).copy()
            ctx.spmv(A, vx, vy)                                                                         # host-facing product
            out[mode] = (ctx.vec_get(vy, 1).copy(), sol, info.iters)
            assert np.abs(out[mode][0] - b).max() <= 1e-13 * np.abs(b).max()
            ctx.close()
        finally:
            os.environ.pop("PYNAMA_SELL_IMAGE", None)
    assert np.abs(out["csr"][1] - out["image"][1]).max() <= 1e-9 * np.abs(out["image"][1]).max()
    assert abs(out["csr"][2] - out["image"][2]) <= 1


# ---- the record of what ran equals the chooser's answer for the facts of the context -----------------------------------------
def _permuted(mesh, seed=4):
    perm = np.random.default_rng(seed).permutation(mesh.n_node)
    mesh.conn = perm[mesh.conn].astype(np.int32)
    mesh.xyz = mesh.xyz[np.argsort(perm)]
    mesh.boundary = np.sort(perm[mesh.boundary])
    return mesh


@pytest.mark.parametrize("name", ["q1_3d", "q1_3d_jitter", "q1_3d_general", "q1_2d", "ngl3_2d", "ngl3_3d", "ngl4_2d", "tets",
                                  "q1_3d_permuted"])
def test_assemble_last_matches_choose(lib, name):
    """assemble the scalar Laplacian and K / Krhs / Rw once on a tiny mesh of every family, feed the facts of the context -- read back
    through the ABI where it reports them, known from how the mesh was made otherwise -- to the host chooser, and compare its answer
    with the record of what ran"""
    from pynama_amd.elements.simplex import Simplex
    from pynama_amd.elements.spectral import Spectral
    nelem, ngl, jitter = {"q1_3d": ([2, 1, 3], 2, 0.0), "q1_3d_jitter": ([2, 1, 3], 2, 0.2), "q1_3d_general": ([2, 2, 3], 2, 0.2),
                          "q1_2d": ([3, 2], 2, 0.0),
                          "ngl3_2d": ([3, 2], 3, 0.0), "ngl3_3d": ([2, 2, 2], 3, 0.0), "ngl4_2d": ([2, 2], 4, 0.0),
                          "tets": ([1, 1, 1], 2, 0.0), "q1_3d_permuted": ([2, 1, 3], 2, 0.0)}[name]
    dim = len(nelem)
    if name == "tets":
        mesh = fo.simplex_box_mesh(nelem, [0.0] * dim, [1.0] * dim)
        assert mesh.n_elem == 6
        tables = Simplex(dim).deviceTables()
    else:
        mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0, 0.8, 1.1][:dim], ngl, jitter=jitter)
        if name == "q1_3d_permuted":
            mesh = _permuted(mesh)
        tables = Spectral(ngl, dim).deviceTables()
    ctx = lib.Context(0)
    ctx.mesh_set(dim, mesh.conn, mesh.xyz)
    for t in tables:
        ctx.tables_set(*t)
    ctx.csr_symbolic()
    topo = ctx.mesh_topology()[0]
    assert topo == {"q1_3d": "lattice", "q1_3d_jitter": "lattice", "q1_3d_general": "lattice", "q1_2d": "lattice-q1-2d", "ngl3_2d": "lattice-ngl3",
                    "ngl3_3d": "lattice-ngl3"}.get(name, "general")
    nn = mesh.conn.shape[1]
    hex8 = dim == 3 and nn == 8
    affine = 0 if jitter and min(nelem) >= 2 else 1      # the jitter moves interior nodes: [2, 1, 3] has none and stays a box
    facts = dict(dim=dim, nn=nn, nc=dim + 1 if name == "tets" else 2 ** dim, ngl=ngl, const_grad=name == "tets",
                 q1_gauss_standard=hex8, q1_red_standard=hex8, aff_standard=hex8, aff_rw_standard=hex8,
                 mesh_affine=affine if hex8 else -1, lat_valid=topo == "lattice", lat_std_ok=1 if topo == "lattice" else -1,
                 ho3_valid=topo != "general", ho3_affine=affine if topo.startswith("lattice-") else -1, ho3_tabs_nn=nn,
                 ho3_tabs_ok0=topo != "general", ho3_tabs_ok1=topo != "general", ho3_tabs_ok2=topo != "general")
    for t in tables:
        facts["ngp%d" % t[0]] = np.size(t[1])
    dw = 1 if dim == 2 else 3
    mask = np.zeros((mesh.n_node, dim), np.uint8)
    mask[mesh.boundary] = 1
    mats = [ctx.mat_create(1, 1), ctx.mat_create(1, 1), ctx.mat_create(dim, dim), ctx.mat_create(dim, dim), ctx.mat_create(dim, dw)]
    for form in (lib.FORM_LAPLACE, lib.FORM_KLE):
        if form == lib.FORM_KLE:
            ctx.bc_set(dim, mask)
            ctx.assemble_kle(1e3, 1e2, *mats[2:], -1)
        else:
            ctx.bc_set(1, np.ascontiguousarray(mask[:, :1]))
            ctx.assemble_scalar(form, *mats[:2])
        for kd in (0, 1):      # after the assembly: it builds the automatic plan of a graph without one
            facts["plan%d_present" % kd] = ctx.patch_plan_info(kd)[0] > 0
        want = lib.assemble_choose(dict(form=form, K=1, Krhs=1, Rw=form == lib.FORM_KLE), facts)
        last = ctx.assemble_last()
        assert {k: last[k] for k in want if k in last} == {k: v for k, v in want.items() if k in last}, (name, form, want, last)
    assert last["count"] == 2
    ctx.close()
