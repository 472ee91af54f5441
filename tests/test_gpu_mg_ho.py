"""Multigrid-preconditioned CG on box lattices of order ngl >= 4 (pynama_amd/csrc/pyn_mg.hip): level 1 is the Q1 lattice of the same
cells, reached through P0 (tests/mg_ho_model.py).  The Galerkin levels against P^T A P of the model, one V-cycle against the numpy
restatement, the symmetry of the preconditioner, CG+MG against Jacobi-PCG and the model's PCG (assembled product and ngl >= 4 shell),
the hierarchy cache, the refusals and the KspSolver facade."""
import types

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import mg_ho_model as mm
from tests.test_gpu_ho3 import boundary_mask, make_ctx
from tests.test_gpu_mg import decoupled, numpy_vcycle, stencil_to_scipy
from tests.util import mat_to_scipy, rel_err, sp_rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


def system(lib, nel, ngl, mask_kind):
    """(ctx, matrix id, A scipy, b, ids) of the KLE matrix on a box lattice of order ngl"""
    dim = len(nel)
    mesh = fo.box_mesh(nel, [0.0] * dim, [1.0] * dim, ngl)
    mask = boundary_mask(mesh)
    if mask_kind == "partial":
        mask = (np.random.default_rng(5).random((mesh.n_node, dim)) < 0.25).astype(np.uint8)
    ctx = make_ctx(lib, mesh, mask, dim, ngl=ngl)
    assert ctx.mesh_topology()[0] == "general" and ctx.mesh_ho_lattice()[0] == ngl
    M = ctx.mat_create(dim, dim)
    ctx.assemble_kle(1e3, 1e2, M)
    _, ids = mm.ho_lattice_of(mesh, nel, ngl)
    return ctx, M, mat_to_scipy(ctx, M, dim, dim), dim, ids


@pytest.mark.parametrize("mask_kind", ["faces", "partial"])
@pytest.mark.parametrize("nel,ngl", [([6, 4], 4), ([6, 4], 5), ([4, 4], 9), ([4, 2, 2], 4)])
def test_galerkin_levels(lib, nel, ngl, mask_kind):
    """every coarse level == P^T A P of the model (1e-12 relative); [6, 4] cells stop at the odd count after three levels"""
    ctx, M, A, b, ids = system(lib, nel, ngl, mask_kind)
    ctx.mg_setup(M, coarse_max_rows=20)
    info = ctx.mg_info(M)
    assert info["levels"] == mm.ho_level_count(nel, ngl, b, coarse_max_rows=20) >= 3 and info["rows"][0] == A.shape[0]
    ref = mm.ho_levels(A, ids, nel, ngl, b, info["levels"])
    for l in range(1, info["levels"]):
        Al, _, _, nl = ref[l]
        assert info["rows"][l] == Al.shape[0]
        S = ctx.mg_level_get(M, l, b)
        assert sp_rel_err(stencil_to_scipy(S, nl, b), Al) < 1e-12, l
    ctx.close()


def test_scalar_matrix_levels_and_vcycle(lib):
    """one DOF per node (the Laplacian on [5, 4] cells of ngl 6, faces imposed): levels == the model's (1e-12), V-cycle == numpy (1e-11)"""
    nel, ngl = [5, 4], 6
    mesh = fo.box_mesh(nel, [0.0] * 2, [1.0] * 2, ngl)
    ctx = make_ctx(lib, mesh, boundary_mask(mesh)[:, 0], 1, ngl=ngl)
    M = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, M)
    A = mat_to_scipy(ctx, M, 1, 1)
    _, ids = mm.ho_lattice_of(mesh, nel, ngl)
    ctx.mg_setup(M, coarse_max_rows=20)
    info = ctx.mg_info(M)
    assert info["rows"] == [A.shape[0], 30]
    levels = mm.ho_levels(A, ids, nel, ngl, 1, 2)
    assert sp_rel_err(stencil_to_scipy(ctx.mg_level_get(M, 1, 1), levels[1][3], 1), levels[1][0]) < 1e-12
    r = np.random.default_rng(4).standard_normal(A.shape[0])
    vr, vz = ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vr, r)
    ctx.mg_apply(M, vr, vz)
    assert rel_err(ctx.vec_get(vz, 1), numpy_vcycle(levels, info["lambda"], 2, r)) < 1e-11
    ctx.close()


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("nel,ngl", [([4, 4], 5), ([2, 2, 2], 4)])
def test_vcycle_matches_numpy(lib, nel, ngl, degree):
    """one V-cycle (mg_apply) == the model from mg_info's lambda estimates (1e-11); two calls return identical bits"""
    ctx, M, A, b, ids = system(lib, nel, ngl, "faces")
    ctx.mg_setup(M, coarse_max_rows=20, smooth_degree=degree)
    info = ctx.mg_info(M)
    assert info["levels"] == 3 and all(v > 0 for v in info["lambda"][:-1])
    levels = mm.ho_levels(A, ids, nel, ngl, b, info["levels"])
    r = np.random.default_rng(2).standard_normal(A.shape[0])
    vr, vz = ctx.vec_create(b), ctx.vec_create(b)
    ctx.vec_set(vr, r)
    ctx.mg_apply(M, vr, vz)
    z1 = ctx.vec_get(vz, b).copy()
    assert rel_err(z1, numpy_vcycle(levels, info["lambda"], degree, r)) < 1e-11
    ctx.vec_set(vz, np.zeros_like(r))
    ctx.mg_apply(M, vr, vz)
    assert np.array_equal(ctx.vec_get(vz, b), z1)
    ctx.close()


@pytest.mark.parametrize("nel,ngl", [([6, 4], 5), ([2, 2, 2], 4)])
def test_preconditioner_is_spd(lib, nel, ngl):
    """u' M^-1 v == v' M^-1 u, u' M^-1 u > 0; decoupled rows give r / a_ii"""
    ctx, M, A, b, ids = system(lib, nel, ngl, "faces")
    ctx.mg_setup(M, coarse_max_rows=20)
    n = A.shape[0]
    rng = np.random.default_rng(11)
    vecs = [ctx.vec_create(b) for _ in range(4)]
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    ctx.vec_set(vecs[0], u)
    ctx.vec_set(vecs[1], v)
    ctx.mg_apply(M, vecs[0], vecs[2])
    ctx.mg_apply(M, vecs[1], vecs[3])
    Mu, Mv = ctx.vec_get(vecs[2], b), ctx.vec_get(vecs[3], b)
    assert abs(u @ Mv - v @ Mu) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv)
    assert u @ Mu > 0 and v @ Mv > 0
    dec = decoupled(A)
    assert dec.any()
    assert np.array_equal(Mu[dec], u[dec] / A.diagonal()[dec])
    ctx.close()


def kle_system(lib, dim, nel, ngl, alpha=(1e3, 1e2)):
    """tests/test_gpu_mg.py::kle_system at order ngl: faces imposed, seeded right-hand side, zero on imposed rows"""
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    dom = DMPlexDom(boxMesh={"nelem": [nel] * dim, "lower": [0] * dim, "upper": [1] * dim})
    dom.setFemIndexing(ngl)
    ctx = dom.ctx
    for t in Spectral(ngl, dim).deviceTables():
        ctx.tables_set(*t)
    bm = dom.boundaryMaskLocal()
    ctx.bc_set(dim, np.repeat(bm[:, None], dim, axis=1))
    n_rows, _ = ctx.csr_symbolic()
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(*alpha, K)
    ctx.matfree_set(lib.MATFREE_KLE, *alpha)
    rhs = np.random.default_rng(0).standard_normal(n_rows * dim)
    rhs[np.repeat(bm != 0, dim)] = 0.0
    vb, vx = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vb, rhs)
    return dom, ctx, K, vb, vx, rhs


# (dim, cells per axis, ngl, factor f of the ratio check f * MG <= Jacobi)
CONVERGENCE = [(2, 8, 5, 4), (2, 32, 5, 10), (2, 8, 9, 4), (3, 4, 4, 2)]


@pytest.mark.parametrize("dim,nel,ngl,factor", CONVERGENCE)
def test_cg_mg_converges(lib, dim, nel, ngl, factor):
    """CG+MG (degree 2, coarse_max_rows 100) to rtol 1e-10 with the assembled product and with the shell: converged, true residual
    <= 1e-9, Jacobi-PCG's solution (1e-8), shell and assembled counts within 1, the count within max(3, 10 %) of the model's PCG run
    with mg_info's lambda, and factor * MG <= Jacobi (prototype with the exact lambda: 44 / 333 at 2-D 8^2 ngl 5, 83 / 1,347 at
    32^2, 103 / 817 at 8^2 ngl 9, 48 / 157 at 3-D 4^3 ngl 4).  Measured on an MI355X with the device's 10-step Lanczos lambda:
    44 / 333, 82 / 1,347, 103 / 817, 48 / 157, assembled and shell alike and equal to the model's count in every case."""
    dom, ctx, K, vb, vx, rhs = kle_system(lib, dim, nel, ngl)
    kw = dict(rtol=1e-10, atol=1e-300, maxit=200000, norm_type=lib.NORM_UNPRECONDITIONED)
    ij = ctx.solve(K, vb, vx, pc=lib.PC_JACOBI, **kw)
    xj = ctx.vec_get(vx, dim).copy()
    ctx.mg_setup(K, coarse_max_rows=100)
    info = ctx.mg_info(K)
    its = {}
    for name, mf in (("assembled", lib.MATFREE_OFF), ("shell", lib.MATFREE_KLE)):
        ctx.vec_set(vx, np.zeros_like(rhs))
        im = ctx.solve(K, vb, vx, pc=lib.PC_MG, matfree=mf, **kw)
        assert ij.reason == 2 and im.reason == 2, (name, ij.reason, im.reason)
        assert im.true_resid <= 1e-9, (name, im.true_resid)
        assert rel_err(ctx.vec_get(vx, dim), xj) < 1e-8, name
        its[name] = im.iters
    assert ctx.mg_info(K)["builds"] == info["builds"]
    A = mat_to_scipy(ctx, K, dim, dim)
    xyz = np.asarray(dom.xyz)[:, :dim]            # the coordinates handed to mesh_set: the context's numbering
    _, ids = mm.ho_lattice_of(types.SimpleNamespace(xyz=xyz, n_node=len(xyz)), [nel] * dim, ngl)
    levels = mm.ho_levels(A, ids, [nel] * dim, ngl, dim, info["levels"])
    assert info["rows"] == [l[0].shape[0] for l in levels]
    _, model = mm.mg_pcg(levels, info["lambda"], 2, rhs)
    print(f"{dim}-D {nel}^{dim} ngl {ngl}: Jacobi {ij.iters}, MG assembled {its['assembled']} shell {its['shell']}, model {model}, "
          f"levels {info['rows']}, lambda {info['lambda']}")
    assert abs(its["assembled"] - its["shell"]) <= 1, its
    for name, n in its.items():
        assert abs(n - model) <= max(3, 0.1 * model), (name, n, model)
        assert factor * n <= ij.iters, (name, n, ij.iters)
    ctx.close()


def test_hierarchy_cache(lib):
    """a second solve does not rebuild; new values (mat_zero + assembly with other alpha) do, and equal a fresh hierarchy"""
    dom, ctx, K, vb, vx, rhs = kle_system(lib, 2, 8, 4)
    kw = dict(pc=lib.PC_MG, rtol=1e-10, atol=1e-300, norm_type=lib.NORM_UNPRECONDITIONED)
    ctx.mg_setup(K, coarse_max_rows=100)
    i1 = ctx.solve(K, vb, vx, **kw)
    n0 = ctx.mg_info(K)["builds"]
    ctx.solve(K, vb, vx, **kw)
    assert ctx.mg_info(K)["builds"] == n0
    ctx.mg_setup(K, coarse_max_rows=100)               # same options, same values: no rebuild
    assert ctx.mg_info(K)["builds"] == n0
    ctx.mat_zero(K)
    ctx.assemble_kle(2e3, 3e2, K)
    i2 = ctx.solve(K, vb, vx, **kw)
    x2 = ctx.vec_get(vx, 2).copy()
    info = ctx.mg_info(K)
    assert info["builds"] == n0 + 1 and i2.reason == 2 and i1.reason == 2
    K2 = ctx.mat_create(2, 2)
    ctx.assemble_kle(2e3, 3e2, K2)
    ctx.mg_setup(K2, coarse_max_rows=100)
    info2 = ctx.mg_info(K2)
    assert info2["rows"] == info["rows"] and info["levels"] == 3
    # K and K2 come from two runs of the generic assembly, whose atomic sums agree to round-off only: as tests/test_gpu_mg.py
    assert np.allclose(info2["lambda"], info["lambda"], rtol=1e-10, atol=0)
    for l in range(1, info["levels"]):
        assert rel_err(ctx.mg_level_get(K, l, 2), ctx.mg_level_get(K2, l, 2)) < 1e-13
    i3 = ctx.solve(K2, vb, vx, **kw)
    assert abs(i3.iters - i2.iters) <= 1 and rel_err(ctx.vec_get(vx, 2), x2) < 1e-9
    ctx.close()


def test_builds_are_bit_identical(lib):
    """two builds of the same values give the same bits (no atomics, fixed summation order in the probing chain)"""
    ctx, M, A, b, ids = system(lib, [5, 3], 6, "partial")
    ctx.mg_setup(M, coarse_max_rows=20)
    S1 = ctx.mg_level_get(M, 1, b).copy()
    ctx.mg_setup(M, coarse_max_rows=20, smooth_degree=3)   # other options: a rebuild
    assert ctx.mg_info(M)["builds"] == 2
    assert np.array_equal(ctx.mg_level_get(M, 1, b), S1)
    ctx.close()


def test_refusals(lib):
    """each refusal raises with its message"""
    mesh = fo.box_mesh([4, 4], [0.0] * 2, [1.0] * 2, 4)
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), 2, ngl=4)
    K = ctx.mat_create(2, 2)
    ctx.assemble_kle(1e3, 1e2, K)
    ctx.mg_setup(K, coarse_max_rows=20)                     # accepted on one rank ...
    ctx.comm_init(0, 2, None)                               # ... refused with a detached second rank
    with pytest.raises(lib.PynamaHipError, match="one rank"):
        ctx.mg_setup(K, coarse_max_rows=10)
    ctx.close()
    mesh = fo.box_mesh([65, 65], [0.0] * 2, [1.0] * 2, 4)   # level 1 is 66^2 nodes = 8,712 rows, odd cell counts stop there
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), 2, ngl=4)
    K = ctx.mat_create(2, 2)
    ctx.assemble_kle(1e3, 1e2, K)
    with pytest.raises(lib.PynamaHipError, match="above the dense LU limit"):
        ctx.mg_setup(K)
    ctx.close()
    mesh = fo.box_mesh([2, 2], [0.0] * 2, [1.0] * 2, 13)    # above the shell's order limit: not a recognised lattice
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), 2, ngl=13)
    assert ctx.mesh_ho_lattice()[0] == 0
    K = ctx.mat_create(2, 2)
    ctx.assemble_kle(1e3, 1e2, K)
    with pytest.raises(lib.PynamaHipError, match="general connectivity"):
        ctx.mg_setup(K, coarse_max_rows=20)
    ctx.close()
    mesh = fo.box_mesh([4, 4], [0.0] * 2, [1.0] * 2, 4)     # an ngl 4 box whose node numbering is shuffled
    perm = np.random.default_rng(1).permutation(mesh.n_node)
    inv = np.argsort(perm)
    mesh.conn = inv[mesh.conn].astype(mesh.conn.dtype)
    mesh.xyz = mesh.xyz[perm]
    ctx = make_ctx(lib, mesh, None, 2, ngl=4)
    assert ctx.mesh_ho_lattice()[0] == 0
    K = ctx.mat_create(2, 2)
    ctx.assemble_kle(1e3, 1e2, K)
    with pytest.raises(lib.PynamaHipError, match="general connectivity"):
        ctx.mg_setup(K, coarse_max_rows=20)
    ctx.close()


def test_facade_solveKLE_taylor_green():
    """CustomFuncCase Taylor-Green, 8 x 8 cells of ngl 5, -ksp_type cg -pc_type mg with the ngl >= 4 shell (-pynama_mat_free_ho) and
    without it: converged, true residual <= 1e-10, at least three levels, and the velocity of the same run with -pc_type jacobi (1e-8)"""
    import pynama_amd
    from tests.test_gpu_api import setFemProblem
    from common.options import Options
    pynama_amd.install_reference_layout()
    tail = ["-ksp_rtol", "1e-12", "-ksp_norm_type", "unpreconditioned", "-pynama_mg_coarse_max_rows", "100"]
    vel = {}
    try:
        for pc, shell in (("mg", True), ("mg", False), ("jacobi", True)):
            Options(["-ksp_type", "cg", "-pc_type", pc] + tail + (["-pynama_mat_free_ho"] if shell else []))
            fem = setFemProblem('taylor-green', nelem=[8, 8], ngl=5)
            exactVel, exactVort = fem.generateExactVecs(0.0)
            fem.solveKLE(time=0.0, vort=exactVort)
            assert fem.solver.getConvergedReason() == 2
            assert fem.solver.info.true_resid <= 1e-10
            assert bool(fem.solver.shell_used) == shell
            if pc == "mg":
                A = fem.solver.mat
                assert A.ctx.mg_info(A.id)["levels"] >= 3
            vel[pc, shell] = fem.vel.getArray().copy()
    finally:
        Options([])
    ref = vel["jacobi", True]
    for shell in (True, False):
        assert np.abs(vel["mg", shell] - ref).max() <= 1e-8 * np.abs(ref).max(), shell
