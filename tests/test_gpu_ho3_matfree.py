"""GPU parity of the matrix-free KLE operator on second-order (ngl = 3) structured meshes of affine cells
(pynama_amd/csrc/pyn_matfree_ho3.hip): pyn_matfree_set / pyn_matfree_apply(PYN_MATFREE_KLE) against the CPU oracle's K and the
assembled K, the Dirichlet snapshot, the refusals, rank slabs, the Krylov solvers with the shell, ranks sharing one GPU and the
opt-in facade flag -pynama_mat_free_ngl3."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.test_gpu_ho3 import boundary_mask, make_ctx
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP_TOL = 2e-13


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


def oracle_K(mesh, mask, alpha_d, alpha_w):
    """K of assemble_kle_freeslip with a per-DOF mask [n_node, dim] (None: nothing imposed): imposed columns eliminated, imposed rows
    identity"""
    import scipy.sparse as sp
    dim = mesh.dim
    Ke, _, _ = fo.elem_kle_matrices(fo.Tables(3, dim), mesh.corners(), alpha_d, alpha_w)
    n = mesh.n_node
    vdof = fo.dof_indices(mesh.conn, dim)
    is_bc = np.zeros(n * dim, bool) if mask is None else np.asarray(mask, bool).reshape(-1)
    rfree = ~is_bc[vdof]
    R = np.broadcast_to(vdof[:, :, None], Ke.shape)
    C = np.broadcast_to(vdof[:, None, :], Ke.shape)
    mff = rfree[:, :, None] & rfree[:, None, :]
    K = fo._scatter((n * dim, n * dim), R[mff], C[mff], Ke[mff])
    bc_idx = np.nonzero(is_bc)[0]
    return (K + sp.coo_matrix((np.ones(len(bc_idx)), (bc_idx, bc_idx)), shape=K.shape)).tocsr()


def geometry(dim, nelem, kind):
    lo, up = [0.0] * dim, ([1.0, 0.8, 1.2][:dim] if kind == "stretched" else [1.0] * dim)
    mesh = fo.box_mesh(nelem, lo, up, 3)
    if kind == "sheared":
        A = np.eye(dim) + 0.25 * np.random.default_rng(3).standard_normal((dim, dim))
        assert np.linalg.det(A) > 0
        mesh.xyz = mesh.xyz @ A.T + 0.3
    return mesh


def masks(mesh):
    dim, n = mesh.dim, mesh.n_node
    per_dof = np.zeros((n, dim), np.uint8)
    per_dof[mesh.boundary, 0] = 1                              # one component imposed on the boundary (free-slip like)
    rnd = (np.random.default_rng(7).random((n, dim)) < 0.3).astype(np.uint8)
    return {"none": None, "boundary": boundary_mask(mesh), "per_dof": per_dof, "random": rnd}


def shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w):
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(alpha_d, alpha_w, K)
    ctx.matfree_set(lib.MATFREE_KLE, alpha_d, alpha_w)
    vx, vy, va = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    ctx.spmv(K, vx, va)
    return K, ctx.vec_get(vy, dim), ctx.vec_get(va, dim)


@pytest.mark.parametrize("dim,nelem", [(2, [1, 1]), (2, [5, 4]), (2, [16, 7]), (2, [33, 2]), (3, [1, 1, 1]), (3, [3, 2, 3]),
                                       (3, [4, 4, 4]), (3, [7, 2, 5]), (3, [12, 3, 2])])
@pytest.mark.parametrize("kind", ["unit", "stretched", "sheared"])
def test_shell_equals_oracle_and_assembled(lib, dim, nelem, kind):
    """matfree_apply == oracle K x == spmv(K) x: odd / even cell counts (several tiles and a single cell), axis-aligned (diagonal
    J^-1 forms) and sheared cells, every kind of mask, penalty weights on and off"""
    mesh = geometry(dim, nelem, kind)
    x = np.random.default_rng(1).standard_normal(mesh.n_node * dim)
    for name, mask in masks(mesh).items():
        for alpha_d, alpha_w in ((1e3, 1e2), (0.0, 0.0)):
            ctx = make_ctx(lib, mesh, mask, dim)
            assert ctx.mesh_topology()[0] == "lattice-ngl3"
            _, y, ya = shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w)
            yo = oracle_K(mesh, mask, alpha_d, alpha_w) @ x
            assert rel_err(y, yo) < FP_TOL, (name, alpha_d)
            assert rel_err(y, ya) < FP_TOL, (name, alpha_d)
            ctx.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_mask_is_a_snapshot(lib, dim):
    """a bc_set after matfree_set leaves the shell alone; matfree_set again takes the new mask"""
    mesh = geometry(dim, [6, 5] if dim == 2 else [3, 4, 2], "stretched")
    m0 = boundary_mask(mesh)
    m1 = masks(mesh)["random"]
    ctx = make_ctx(lib, mesh, m0, dim)
    x = np.random.default_rng(4).standard_normal(mesh.n_node * dim)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.bc_set(dim, m1)
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    assert rel_err(ctx.vec_get(vy, dim), oracle_K(mesh, m0, 1e3, 1e2) @ x) < FP_TOL
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    assert rel_err(ctx.vec_get(vy, dim), oracle_K(mesh, m1, 1e3, 1e2) @ x) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals(lib, dim):
    """a bent (non-affine) cell, the Laplacian at ngl 3 and vectors of the wrong block size are refused with a message"""
    mesh = geometry(dim, [5, 4] if dim == 2 else [3, 2, 3], "unit")
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), dim)
    with pytest.raises(lib.PynamaHipError, match="KLE operator only"):
        ctx.matfree_set(lib.MATFREE_LAPLACE)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    wrong = 3 if dim == 2 else 2
    vx, vy = ctx.vec_create(wrong), ctx.vec_create(wrong)
    with pytest.raises(lib.PynamaHipError, match="block size"):
        ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    ctx.close()
    corner_nodes = np.unique(mesh.conn[:, :2 ** dim])
    inner = np.setdiff1d(corner_nodes, mesh.boundary)
    mesh.xyz[inner[len(inner) // 2]] += 0.02
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), dim)
    with pytest.raises(lib.PynamaHipError, match="affine"):
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.close()


@pytest.mark.parametrize("nelem,size", [([5, 8], 2), ([4, 9], 3), ([3, 2, 6], 2), ([2, 3, 7], 3)])
def test_rank_slabs(lib, nelem, size):
    """a rank's slab (detached context, ghost planes with the last ids): the owned rows of the shell equal the serial oracle rows"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    dim = len(nelem)
    lo, up = [0.0] * dim, [1.0, 0.8, 1.2][:dim]
    glob = fo.box_mesh(nelem, lo, up, 3)
    xg = np.random.default_rng(11).standard_normal(glob.n_node * dim)
    yg = oracle_K(glob, boundary_mask(glob), 1e3, 1e2) @ xg
    for r in range(size):
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': lo, 'upper': up}, comm=Comm(r, size))
        dom.setFemIndexing(3)
        ctx = lib.Context(0)
        ctx.comm_init(r, size, None)                      # detached
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(dim, dom.conn, dom.xyz)
        for t in Spectral(3, dim).deviceTables():
            ctx.tables_set(*t)
        ctx.bc_set(dim, np.repeat(dom.boundaryMaskLocal()[:, None], dim, axis=1))
        ctx.csr_symbolic()
        assert ctx.mesh_topology()[0] == "lattice-ngl3"
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
        l2g = dom._local2global(np.arange(dom.nLocal))
        rows = (np.arange(dom.rStart, dom.rEnd)[:, None] * dim + np.arange(dim)).ravel()
        cv = (l2g[:, None] * dim + np.arange(dim)).ravel()
        vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
        ctx.vec_set_local(vx, xg[cv])
        ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
        assert rel_err(ctx.vec_get(vy, dim), yg[rows]) < FP_TOL, r
        ctx.close()


@pytest.mark.parametrize("dim,nelem,kind", [(2, [12, 9], "stretched"), (2, [8, 8], "sheared"), (3, [5, 4, 4], "unit"),
                                            (3, [4, 3, 4], "sheared")])
def test_krylov_with_the_shell(lib, dim, nelem, kind):
    """CG and GMRES with the shell follow the assembled solves; a shell of other weights is refused before the iteration"""
    mesh = geometry(dim, nelem, kind)
    mask = boundary_mask(mesh)
    ctx = make_ctx(lib, mesh, mask, dim)
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(1e3, 1e2, K)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    b = np.random.default_rng(2).standard_normal(mesh.n_node * dim)
    b[mask.reshape(-1).astype(bool)] = 0.0
    vb, vx = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vb, b)
    kw = dict(rtol=1e-10, atol=1e-300, maxit=100000, norm_type=lib.NORM_UNPRECONDITIONED)
    for method in (lib.KSP_CG, lib.KSP_GMRES):
        ctx.vec_set(vx, np.zeros_like(b))
        ia = ctx.solve(K, vb, vx, method=method, **kw)
        xa = ctx.vec_get(vx, dim)
        ctx.vec_set(vx, np.zeros_like(b))
        im = ctx.solve(K, vb, vx, method=method, matfree=lib.MATFREE_KLE, **kw)
        xm = ctx.vec_get(vx, dim)
        assert ia.reason > 0 and im.reason > 0, (method, ia.reason, im.reason)
        assert abs(ia.iters - im.iters) <= 2, (method, ia.iters, im.iters)
        assert rel_err(xm, xa) < 1e-9, method
        assert im.true_resid <= 1e-10, (method, im.true_resid)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 3e2)
    with pytest.raises(lib.PynamaHipError, match="matrix-free operator differs"):
        ctx.solve(K, vb, vx, matfree=lib.MATFREE_KLE, **kw)
    ctx.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_uniform_flow_solve_with_the_shell(lib, dim):
    """the reference's uniform-flow assertion (test_gpu_ho3.test_uniform_flow_solve) with Jacobi-PCG multiplying with the shell"""
    nelem = [10, 10] if dim == 2 else [3, 3, 3]
    mesh = fo.box_mesh(nelem, [0.0] * dim, [1.0] * dim, 3)
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), dim)
    dw = 1 if dim == 2 else 3
    K, Krhs, Rw = ctx.mat_create(dim, dim), ctx.mat_create(dim, dim), ctx.mat_create(dim, dw)
    ctx.assemble_kle(1e3, 1e2, K, Krhs, Rw, -1)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    cte = np.array([1.0, 4.0, -2.0][:dim])
    vel = np.zeros((mesh.n_node, dim))
    vel[mesh.boundary] = cte
    vv, vr, vx = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vv, vel.ravel())
    ctx.spmv(Krhs, vv, vr)
    info = ctx.solve(K, vr, vx, rtol=1e-14, atol=1e-300, dtol=1e8, norm_type=lib.NORM_UNPRECONDITIONED, maxit=200000,
                     matfree=lib.MATFREE_KLE)
    err = np.linalg.norm(ctx.vec_get(vx, dim) - np.tile(cte, mesh.n_node))
    assert err < 5e-12, (err, info.iters, info.reason)
    ctx.close()


@pytest.mark.parametrize("size,nelem", [(2, "6,9"), (3, "5,13"), (2, "3,4,7"), (3, "3,2,9")])
def test_ranks_sharing_one_gpu(size, nelem):
    """one ngl 3 KLE solve per rank over the shared-memory transport (single-reduction CG, blocking exchange): assembled and shell"""
    from pynama_amd import _lib
    cap = 4 << 20
    with tempfile.NamedTemporaryFile(dir="/dev/shm" if os.path.isdir("/dev/shm") else None, prefix="pynama_shm_") as f:
        f.truncate(_lib.Context.shm_size(size, cap))
        f.flush()
        env = dict(os.environ, PYNAMA_SHM_CAP=str(cap))
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ho3_matfree_dist_worker.py"), str(r), str(size), f.name,
                                   nelem], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(size)]
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=280)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                pytest.fail("distributed GPU worker timed out")
        assert all(p.returncode == 0 for p in procs), "\n".join(outs)


def _set_fem(case, **kw):
    import yaml
    import pynama_amd
    pynama_amd.install_reference_layout()
    from cases.uniform import UniformFlow
    with open(os.path.join(os.path.dirname(pynama_amd.__file__), "cases", f"{case}.yaml")) as f:
        data = yaml.load(f, Loader=yaml.Loader)
    fem = UniformFlow(data, case=case, **kw)
    fem.setUp()
    fem.setUpSolver()
    return fem


def test_facade_flag(monkeypatch):
    """-pynama_mat_free_ngl3: Mat.assembleKLE tags K on second-order lattices and the solves take the shell (2-D 10 x 10 and 3-D
    3 x 3 x 3 uniform flow, the reference's bars); -pynama_mat_free 0 keeps the assembled product; a non-affine mesh (one vertex
    moved: the box generator jitters first-order meshes only) stays untagged, and asking for the shell there still raises"""
    import pynama_amd
    pynama_amd.install_reference_layout()
    from common.options import Options
    from pynama_amd.domain.dmplex import DMPlexDom
    try:
        for kw, bar in (({}, 1e-12), (dict(lower=[0, 0, 0], upper=[1, 1, 1], nelem=[3, 3, 3], ngl=3), 2e-13)):
            for extra in ([], ["-pynama_mat_free"]):
                Options(["-pynama_mat_free_ngl3"] + extra)
                fem = _set_fem('uniform', **kw)
                assert fem.mat.K.matfree is not None
                exactVel, exactVort = fem.generateExactVecs()
                fem.solveKLE(time=0.0, vort=exactVort)
                assert fem.solver.shell_used
                # default preonly / lu: the direct solve (the reference's bar); -pynama_mat_free: Jacobi-PCG with the shell to round-off
                assert (exactVel - fem.vel).norm(norm_type=2) < (bar if not extra else 5e-12), extra
            Options(["-pynama_mat_free_ngl3", "-pynama_mat_free", "0", "-ksp_type", "cg", "-pc_type", "jacobi", "-ksp_rtol", "1e-14"])
            fem = _set_fem('uniform', **kw)
            exactVel, exactVort = fem.generateExactVecs()
            fem.solveKLE(time=0.0, vort=exactVort)
            assert fem.mat.K.matfree is not None and not fem.solver.shell_used
            assert (exactVel - fem.vel).norm(norm_type=2) < 1e-10
        lattice_coordinates = DMPlexDom._lattice_coordinates

        def bent(dom):                                  # the vertex at lattice point (10, 10) of the 10 x 10 cell box moves
            xyz = lattice_coordinates(dom)
            at = np.all([dom._lat_idx[d] == 10 for d in range(dom.dim)], axis=0)
            assert at.sum() == 1
            xyz[at] += 0.01
            return xyz

        monkeypatch.setattr(DMPlexDom, "_lattice_coordinates", bent)
        monkeypatch.setenv("PYNAMA_HOST_MESH", "1")     # the host coordinates, not the device box generator
        Options(["-pynama_mat_free_ngl3"])
        fem = _set_fem('uniform')
        assert fem.mat.K.matfree is None
        Options(["-pynama_mat_free_ngl3", "-pynama_mat_free"])
        fem = _set_fem('uniform')
        with pytest.raises(ValueError, match="no matrix-free form"):
            fem.solveKLE(time=0.0, vort=fem.generateExactVecs()[1])
    finally:
        Options([])
