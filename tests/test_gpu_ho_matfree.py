"""GPU parity of the matrix-free KLE operator on box lattices of affine cells at orders ngl >= 4 (pynama_amd/csrc/pyn_matfree_ho.hip):
pyn_matfree_set / pyn_matfree_apply(PYN_MATFREE_KLE) against the CPU oracle's K and the assembled K, the Dirichlet snapshot, the
refusals, rank slabs, Jacobi-PCG with the shell, ranks sharing one GPU, the opt-in facade flag -pynama_mat_free_ho and run-to-run
determinism.

Bar of the products: FP_TOL = 2e-13 with tests.util.rel_err.  Reference: a sum-factorised K_e x_e from the 1-D tables equals the
oracle's dense K_e x_e to <= 2.3e-15 per cell (numpy, ngl 4..12 in 2-D, 4..8 in 3-D; tests/test_ho_matfree_host.py repeats the
comparison with the library's own tables); the factor 100 covers the accumulation over a node's cells and the row sums of a whole mesh."""
import functools
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


@functools.lru_cache(maxsize=None)
def _tables(ngl, dim):
    return fo.Tables(ngl, dim)


_KE = {}


def _elem_K(mesh, ngl, alpha_d, alpha_w):
    """K_e of the mesh's cells: affine cells of one box are congruent, so cell 0's matrix serves them all"""
    c0 = np.ascontiguousarray(mesh.corners()[:1])
    key = (mesh.dim, ngl, alpha_d, alpha_w, c0.tobytes())
    if key not in _KE:
        _KE[key] = fo.elem_kle_matrices(_tables(ngl, mesh.dim), c0, alpha_d, alpha_w)[0][0]
    return _KE[key]


def oracle_K(mesh, ngl, mask, alpha_d, alpha_w):
    """K of assemble_kle_freeslip with a per-DOF mask [n_node, dim] (None: nothing imposed): imposed columns eliminated, imposed rows
    identity (tests/test_gpu_ho3_matfree.py: oracle_K, at order ngl)"""
    import scipy.sparse as sp
    dim = mesh.dim
    Ke = np.broadcast_to(_elem_K(mesh, ngl, alpha_d, alpha_w), (mesh.n_elem,) + (ngl ** dim * dim,) * 2)
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


def geometry(dim, nelem, kind, ngl):
    lo, up = [0.0] * dim, ([1.0, 0.8, 1.2][:dim] if kind == "stretched" else [1.0] * dim)
    mesh = fo.box_mesh(nelem, lo, up, ngl)
    if kind == "sheared":
        A = np.eye(dim) + 0.25 * np.random.default_rng(3).standard_normal((dim, dim))
        assert np.linalg.det(A) > 0
        mesh.xyz = mesh.xyz @ A.T + 0.3
    return mesh


def masks(mesh):
    dim, n = mesh.dim, mesh.n_node
    per_dof = np.zeros((n, dim), np.uint8)
    per_dof[mesh.boundary, 0] = 1
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


# one cell, fewer cells than one workgroup takes, several workgroups, odd remainders (cells per workgroup: 2-D ngl 4: 16, 5: 10, 8: 4,
# 12: 1; 3-D ngl 4: 4, 5: 2, 6: 1)
ORACLE_CASES = [(2, 4, [1, 1]), (2, 4, [5, 2]), (2, 4, [7, 5]), (2, 5, [1, 1]), (2, 5, [3, 3]), (2, 5, [6, 5]), (2, 8, [1, 1]),
                (2, 8, [3, 2]), (2, 8, [5, 3]), (2, 12, [1, 1]), (2, 12, [3, 2]),
                (3, 4, [1, 1, 1]), (3, 4, [3, 2, 3]), (3, 4, [2, 2, 2]), (3, 5, [1, 1, 1]), (3, 5, [2, 3, 2]), (3, 5, [3, 1, 1]),
                (3, 6, [1, 1, 1]), (3, 6, [2, 2, 3])]


@pytest.mark.parametrize("dim,ngl,nelem", ORACLE_CASES)
@pytest.mark.parametrize("kind", ["unit", "stretched", "sheared"])
def test_shell_equals_oracle_and_assembled(lib, dim, ngl, nelem, kind):
    """matfree_apply == oracle K x == spmv(K) x: axis-aligned and sheared cells, every kind of mask, penalty weights on and off"""
    mesh = geometry(dim, nelem, kind, ngl)
    x = np.random.default_rng(1).standard_normal(mesh.n_node * dim)
    for name, mask in masks(mesh).items():
        for alpha_d, alpha_w in ((1e3, 1e2), (0.0, 0.0)):
            ctx = make_ctx(lib, mesh, mask, dim, ngl=ngl)
            assert ctx.mesh_topology()[0] == "general"
            assert ctx.mesh_ho_lattice()[0] == ngl
            _, y, ya = shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w)
            yo = oracle_K(mesh, ngl, mask, alpha_d, alpha_w) @ x
            eo, ea = rel_err(y, yo), rel_err(y, ya)
            print(f"dim {dim} ngl {ngl} {nelem} {kind} {name} alpha_d {alpha_d}: vs oracle {eo:.3e} vs assembled {ea:.3e}")
            assert eo < FP_TOL, (name, alpha_d, eo)
            assert ea < FP_TOL, (name, alpha_d, ea)
            ctx.close()


ASSEMBLED_CASES = [(2, n, [3, 2]) for n in range(4, 13)] + [(3, n, [2, 1, 2]) for n in range(4, 8)] + [(3, 8, [1, 1, 1]), (3, 8, [2, 2, 1])]


@pytest.mark.parametrize("dim,ngl,nelem", ASSEMBLED_CASES)
def test_shell_equals_assembled_every_order(lib, dim, ngl, nelem):
    """every supported order against spmv of the assembled K (the oracle is too slow at 3-D ngl 7, 8): stretched and sheared cells,
    boundary and random masks, penalties on and off"""
    for kind in ("stretched", "sheared"):
        mesh = geometry(dim, nelem, kind, ngl)
        x = np.random.default_rng(1).standard_normal(mesh.n_node * dim)
        mk = masks(mesh)
        for name in ("boundary", "random"):
            for alpha_d, alpha_w in ((1e3, 1e2), (0.0, 0.0)):
                ctx = make_ctx(lib, mesh, mk[name], dim, ngl=ngl)
                _, y, ya = shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w)
                ea = rel_err(y, ya)
                print(f"dim {dim} ngl {ngl} {nelem} {kind} {name} alpha_d {alpha_d}: vs assembled {ea:.3e}")
                assert ea < FP_TOL, (kind, name, alpha_d, ea)
                ctx.close()


@pytest.mark.parametrize("dim,ngl", [(2, 5), (3, 4)])
def test_mask_is_a_snapshot(lib, dim, ngl):
    """a bc_set after matfree_set leaves the shell alone; matfree_set again takes the new mask; a second assembly with another mask
    on the same context gives a shell equal to the second K"""
    mesh = geometry(dim, [4, 3] if dim == 2 else [2, 3, 2], "stretched", ngl)
    m0 = boundary_mask(mesh)
    m1 = masks(mesh)["random"]
    ctx = make_ctx(lib, mesh, m0, dim, ngl=ngl)
    x = np.random.default_rng(4).standard_normal(mesh.n_node * dim)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    vx, vy, va = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.bc_set(dim, m1)
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    assert rel_err(ctx.vec_get(vy, dim), oracle_K(mesh, ngl, m0, 1e3, 1e2) @ x) < FP_TOL
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    assert rel_err(ctx.vec_get(vy, dim), oracle_K(mesh, ngl, m1, 1e3, 1e2) @ x) < FP_TOL
    # two assemblies on one context, each followed by its own snapshot (what Mat.assembleKLE does)
    for m in (m0, m1):
        ctx.bc_set(dim, m)
        K = ctx.mat_create(dim, dim)
        ctx.assemble_kle(1e3, 1e2, K)
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
        ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
        ctx.spmv(K, vx, va)
        assert rel_err(ctx.vec_get(vy, dim), ctx.vec_get(va, dim)) < FP_TOL
        assert rel_err(ctx.vec_get(vy, dim), oracle_K(mesh, ngl, m, 1e3, 1e2) @ x) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals(lib, dim):
    """the Laplacian, vectors of the wrong block size, a bent (non-affine) cell, a renumbered connectivity and an order above the
    limit are refused with a message; mesh_topology keeps saying "general" """
    ngl = 4
    mesh = geometry(dim, [3, 2] if dim == 2 else [2, 2, 2], "unit", ngl)
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), dim, ngl=ngl)
    assert ctx.mesh_topology()[0] == "general"
    with pytest.raises(lib.PynamaHipError, match="KLE operator only"):
        ctx.matfree_set(lib.MATFREE_LAPLACE)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    wrong = 3 if dim == 2 else 2
    vx, vy = ctx.vec_create(wrong), ctx.vec_create(wrong)
    with pytest.raises(lib.PynamaHipError, match="block size"):
        ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    ctx.close()
    # one interior vertex moved: the cells around it are no parallelograms / parallelepipeds
    bent = geometry(dim, [3, 2] if dim == 2 else [2, 2, 2], "unit", ngl)
    inner = np.setdiff1d(np.unique(bent.conn[:, :2 ** dim]), bent.boundary)
    bent.xyz[inner[len(inner) // 2]] += 0.02
    ctx = make_ctx(lib, bent, boundary_mask(bent), dim, ngl=ngl)
    with pytest.raises(lib.PynamaHipError, match="affine"):
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.close()
    # renumbered nodes (what an imported mesh looks like): not the lexicographic lattice
    perm = np.random.default_rng(1).permutation(mesh.n_node)
    ren = geometry(dim, [3, 2] if dim == 2 else [2, 2, 2], "unit", ngl)
    ren.conn = perm[ren.conn].astype(np.int32)
    ren.xyz = ren.xyz[np.argsort(perm)]
    ctx = make_ctx(lib, ren, None, dim, ngl=ngl)
    assert ctx.mesh_ho_lattice()[0] == 0
    with pytest.raises(lib.PynamaHipError, match="imported / renumbered"):
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.close()
    # one order above the limit
    big = 13 if dim == 2 else 9
    mesh = fo.box_mesh([1] * dim, [0.0] * dim, [1.0] * dim, big)
    ctx = make_ctx(lib, mesh, None, dim, ngl=big)
    assert ctx.mesh_topology()[0] == "general"
    with pytest.raises(lib.PynamaHipError, match=f"ngl {big} is above the limit.*ngl <= {big - 1}"):
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.close()


@pytest.mark.parametrize("nelem,size,ngl", [([3, 6], 2, 5), ([2, 7], 3, 4), ([2, 2, 4], 2, 4), ([2, 1, 5], 3, 5)])
def test_rank_slabs(lib, nelem, size, ngl):
    """a rank's slab (detached context, ghost planes with the last ids): the owned rows of the shell equal the serial oracle rows"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    dim = len(nelem)
    lo, up = [0.0] * dim, [1.0, 0.8, 1.2][:dim]
    glob = fo.box_mesh(nelem, lo, up, ngl)
    xg = np.random.default_rng(11).standard_normal(glob.n_node * dim)
    yg = oracle_K(glob, ngl, boundary_mask(glob), 1e3, 1e2) @ xg
    for r in range(size):
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': lo, 'upper': up}, comm=Comm(r, size))
        dom.setFemIndexing(ngl)
        ctx = lib.Context(0)
        ctx.comm_init(r, size, None)                      # detached
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(dim, dom.conn, dom.xyz)
        for t in Spectral(ngl, dim).deviceTables():
            ctx.tables_set(*t)
        ctx.bc_set(dim, np.repeat(dom.boundaryMaskLocal()[:, None], dim, axis=1))
        ctx.csr_symbolic()
        assert ctx.mesh_topology()[0] == "general" and ctx.mesh_ho_lattice()[0] == ngl
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
        l2g = dom._local2global(np.arange(dom.nLocal))
        rows = (np.arange(dom.rStart, dom.rEnd)[:, None] * dim + np.arange(dim)).ravel()
        cv = (l2g[:, None] * dim + np.arange(dim)).ravel()
        vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
        ctx.vec_set_local(vx, xg[cv])
        ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
        err = rel_err(ctx.vec_get(vy, dim), yg[rows])
        print(f"{nelem} ngl {ngl} rank {r}/{size}: {err:.3e}")
        assert err < FP_TOL, r
        ctx.close()


@pytest.mark.parametrize("dim,ngl,nelem", [(2, 5, [16, 16]), (3, 4, [6, 6, 6])])
def test_krylov_with_the_shell(lib, dim, ngl, nelem):
    """Jacobi-PCG with the shell and with the assembled product on the same system: rtol 1e-10, iteration counts within +-1, true
    residual against the assembled matrix <= 1e-10; the guard trips when K is edited after the snapshot"""
    mesh = geometry(dim, nelem, "stretched", ngl)
    mask = boundary_mask(mesh)
    ctx = make_ctx(lib, mesh, mask, dim, ngl=ngl)
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(1e3, 1e2, K)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    b = np.random.default_rng(2).standard_normal(mesh.n_node * dim)
    b[mask.reshape(-1).astype(bool)] = 0.0
    vb, vx = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vb, b)
    kw = dict(method=lib.KSP_CG, pc=lib.PC_JACOBI, rtol=1e-10, atol=1e-300, maxit=100000, norm_type=lib.NORM_UNPRECONDITIONED)
    ctx.vec_set(vx, np.zeros_like(b))
    ia = ctx.solve(K, vb, vx, **kw)
    xa = ctx.vec_get(vx, dim)
    ctx.vec_set(vx, np.zeros_like(b))
    im = ctx.solve(K, vb, vx, matfree=lib.MATFREE_KLE, **kw)
    xm = ctx.vec_get(vx, dim)
    print(f"dim {dim} ngl {ngl}: iters assembled {ia.iters} shell {im.iters}, true_resid {im.true_resid:.3e}, x diff {rel_err(xm, xa):.3e}")
    assert ia.reason > 0 and im.reason > 0, (ia.reason, im.reason)
    assert abs(ia.iters - im.iters) <= 1, (ia.iters, im.iters)
    assert im.true_resid <= 1e-10, im.true_resid
    assert rel_err(xm, xa) < 1e-7
    # K edited after the snapshot (a free DOF, where b is not zero): the shell no longer is this matrix
    free = np.nonzero(~mask.reshape(-1).astype(bool))[0]
    d = int(free[len(free) // 2])
    ctx.mat_add_values(K, np.array([d], np.int32), np.array([d], np.int32), np.array([1.0e3]), insert=False)
    with pytest.raises(lib.PynamaHipError, match="matrix-free operator differs"):
        ctx.solve(K, vb, vx, matfree=lib.MATFREE_KLE, **kw)
    ctx.close()


@pytest.mark.parametrize("size,nelem,ngl", [(2, "3,6", 5), (3, "2,2,7", 4)])
def test_ranks_sharing_one_gpu(size, nelem, ngl):
    """one KLE solve per rank over the shared-memory transport (single-reduction CG, blocking exchange): assembled and shell"""
    from pynama_amd import _lib
    cap = 4 << 20
    with tempfile.NamedTemporaryFile(dir="/dev/shm" if os.path.isdir("/dev/shm") else None, prefix="pynama_shm_") as f:
        f.truncate(_lib.Context.shm_size(size, cap))
        f.flush()
        env = dict(os.environ, PYNAMA_SHM_CAP=str(cap))
        worker = os.path.join(ROOT, "tests", "ho_matfree_dist_worker.py")
        procs = [subprocess.Popen(["timeout", "-k", "10", "280", sys.executable, worker, str(r), str(size), f.name, nelem, str(ngl)],
                                  env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(size)]
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=300)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                pytest.fail("distributed GPU worker timed out")
        print("".join(outs))
        assert all(p.returncode == 0 for p in procs), "\n".join(outs)


def _facade_run(mode, tmp_path):
    out = str(tmp_path / f"tg_{mode}.npz")
    worker = os.path.join(ROOT, "tests", "ho_matfree_facade_worker.py")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, worker, mode, out], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return np.load(out)


def test_facade_flag(tmp_path):
    """-pynama_mat_free_ho: Mat.assembleKLE tags K at ngl 5 and the Taylor-Green solve takes the shell; without the option K stays
    untagged; both runs give the same velocity.  Each run in a fresh child process under its own time limit."""
    off = _facade_run("off", tmp_path)
    assert not bool(off["tagged"]) and not bool(off["shell_used"]) and str(off["topo"]) == "general"
    on = _facade_run("on", tmp_path)          # (sequential: the second child starts only after the first ended well)
    assert bool(on["tagged"]) and bool(on["shell_used"]) and str(on["topo"]) == "general"
    print(f"facade: err off {float(off['err']):.3e} on {float(on['err']):.3e} diff {rel_err(on['vel'], off['vel']):.3e}")
    assert rel_err(on["vel"], off["vel"]) < 1e-9


@pytest.mark.parametrize("dim,ngl,nelem", [(2, 5, [9, 7]), (2, 12, [3, 2]), (3, 4, [3, 3, 3]), (3, 8, [2, 1, 1])])
def test_two_applications_are_bit_identical(lib, dim, ngl, nelem):
    mesh = geometry(dim, nelem, "sheared", ngl)
    ctx = make_ctx(lib, mesh, masks(mesh)["per_dof"], dim, ngl=ngl)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    x = np.random.default_rng(8).standard_normal(mesh.n_node * dim)
    vx, vy, vz = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.vec_set(vy, np.full_like(x, np.nan))              # no pre-zeroed y: every owned row is written
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE)
    ctx.matfree_apply(vx, vz, lib.MATFREE_KLE)
    y, z = ctx.vec_get(vy, dim), ctx.vec_get(vz, dim)
    assert np.all(np.isfinite(y)) and np.array_equal(y, z)
    ctx.close()
