"""GPU parity of the general matrix-free KLE operator PYN_MATFREE_KLE_GENERAL (pynama_amd/csrc/pyn_matfree_ho_general.hip): any
quadrilateral / hexahedral mesh of order ngl 4..12 (2-D) / 4..8 (3-D) -- bent cells, random numbering, cell order and cell orientation,
vertices of valence 3 and 5 -- against the CPU oracle's K (one K_e per cell) and the assembled K; the two operator ids side by side on
an affine lattice, the refusals, Jacobi-PCG with the shell, run-to-run determinism and the opt-in facade flag
-pynama_mat_free_ho_general on Gmsh files.

Bars: those of tests/test_gpu_ho_matfree.py.  FP_TOL = 2e-13 with tests.util.rel_err for the products: the numpy model of the kernel
(pointwise J from the corners, the library's own tables) equals the oracle's dense K_e x_e to <= 1e-14 per cell on bent and rotated
cells (tests/test_ho_matfree_general_host.py), which leaves a factor 20 for the accumulation over a node's cells and the row sums."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import ho_general_meshes as gm
from tests.test_gpu_ho3 import make_ctx
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP_TOL = 2e-13
ALPHAS = ((1e3, 1e2), (0.0, 0.0))


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


def build(kind, dim, ngl, nelem):
    return gm.bent_lattice(dim, nelem, ngl, seed=3) if kind == "bent" else gm.imported(dim, nelem, ngl)


def shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w):
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(alpha_d, alpha_w, K)
    ctx.matfree_set(lib.MATFREE_KLE_GENERAL, alpha_d, alpha_w)
    vx, vy, va = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE_GENERAL)
    ctx.spmv(K, vx, va)
    return K, ctx.vec_get(vy, dim), ctx.vec_get(va, dim)


def check_products(lib, mesh, mask_names, tag, oracle=True):
    dim, ngl = mesh.dim, mesh.ngl
    x = np.random.default_rng(1).standard_normal(mesh.n_node * dim)
    mk = gm.masks(mesh)
    for alpha_d, alpha_w in ALPHAS:                       # (outer: the oracle's element matrices are cached per penalty pair)
        for name in mask_names:
            ctx = make_ctx(lib, mesh, mk[name], dim, ngl=ngl)
            assert ctx.mesh_topology()[0] == "general"
            _, y, ya = shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w)
            ea = rel_err(y, ya)
            eo = rel_err(y, gm.oracle_K(mesh, mk[name], alpha_d, alpha_w) @ x) if oracle else 0.0
            print(f"{tag} {name} alpha_d {alpha_d}: vs oracle {eo:.3e} vs assembled {ea:.3e}")
            assert eo < FP_TOL, (name, alpha_d, eo)
            assert ea < FP_TOL, (name, alpha_d, ea)
            ctx.close()


# one cell, fewer cells than one workgroup takes, several workgroups with a remainder, several groups per workgroup (cells per
# workgroup: 2-D ngl 4: 16, 5: 10, 8: 4, 12: 1; 3-D ngl 4: 4, 5: 2, 6: 1)
ORACLE_CASES = [(2, 4, [1, 1]), (2, 4, [5, 2]), (2, 4, [7, 5]), (2, 5, [3, 3]), (2, 5, [6, 5]), (2, 8, [3, 2]), (2, 12, [3, 2]),
                (3, 4, [1, 1, 1]), (3, 4, [3, 2, 3]), (3, 5, [2, 3, 2]), (3, 5, [3, 1, 1]), (3, 6, [2, 2, 3])]


@pytest.mark.parametrize("dim,ngl,nelem", ORACLE_CASES)
@pytest.mark.parametrize("kind", ["bent", "imported"])
def test_shell_equals_oracle_and_assembled(lib, dim, ngl, nelem, kind):
    """matfree_apply == oracle K x == spmv(K) x on bent lattices and on imported meshes: every kind of mask, penalties on and off"""
    mesh = build(kind, dim, ngl, nelem)
    if kind == "imported":
        ctx = make_ctx(lib, mesh, None, dim, ngl=ngl)
        assert ctx.mesh_ho_lattice()[0] == 0               # no box lattice: what the affine shell refuses
        ctx.close()
    check_products(lib, mesh, ("none", "boundary", "per_dof", "random"), f"dim {dim} ngl {ngl} {nelem} {kind}")


ASSEMBLED_CASES = [(2, n, [3, 2]) for n in range(4, 13)] + [(3, n, [2, 1, 2]) for n in range(4, 8)] + [(3, 8, [1, 1, 1]), (3, 8, [2, 2, 1])]


@pytest.mark.parametrize("dim,ngl,nelem", ASSEMBLED_CASES)
def test_shell_equals_assembled_every_order(lib, dim, ngl, nelem):
    """every supported order against spmv of the assembled K (the oracle is too slow at 3-D ngl 7, 8) on imported meshes: boundary
    and random masks, penalties on and off"""
    check_products(lib, gm.imported(dim, nelem, ngl), ("boundary", "random"), f"dim {dim} ngl {ngl} {nelem} imported", oracle=False)


@pytest.mark.parametrize("k,ngl,layers", [(3, 4, 0), (3, 5, 0), (3, 8, 0), (5, 4, 0), (5, 5, 0), (5, 8, 0), (3, 4, 2), (3, 5, 2)])
def test_valence_three_and_five(lib, k, ngl, layers):
    """k cells around a vertex (and, extruded, around an edge): the gather pass follows the incidence list, not a lattice"""
    mesh = gm.star(k, ngl, layers)
    assert gm.valences(mesh).max() == (2 * k if layers else k)
    check_products(lib, mesh, ("none", "boundary", "random"), f"star {k} ngl {ngl} layers {layers}")


@pytest.mark.parametrize("dim,ngl,nelem", [(2, 5, [4, 3]), (3, 4, [2, 3, 2])])
def test_both_ids_on_an_affine_lattice(lib, dim, ngl, nelem):
    """a lexicographic lattice of affine cells takes both operators: they agree, and two snapshots with different masks AND different
    penalties on one context each reproduce their own oracle K, whatever the order of the applications"""
    mesh = fo.box_mesh(nelem, [0.0] * dim, gm.UPPER[:dim], ngl)
    mk = gm.masks(mesh)
    m0, m1 = mk["boundary"], mk["random"]
    x = np.random.default_rng(4).standard_normal(mesh.n_node * dim)
    ctx = make_ctx(lib, mesh, m0, dim, ngl=ngl)
    assert ctx.mesh_ho_lattice()[0] == ngl
    vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)

    def apply(op):
        ctx.matfree_apply(vx, vy, op)
        return ctx.vec_get(vy, dim)

    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.matfree_set(lib.MATFREE_KLE_GENERAL, 1e3, 1e2)
    ya, yg = apply(lib.MATFREE_KLE), apply(lib.MATFREE_KLE_GENERAL)
    print(f"dim {dim} ngl {ngl}: general vs affine {rel_err(yg, ya):.3e}")
    assert rel_err(yg, ya) < FP_TOL
    # independent snapshots: the affine operator keeps (m0, 1e3, 1e2); the general one takes (m1, 4e2, 3e1)
    ctx.bc_set(dim, m1)
    ctx.matfree_set(lib.MATFREE_KLE_GENERAL, 4e2, 3e1)
    want_a = gm.oracle_K(mesh, m0, 1e3, 1e2) @ x
    want_g = gm.oracle_K(mesh, m1, 4e2, 3e1) @ x
    for op, want in ((lib.MATFREE_KLE, want_a), (lib.MATFREE_KLE_GENERAL, want_g), (lib.MATFREE_KLE, want_a)):
        assert rel_err(apply(op), want) < FP_TOL, op
    # ... and the other way round: the affine snapshot is replaced, the general one stays
    ctx.bc_set(dim, None)
    ctx.matfree_set(lib.MATFREE_KLE, 0.0, 0.0)
    assert rel_err(apply(lib.MATFREE_KLE_GENERAL), want_g) < FP_TOL
    assert rel_err(apply(lib.MATFREE_KLE), gm.oracle_K(mesh, None, 0.0, 0.0) @ x) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals(lib, dim):
    """an inverted cell, a rank's slab, an order above the limit, an ngl 3 mesh and vectors of the wrong block size are refused with a
    message; after the refusal of the inverted cell the operator is not set, so nothing is launched on that mesh"""
    ngl = 4
    G = lib.MATFREE_KLE_GENERAL
    mesh = gm.imported(dim, [3, 2] if dim == 2 else [2, 2, 2], ngl)
    ctx = make_ctx(lib, mesh, gm.boundary_mask(mesh), dim, ngl=ngl)
    ctx.matfree_set(G, 1e3, 1e2)
    wrong = 3 if dim == 2 else 2
    vx, vy = ctx.vec_create(wrong), ctx.vec_create(wrong)
    with pytest.raises(lib.PynamaHipError, match="block size"):
        ctx.matfree_apply(vx, vy, G)
    ctx.close()
    # one corner of a single cell pushed through the opposite edges: det J <= 0 near that corner
    bad = fo.box_mesh([1] * dim, [0.0] * dim, [1.0] * dim, ngl)
    nc = 2 ** dim
    corners = bad.xyz[bad.conn[0, :nc]].copy()
    far = int(np.argmin(np.linalg.norm(corners, axis=1)))              # the corner at the origin ...
    corners[far] = 1.25                                                # ... to beyond the opposite corner
    bad.xyz[bad.conn[0]] = gm._corner_image(ngl, dim, corners[None])[0]
    ctx = make_ctx(lib, bad, None, dim, ngl=ngl)
    with pytest.raises(lib.PynamaHipError, match="non-positive Jacobian"):
        ctx.matfree_set(G, 1e3, 1e2)
    vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
    with pytest.raises(lib.PynamaHipError, match="pyn_matfree_set first"):
        ctx.matfree_apply(vx, vy, G)
    ctx.close()
    # a rank's slab (detached context with a ghost tail)
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    nelem, size = ([2, 7], 3) if dim == 2 else ([2, 2, 4], 2)          # slabs of tests/test_gpu_ho_matfree.py::test_rank_slabs
    dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0.0] * dim, 'upper': gm.UPPER[:dim]}, comm=Comm(0, size))
    dom.setFemIndexing(ngl)
    ctx = lib.Context(0)
    ctx.comm_init(0, size, None)
    ctx.halo_set(*dom._halo_plan())
    ctx.mesh_set(dim, dom.conn, dom.xyz)
    for t in Spectral(ngl, dim).deviceTables():
        ctx.tables_set(*t)
    ctx.csr_symbolic()
    with pytest.raises(lib.PynamaHipError, match="one rank"):
        ctx.matfree_set(G, 1e3, 1e2)
    ctx.close()
    # one order above the limit
    big = 13 if dim == 2 else 9
    mesh = fo.box_mesh([1] * dim, [0.0] * dim, [1.0] * dim, big)
    ctx = make_ctx(lib, mesh, None, dim, ngl=big)
    with pytest.raises(lib.PynamaHipError, match=f"ngl {big} is above the limit.*ngl <= {big - 1}"):
        ctx.matfree_set(G, 1e3, 1e2)
    ctx.close()
    # a second-order mesh: the message names the orders the operator serves
    mesh = fo.box_mesh([2] * dim, [0.0] * dim, [1.0] * dim, 3)
    ctx = make_ctx(lib, mesh, None, dim, ngl=3)
    with pytest.raises(lib.PynamaHipError, match=r"order ngl 4\.\.12 \(2-D\) / 4\.\.8 \(3-D\).*ngl 3"):
        ctx.matfree_set(G, 1e3, 1e2)
    vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
    with pytest.raises(lib.PynamaHipError, match=r"order ngl 4\.\.12"):
        ctx.matfree_apply(vx, vy, G)
    ctx.close()


@pytest.mark.parametrize("kind,dim,ngl,nelem", [("bent", 2, 5, [16, 16]), ("imported", 3, 4, [6, 6, 6])])
def test_krylov_with_the_shell(lib, kind, dim, ngl, nelem):
    """Jacobi-PCG with the shell and with the assembled product on the same system: rtol 1e-10, iteration counts within +-1, true
    residual against the assembled matrix <= 1e-10; the guard trips when K is edited after the snapshot"""
    mesh = build(kind, dim, ngl, nelem)
    mask = gm.boundary_mask(mesh)
    ctx = make_ctx(lib, mesh, mask, dim, ngl=ngl)
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(1e3, 1e2, K)
    ctx.matfree_set(lib.MATFREE_KLE_GENERAL, 1e3, 1e2)
    b = np.random.default_rng(2).standard_normal(mesh.n_node * dim)
    b[mask.reshape(-1).astype(bool)] = 0.0
    vb, vx = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vb, b)
    kw = dict(method=lib.KSP_CG, pc=lib.PC_JACOBI, rtol=1e-10, atol=1e-300, maxit=100000, norm_type=lib.NORM_UNPRECONDITIONED)
    ctx.vec_set(vx, np.zeros_like(b))
    ia = ctx.solve(K, vb, vx, **kw)
    xa = ctx.vec_get(vx, dim)
    ctx.vec_set(vx, np.zeros_like(b))
    im = ctx.solve(K, vb, vx, matfree=lib.MATFREE_KLE_GENERAL, **kw)
    xm = ctx.vec_get(vx, dim)
    print(f"{kind} dim {dim} ngl {ngl}: iters assembled {ia.iters} shell {im.iters}, true_resid {im.true_resid:.3e}, "
          f"x diff {rel_err(xm, xa):.3e}")
    assert ia.reason > 0 and im.reason > 0, (ia.reason, im.reason)
    assert abs(ia.iters - im.iters) <= 1, (ia.iters, im.iters)
    assert im.true_resid <= 1e-10, im.true_resid
    assert rel_err(xm, xa) < 1e-7
    # K edited after the snapshot (a free DOF, where b is not zero): the shell no longer is this matrix
    free = np.nonzero(~mask.reshape(-1).astype(bool))[0]
    d = int(free[len(free) // 2])
    ctx.mat_add_values(K, np.array([d], np.int32), np.array([d], np.int32), np.array([1.0e3]), insert=False)
    with pytest.raises(lib.PynamaHipError, match="matrix-free operator differs"):
        ctx.solve(K, vb, vx, matfree=lib.MATFREE_KLE_GENERAL, **kw)
    ctx.close()


@pytest.mark.parametrize("case", [(2, 5, [9, 7]), (2, 12, [3, 2]), (3, 4, [3, 3, 3]), (3, 8, [2, 1, 1]), "star5"], ids=str)
def test_two_applications_are_bit_identical(lib, case):
    mesh = gm.star(5, 5) if case == "star5" else gm.imported(case[0], case[2], case[1])
    dim = mesh.dim
    ctx = make_ctx(lib, mesh, gm.masks(mesh)["per_dof"], dim, ngl=mesh.ngl)
    ctx.matfree_set(lib.MATFREE_KLE_GENERAL, 1e3, 1e2)
    x = np.random.default_rng(8).standard_normal(mesh.n_node * dim)
    vx, vy, vz = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.vec_set(vy, np.full_like(x, np.nan))              # no pre-zeroed y: every row is written
    ctx.matfree_apply(vx, vy, lib.MATFREE_KLE_GENERAL)
    ctx.matfree_apply(vx, vz, lib.MATFREE_KLE_GENERAL)
    y, z = ctx.vec_get(vy, dim), ctx.vec_get(vz, dim)
    assert np.all(np.isfinite(y)) and np.array_equal(y, z)
    ctx.close()


def _facade_run(mode, tmp_path):
    out = str(tmp_path / f"run_{mode}.npz")
    worker = os.path.join(ROOT, "tests", "ho_matfree_general_facade_worker.py")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, worker, mode, out, str(tmp_path)], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return np.load(out)


@pytest.mark.parametrize("case", ["gmsh2d", "gmsh3d"])
def test_facade_flag_on_gmsh_files(lib, tmp_path, case):
    """-pynama_mat_free_ho_general: on an imported Gmsh mesh lifted to ngl 5 (2-D) / 4 (3-D) Mat.assembleKLE tags K with the general
    operator and the uniform-flow solve takes the shell; without the option K stays untagged; both runs meet the uniform field and
    give the same velocity.  Each run in a fresh child process under its own time limit, one after the other."""
    off = _facade_run(f"{case}:off", tmp_path)
    assert int(off["tag"]) == -1 and not bool(off["shell_used"]) and str(off["topo"]) == "general"
    on = _facade_run(f"{case}:on", tmp_path)              # (sequential: the second child starts only after the first ended well)
    assert int(on["tag"]) == lib.MATFREE_KLE_GENERAL and bool(on["shell_used"]) and str(on["topo"]) == "general"
    print(f"facade {case}: err off {float(off['err']):.3e} on {float(on['err']):.3e} diff {rel_err(on['vel'], off['vel']):.3e}")
    assert float(on["err"]) < 1e-10 and float(off["err"]) < 1e-10
    assert rel_err(on["vel"], off["vel"]) < 1e-9


def test_facade_both_flags_on_an_affine_box(lib, tmp_path):
    """with -pynama_mat_free_ho and -pynama_mat_free_ho_general on the Taylor-Green box the affine shell is taken"""
    both = _facade_run("tg:both", tmp_path)
    assert int(both["tag"]) == lib.MATFREE_KLE and bool(both["shell_used"])
