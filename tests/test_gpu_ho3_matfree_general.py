"""GPU parity of the general ngl 3 matrix-free KLE operator PYN_MATFREE_KLE_NGL3_GENERAL (pynama_amd/csrc/pyn_matfree_ho3_general.hip):
any quadrilateral / hexahedral mesh of order ngl 3 -- bent cells, random numbering, cell order and cell orientation, vertices of valence
3 and 5 -- against the CPU oracle's K (one K_e per cell) and the assembled K; the refusals, the snapshot, the new id next to
PYN_MATFREE_KLE on an affine lattice, CG and GMRES with the shell, run-to-run determinism and the opt-in facade flag
-pynama_mat_free_ngl3_general.

Bars: FP_TOL = 2e-13 with tests.util.rel_err for the products, the project's bar for every shell: the numpy model of the kernel equals
the oracle's dense K_e x_e to <= 1e-14 per cell on bent and rotated cells (tests/test_ho3_matfree_general_host.py), which leaves a
factor 20 for the accumulation over a node's cells and the row sums.  Krylov: the bars of
tests/test_gpu_ho_matfree_general.py::test_krylov_with_the_shell."""
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
NGL = 3


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


def build(kind, dim, nelem):
    return gm.bent_lattice(dim, nelem, NGL, seed=3) if kind == "bent" else gm.imported(dim, nelem, NGL)


def shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w):
    G = lib.MATFREE_KLE_NGL3_GENERAL
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(alpha_d, alpha_w, K)
    ctx.matfree_set(G, alpha_d, alpha_w)
    vx, vy, va = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.matfree_apply(vx, vy, G)
    ctx.spmv(K, vx, va)
    return K, ctx.vec_get(vy, dim), ctx.vec_get(va, dim)


def check_products(lib, mesh, mask_names, tag, topo=None):
    dim = mesh.dim
    x = np.random.default_rng(1).standard_normal(mesh.n_node * dim)
    mk = gm.masks(mesh)
    for alpha_d, alpha_w in ALPHAS:                       # (outer: the oracle's element matrices are cached per penalty pair)
        for name in mask_names:
            ctx = make_ctx(lib, mesh, mk[name], dim, ngl=NGL)
            if topo is not None:
                assert ctx.mesh_topology()[0] == topo
            _, y, ya = shell_and_assembled(lib, ctx, dim, x, alpha_d, alpha_w)
            ea = rel_err(y, ya)
            eo = rel_err(y, gm.oracle_K(mesh, mk[name], alpha_d, alpha_w) @ x)
            print(f"{tag} {name} alpha_d {alpha_d}: vs oracle {eo:.3e} vs assembled {ea:.3e}")
            assert eo < FP_TOL, (name, alpha_d, eo)
            assert ea < FP_TOL, (name, alpha_d, ea)
            ctx.close()


# cells per 256-lane workgroup of h3g_cell_kernel: 2-D 28 (252 lanes), 3-D 9 (243 lanes).  One cell, fewer cells than one workgroup
# takes, exactly one workgroup, one workgroup and a remainder, several workgroups
CASES = [(2, [1, 1]), (2, [3, 2]), (2, [7, 4]), (2, [6, 5]), (2, [9, 7]),
         (3, [1, 1, 1]), (3, [2, 2, 2]), (3, [3, 3, 1]), (3, [5, 2, 1]), (3, [3, 2, 3])]


@pytest.mark.parametrize("dim,nelem", CASES)
@pytest.mark.parametrize("kind", ["bent", "imported"])
def test_shell_equals_oracle_and_assembled(lib, dim, nelem, kind):
    """matfree_apply == oracle K x == spmv(K) x on bent lattices and on imported meshes: every kind of mask, penalties on and off"""
    mesh = build(kind, dim, nelem)
    # (a bent lattice keeps the topology lattice-ngl3; an imported mesh has none)
    check_products(lib, mesh, ("none", "boundary", "per_dof", "random"), f"dim {dim} {nelem} {kind}",
                   topo="general" if kind == "imported" else None)


@pytest.mark.parametrize("k,layers", [(3, 0), (5, 0), (3, 2), (5, 2)])
def test_valence_three_and_five(lib, k, layers):
    """k cells around a vertex (and, extruded, around an edge): the gather pass follows the incidence list, not a lattice"""
    mesh = gm.star(k, NGL, layers)
    assert gm.valences(mesh).max() == (2 * k if layers else k)
    check_products(lib, mesh, ("none", "boundary", "random"), f"star {k} layers {layers}")


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals(lib, dim):
    """messages only, nothing is launched on a refused mesh: orders ngl 4 and 2, an inverted cell, a rank's slab, vectors of the wrong
    block size, apply before set, the scalar (Laplacian) semantics; the two older ids still refuse a bent ngl 3 mesh"""
    G = lib.MATFREE_KLE_NGL3_GENERAL
    small = [3, 2] if dim == 2 else [2, 2, 2]
    for ngl in (4, 2):
        mesh = fo.box_mesh(small, [0.0] * dim, gm.UPPER[:dim], ngl)
        ctx = make_ctx(lib, mesh, None, dim, ngl=ngl)
        with pytest.raises(lib.PynamaHipError, match=rf"order ngl 3; this mesh has ngl {ngl}.*PYN_MATFREE_KLE_GENERAL"):
            ctx.matfree_set(G, 1e3, 1e2)
        vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
        with pytest.raises(lib.PynamaHipError, match="pyn_matfree_set first"):
            ctx.matfree_apply(vx, vy, G)
        ctx.close()
    mesh = gm.imported(dim, small, NGL)
    # apply before set; wrong block size; the scalar semantics of PYN_MATFREE_LAPLACE (a mask of one DOF per node, scalar vectors)
    ctx = make_ctx(lib, mesh, gm.boundary_mask(mesh), dim, ngl=NGL)
    vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
    with pytest.raises(lib.PynamaHipError, match="pyn_matfree_set first"):
        ctx.matfree_apply(vx, vy, G)
    ctx.matfree_set(G, 1e3, 1e2)
    wrong = 3 if dim == 2 else 2
    wx, wy = ctx.vec_create(wrong), ctx.vec_create(wrong)
    with pytest.raises(lib.PynamaHipError, match="block size"):
        ctx.matfree_apply(wx, wy, G)
    sx, sy = ctx.vec_create(1), ctx.vec_create(1)
    with pytest.raises(lib.PynamaHipError, match="block size"):
        ctx.matfree_apply(sx, sy, G)
    with pytest.raises(lib.PynamaHipError):
        ctx.matfree_set(lib.MATFREE_LAPLACE)               # no scalar shell on this mesh, under any id
    ctx.bc_set(1, gm.boundary_mask(mesh)[:, 0].copy())
    with pytest.raises(lib.PynamaHipError, match=rf"{dim} DOF\(s\) per node"):
        ctx.matfree_set(G, 1e3, 1e2)
    ctx.close()
    # one corner of a single cell pushed through the opposite edges: det J <= 0 near that corner
    bad = fo.box_mesh([1] * dim, [0.0] * dim, [1.0] * dim, NGL)
    nc = 2 ** dim
    corners = bad.xyz[bad.conn[0, :nc]].copy()
    far = int(np.argmin(np.linalg.norm(corners, axis=1)))              # the corner at the origin ...
    corners[far] = 1.25                                                # ... to beyond the opposite corner
    bad.xyz[bad.conn[0]] = gm._corner_image(NGL, dim, corners[None])[0]
    ctx = make_ctx(lib, bad, None, dim, ngl=NGL)
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
    nelem, size = ([2, 7], 3) if dim == 2 else ([2, 2, 4], 2)
    dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0.0] * dim, 'upper': gm.UPPER[:dim]}, comm=Comm(0, size))
    dom.setFemIndexing(NGL)
    ctx = lib.Context(0)
    ctx.comm_init(0, size, None)
    ctx.halo_set(*dom._halo_plan())
    ctx.mesh_set(dim, dom.conn, dom.xyz)
    for t in Spectral(NGL, dim).deviceTables():
        ctx.tables_set(*t)
    ctx.csr_symbolic()
    with pytest.raises(lib.PynamaHipError, match="one rank"):
        ctx.matfree_set(G, 1e3, 1e2)
    ctx.close()
    # the older ids on a bent second-order lattice, as before
    mesh = build("bent", dim, small)
    ctx = make_ctx(lib, mesh, gm.boundary_mask(mesh), dim, ngl=NGL)
    with pytest.raises(lib.PynamaHipError, match="affine"):
        ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    with pytest.raises(lib.PynamaHipError, match=r"order ngl 4\.\.12 \(2-D\) / 4\.\.8 \(3-D\).*ngl 3"):
        ctx.matfree_set(lib.MATFREE_KLE_GENERAL, 1e3, 1e2)
    ctx.matfree_set(G, 1e3, 1e2)                           # ... and the new one takes it
    ctx.close()


@pytest.mark.parametrize("dim,nelem", [(2, [4, 3]), (3, [2, 3, 2])])
def test_snapshot_and_both_ids_on_an_affine_lattice(lib, dim, nelem):
    """a bc_set after matfree_set leaves the shell alone, a second matfree_set takes the new mask; on an affine second-order lattice
    the new id and PYN_MATFREE_KLE sit side by side, agree, and keep snapshots of their own (mask AND penalties)"""
    G, A = lib.MATFREE_KLE_NGL3_GENERAL, lib.MATFREE_KLE
    mesh = fo.box_mesh(nelem, [0.0] * dim, gm.UPPER[:dim], NGL)
    mk = gm.masks(mesh)
    m0, m1 = mk["boundary"], mk["random"]
    x = np.random.default_rng(4).standard_normal(mesh.n_node * dim)
    ctx = make_ctx(lib, mesh, m0, dim, ngl=NGL)
    assert ctx.mesh_topology()[0] == "lattice-ngl3"
    vx, vy = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)

    def apply(op):
        ctx.matfree_apply(vx, vy, op)
        return ctx.vec_get(vy, dim)

    ctx.matfree_set(A, 1e3, 1e2)
    ctx.matfree_set(G, 1e3, 1e2)
    ya, yg = apply(A), apply(G)
    print(f"dim {dim}: general vs affine {rel_err(yg, ya):.3e}")
    assert rel_err(yg, ya) < FP_TOL
    want0 = gm.oracle_K(mesh, m0, 1e3, 1e2) @ x
    ctx.bc_set(dim, m1)                                    # the snapshot stays
    assert rel_err(apply(G), want0) < FP_TOL
    ctx.matfree_set(G, 4e2, 3e1)                           # the general operator takes (m1, 4e2, 3e1), the affine one keeps its own
    want_g = gm.oracle_K(mesh, m1, 4e2, 3e1) @ x
    for op, want in ((A, want0), (G, want_g), (A, want0)):
        assert rel_err(apply(op), want) < FP_TOL, op
    ctx.bc_set(dim, None)                                  # ... and the other way round
    ctx.matfree_set(A, 0.0, 0.0)
    assert rel_err(apply(G), want_g) < FP_TOL
    assert rel_err(apply(A), gm.oracle_K(mesh, None, 0.0, 0.0) @ x) < FP_TOL
    ctx.close()


@pytest.mark.parametrize("kind,dim,nelem", [("bent", 2, [16, 16]), ("imported", 3, [6, 6, 6])])
def test_krylov_with_the_shell(lib, kind, dim, nelem):
    """Jacobi-PCG and GMRES with the shell and with the assembled product on the same system: rtol 1e-10, iteration counts within
    +-1, true residual against the assembled matrix <= 1e-10; a shell set with other penalty weights is refused before the iteration"""
    G = lib.MATFREE_KLE_NGL3_GENERAL
    mesh = build(kind, dim, nelem)
    mask = gm.boundary_mask(mesh)
    ctx = make_ctx(lib, mesh, mask, dim, ngl=NGL)
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(1e3, 1e2, K)
    ctx.matfree_set(G, 1e3, 1e2)
    b = np.random.default_rng(2).standard_normal(mesh.n_node * dim)
    b[mask.reshape(-1).astype(bool)] = 0.0
    vb, vx = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vb, b)
    for method, name in ((lib.KSP_CG, "cg"), (lib.KSP_GMRES, "gmres")):
        kw = dict(method=method, pc=lib.PC_JACOBI, rtol=1e-10, atol=1e-300, maxit=100000, norm_type=lib.NORM_UNPRECONDITIONED)
        ctx.vec_set(vx, np.zeros_like(b))
        ia = ctx.solve(K, vb, vx, **kw)
        xa = ctx.vec_get(vx, dim)
        ctx.vec_set(vx, np.zeros_like(b))
        im = ctx.solve(K, vb, vx, matfree=G, **kw)
        xm = ctx.vec_get(vx, dim)
        print(f"{kind} dim {dim} {name}: iters assembled {ia.iters} shell {im.iters}, true_resid {im.true_resid:.3e}, "
              f"x diff {rel_err(xm, xa):.3e}")
        assert ia.reason > 0 and im.reason > 0, (ia.reason, im.reason)
        assert abs(ia.iters - im.iters) <= 1, (ia.iters, im.iters)
        assert im.true_resid <= 1e-10, im.true_resid
        assert rel_err(xm, xa) < 1e-7
    with pytest.raises(lib.PynamaHipError, match="multigrid"):
        ctx.solve(K, vb, vx, method=lib.KSP_CG, pc=lib.PC_MG, matfree=G)
    ctx.matfree_set(G, 4e2, 3e1)                           # no longer the operator K was assembled as
    with pytest.raises(lib.PynamaHipError, match="matrix-free operator differs"):
        ctx.solve(K, vb, vx, matfree=G, **kw)
    ctx.close()


@pytest.mark.parametrize("case", [(2, [9, 7]), (3, [3, 3, 3]), "star5"], ids=str)
def test_two_applications_are_bit_identical(lib, case):
    mesh = gm.star(5, NGL) if case == "star5" else gm.imported(case[0], case[1], NGL)
    dim = mesh.dim
    G = lib.MATFREE_KLE_NGL3_GENERAL
    ctx = make_ctx(lib, mesh, gm.masks(mesh)["per_dof"], dim, ngl=NGL)
    ctx.matfree_set(G, 1e3, 1e2)
    x = np.random.default_rng(8).standard_normal(mesh.n_node * dim)
    vx, vy, vz = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vx, x)
    ctx.vec_set(vy, np.full_like(x, np.nan))              # no pre-zeroed y: every row is written
    ctx.matfree_apply(vx, vy, G)
    ctx.matfree_apply(vx, vz, G)
    y, z = ctx.vec_get(vy, dim), ctx.vec_get(vz, dim)
    assert np.all(np.isfinite(y)) and np.array_equal(y, z)
    ctx.close()


def _facade_run(mode, tmp_path):
    out = str(tmp_path / f"run_{mode.replace(':', '_')}.npz")
    worker = os.path.join(ROOT, "tests", "ho3_matfree_general_facade_worker.py")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, worker, mode, out, str(tmp_path)], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return np.load(out)


@pytest.mark.parametrize("case", ["gmsh2d", "gmsh3d"])
def test_facade_flag_on_gmsh_files(lib, tmp_path, case):
    """-pynama_mat_free_ngl3_general: on an imported Gmsh mesh lifted to ngl 3 Mat.assembleKLE tags K with the new operator and the
    uniform-flow solve takes the shell; without the option K stays untagged; both runs meet the uniform field and give the same
    velocity.  Each run in a fresh child process under its own time limit, one after the other."""
    off = _facade_run(f"{case}:off", tmp_path)
    assert int(off["tag"]) == -1 and not bool(off["shell_used"]) and str(off["topo"]) == "general"
    on = _facade_run(f"{case}:on", tmp_path)              # (sequential: the second child starts only after the first ended well)
    assert int(on["tag"]) == lib.MATFREE_KLE_NGL3_GENERAL and bool(on["shell_used"]) and str(on["topo"]) == "general"
    print(f"facade {case}: err off {float(off['err']):.3e} on {float(on['err']):.3e} diff {rel_err(on['vel'], off['vel']):.3e}")
    assert float(on["err"]) < 1e-10 and float(off["err"]) < 1e-10
    assert rel_err(on["vel"], off["vel"]) < 1e-9


def test_facade_both_flags_on_lattices(lib, tmp_path):
    """with -pynama_mat_free_ngl3 and -pynama_mat_free_ngl3_general a lattice with one vertex moved ends with the new operator (the
    affine shell refuses it), the affine lattice with PYN_MATFREE_KLE"""
    bent = _facade_run("bent2d:both", tmp_path)
    assert str(bent["topo"]) == "lattice-ngl3"
    assert int(bent["tag"]) == lib.MATFREE_KLE_NGL3_GENERAL and bool(bent["shell_used"]) and float(bent["err"]) < 1e-10
    box = _facade_run("box2d:both", tmp_path)
    assert int(box["tag"]) == lib.MATFREE_KLE and bool(box["shell_used"]) and float(box["err"]) < 1e-10
