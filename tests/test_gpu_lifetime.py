"""Every device buffer has an owner (pynama_amd/csrc/pyn_internal.h: DevBuf): the library's count of live allocations and their bytes
(_lib.alloc_live) returns to where it started when a context closes, when the same mesh / graph / matrix is installed again, when a
matrix is destroyed and when a compact imposed-column matrix is laid out again.  Exact integer equalities: no timing, no device-memory
query."""
import gc

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.test_gpu_ho3 import boundary_mask, make_ctx

pytestmark = pytest.mark.gpu

SELL_KINDS = (2, 3, 4, 5)   # Context.product_last()['family'] of the kernels that read a SELL image


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@pytest.fixture(autouse=True)
def no_collection_inside_a_test():
    """contexts that earlier tests left to the garbage collector close now, not between two readings"""
    gc.collect()
    gc.disable()
    yield
    gc.enable()


def q1_box(n=8):
    return fo.box_mesh([n] * 3, [0.0] * 3, [1.0] * 3, 2)


def rhs_vec(ctx, mesh, bs, seed=0):
    b = np.random.default_rng(seed).standard_normal((mesh.n_node, bs))
    b[mesh.boundary] = 0.0
    vb, vx = ctx.vec_create(bs), ctx.vec_create(bs)
    ctx.vec_set(vb, b.ravel())
    return vb, vx


def scalar_system(lib, ctx, mesh):
    """K (scalar Laplacian, Dirichlet faces: the context's current 1-DOF mask), right-hand side and solution vectors"""
    K = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, K)
    return (K,) + rhs_vec(ctx, mesh, 1)


def use_every_matrix_buffer(lib, ctx, K, vb, vx, monkeypatch):
    """SELL image, 1 / diagonal, dense LU, banded LU and a multigrid hierarchy on one scalar matrix"""
    with monkeypatch.context() as m:
        m.setenv("PYNAMA_SELL_IMAGE", "1")
        ctx.spmv(K, vb, vx)                                  # a one-off product that builds the image
    assert ctx.product_last()["family"] in SELL_KINDS
    assert ctx.solve(K, vb, vx, pc=lib.PC_JACOBI, rtol=1e-8).reason == 2
    ctx.mg_setup(K, coarse_max_rows=100)                     # 9^3 nodes: 3 levels (tests/test_gpu_mg.py, q1hex [8, 8, 8])
    assert ctx.mg_info(K)["levels"] >= 2
    assert ctx.solve(K, vb, vx, pc=lib.PC_MG, rtol=1e-8).reason == 2
    assert ctx.mat_stored(K)[1] * 1 <= ctx.direct_max_rows()
    ctx.solve_direct(K, vb, vx)                              # preonly/lu: dense factors ...
    ctx.solve_direct_band(K, vb, vx)                         # ... and the banded ones


# ---- 1. create and close returns to the start ---------------------------------------------------------------------------------------
def test_create_and_close_returns_to_the_start(lib, monkeypatch):
    start = lib.alloc_live()
    mesh = q1_box()
    ctx = make_ctx(lib, mesh, boundary_mask(mesh)[:, 0].copy(), 1, ngl=2)
    assert ctx.mesh_topology()[0] != "general"
    opened = lib.alloc_live()
    assert opened[0] > start[0] and opened[1] > start[1]
    K, vb, vx = scalar_system(lib, ctx, mesh)
    ctx.matfree_set(lib.MATFREE_LAPLACE)                     # the matrix-free Q1 operator: a snapshot of the 1-DOF mask
    ctx.matfree_apply(vb, vx, lib.MATFREE_LAPLACE)
    use_every_matrix_buffer(lib, ctx, K, vb, vx, monkeypatch)
    ctx.bc_set(3, boundary_mask(mesh))
    K3, Kr = ctx.mat_create(3, 3), ctx.mat_create_rhs(3, 3)  # a 3x3 KLE matrix with a compact Krhs
    ctx.assemble_kle(1e3, 1e2, K3, Kr)
    assert ctx.mat_stored(Kr)[0] < ctx.mat_stored(K3)[0]
    vb3, vx3 = rhs_vec(ctx, mesh, 3)
    ctx.spmv(K3, vb3, vx3)
    ctx.spmv(Kr, vb3, vx3)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.matfree_apply(vb3, vx3, lib.MATFREE_KLE)
    s = ctx.nodeset_create(np.unique(mesh.boundary))
    assert s >= 0
    busy = lib.alloc_live()
    assert busy[0] > opened[0] and busy[1] > opened[1]
    ctx.close()
    assert lib.alloc_live() == start


# ---- 2. the same for the other owners, each in its own context ----------------------------------------------------------------------
def _rowrun_and_ho3_operator(lib):
    """2-D ngl 3 box of 4 x 4 cells: the row-run view (d_geom, d_nbits, run flags) and the matrix-free operator of second-order lattices"""
    mesh = fo.box_mesh([4, 4], [0.0, 0.0], [1.0, 1.0], 3)
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), 2, ngl=3)
    K, Kr = ctx.mat_create(2, 2), ctx.mat_create_rhs(2, 2)
    ctx.assemble_kle(1e3, 1e2, K, Kr)
    assert ctx.assemble_last()["kind"] == lib.AK_ROWRUN
    vb, vx = rhs_vec(ctx, mesh, 2)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    ctx.matfree_apply(vb, vx, lib.MATFREE_KLE)
    return ctx


def _high_order_operators(lib):
    """2-D ngl 4 box of 3 x 3 cells under both matrix-free KLE operators: the 1-D tables, d_ho_ye, the incidence lists"""
    mesh = fo.box_mesh([3, 3], [0.0, 0.0], [1.0, 1.0], 4)
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), 2, ngl=4)
    vb, vx = rhs_vec(ctx, mesh, 2)
    for op in (lib.MATFREE_KLE, lib.MATFREE_KLE_GENERAL, lib.MATFREE_KLE_GENERAL):   # (the second set of one operator replaces its lists)
        ctx.matfree_set(op, 1e3, 1e2)
        ctx.matfree_apply(vb, vx, op)
    return ctx


def _tet_patch_plans(lib):
    """the small tetrahedral mesh of tests/test_gpu_simplex.py: the automatic patch plan of the scalar kernel"""
    from tests.test_gpu_simplex import _ctx
    mesh = fo.simplex_box_mesh([7, 6, 5], [0.0] * 3, [1.0] * 3, jitter=0.2, permute_seed=7)
    ctx = _ctx(lib, mesh, bc_ndof=1)
    A, Ar = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)
    assert ctx.assemble_last()["kind"] == lib.AK_PATCH and ctx.patch_plan_info(0)[0] > 0
    return ctx


def _ibm_markers(lib):
    """the small marker set of tests/test_gpu_ibm.py on its 2-D second-order grid: IbmState (set twice: the second one refits)"""
    from tests.test_gpu_ibm import Grid
    g = Grid("2d-ngl3")
    for count in (5, 9):
        X, dl = g.markers(count, seed=3)
        g.ctx.ibm_set(0, X, dl, g.lower, g.h)
        assert g.interp(g.xyz).shape[0] == count
    return g.ctx


@pytest.mark.parametrize("owner", [_rowrun_and_ho3_operator, _high_order_operators, _tet_patch_plans, _ibm_markers])
def test_other_owners_return_to_the_start(lib, owner):
    start = lib.alloc_live()
    ctx = owner(lib)
    assert lib.alloc_live()[0] > start[0]
    ctx.close()
    assert lib.alloc_live() == start


# ---- 3. installing the same thing again replaces, it does not add -------------------------------------------------------------------
def _install_q1(lib, ctx, mesh):
    from pynama_amd.elements.spectral import Spectral
    ctx.mesh_set(3, mesh.conn, mesh.xyz)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    ctx.bc_set(1, boundary_mask(mesh)[:, 0].copy())
    ctx.csr_symbolic()                                       # (drops the matrices of the round before)
    K = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, K)


def _install_tets(lib, ctx, mesh):
    from pynama_amd.elements.simplex import Simplex
    ctx.mesh_set(3, mesh.conn, mesh.xyz)
    for t in Simplex(3).deviceTables():
        ctx.tables_set(*t)
    ctx.bc_set(1, boundary_mask(mesh)[:, 0].copy())
    ctx.csr_symbolic()                                       # the general (sorted) graph; the patch plan goes with the old one
    K = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, K)
    assert ctx.patch_plan_info(0)[0] > 0


@pytest.mark.parametrize("kind", ["q1-lattice", "tets"])
def test_reinstalling_is_idempotent(lib, kind):
    if kind == "q1-lattice":
        mesh, install = q1_box(), _install_q1
    else:
        mesh, install = fo.simplex_box_mesh([4, 3, 3], [0.0] * 3, [1.0] * 3, jitter=0.2, permute_seed=7), _install_tets
    ctx = lib.Context(0)
    install(lib, ctx, mesh)
    first = lib.alloc_live()
    for _ in range(2):
        install(lib, ctx, mesh)
        assert lib.alloc_live() == first
    ctx.close()


# ---- 4. destroying a matrix gives back what it held ---------------------------------------------------------------------------------
def test_mat_destroy_gives_back_what_the_matrix_held(lib, monkeypatch):
    mesh = q1_box()
    ctx = make_ctx(lib, mesh, boundary_mask(mesh)[:, 0].copy(), 1, ngl=2)
    K0, vb, vx = scalar_system(lib, ctx, mesh)
    use_every_matrix_buffer(lib, ctx, K0, vb, vx, monkeypatch)   # the context's own scratch and SELL structure exist from here on
    before = lib.alloc_live()
    K = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, K)
    use_every_matrix_buffer(lib, ctx, K, vb, vx, monkeypatch)
    held = lib.alloc_live()
    nnzb = ctx.mat_stored(K)[0]
    ctx.mat_destroy(K)
    after = lib.alloc_live()
    assert held[1] - after[1] >= nnzb * 1 * 1 * 8
    assert after[0] == before[0]
    assert after == before                                   # (stronger: the bytes return too)
    ctx.close()


# ---- 5. laying a compact Krhs out again does not grow -------------------------------------------------------------------------------
def test_relayout_of_a_compact_krhs_does_not_grow(lib):
    mesh = q1_box()
    set_a = boundary_mask(mesh)
    set_b = np.zeros_like(set_a)
    set_b[mesh.xyz[:, 0] < 0.3] = 1                          # another selection of node rows, and more of them
    ctx = make_ctx(lib, mesh, set_a, 3, ngl=2)
    K, Kr = ctx.mat_create(3, 3), ctx.mat_create_rhs(3, 3)
    ctx.assemble_kle(1e3, 1e2, K, Kr)
    rows_a = ctx.mat_stored(Kr)
    first = lib.alloc_live()
    ctx.bc_set(3, set_b)
    ctx.assemble_kle(1e3, 1e2, K, Kr)
    assert ctx.mat_stored(Kr) != rows_a
    lib.alloc_live()
    ctx.bc_set(3, set_a)
    ctx.assemble_kle(1e3, 1e2, K, Kr)
    assert ctx.mat_stored(Kr) == rows_a
    assert lib.alloc_live() == first
    ctx.close()
