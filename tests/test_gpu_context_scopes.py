"""Context state by lifetime (pynama_amd/csrc/pyn_internal.h: CtxElement, CtxMesh, CtxGraph): what is derived from the element, the
mesh or the node graph ends with it, on one context that installs a second mesh.  The Dirichlet mask and the matrix-free operators end
with the mesh, the element tables with (dim, nn) -- and stay for a mesh of the same element --, matrix handles with the mesh; a refused
mesh leaves nothing of the old one, and installing over every owner is idempotent.

Every case is built so that a scope that ends too late FAILS AN ASSERTION: the stale state is larger than what the new mesh needs, and
dead handles are only handed to host-side calls."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.test_gpu_ho3 import boundary_mask, make_ctx
from tests.test_gpu_ho_matfree import FP_TOL as MF_TOL
from tests.test_gpu_lattice_axes import FP_TOL
from tests.test_gpu_lifetime import (_high_order_operators, _ibm_markers, _install_q1, _rowrun_and_ho3_operator, _tet_patch_plans,
                                     no_collection_inside_a_test, q1_box)   # noqa: F401 (the fixture is autouse here too)
from tests.util import mat_to_scipy, rel_err, sp_rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


def tables(ctx, ngl, dim):
    from pynama_amd.elements.spectral import Spectral
    for t in Spectral(ngl, dim).deviceTables():
        ctx.tables_set(*t)


def laplace(lib, ctx):
    """a new scalar matrix with the Laplacian under the context's current Dirichlet mask"""
    A = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    return A


def test_mask_ends_with_the_mesh_and_same_element_tables_stay(lib):
    big, small = q1_box(4), q1_box(2)
    ctx = make_ctx(lib, big, boundary_mask(big)[:, 0].copy(), 1, ngl=2)
    laplace(lib, ctx)
    ctx.mesh_set(3, small.conn, small.xyz)                   # no bc_set, no tables_set: the same element
    ctx.csr_symbolic()
    A = laplace(lib, ctx)
    free = fo.assemble_scalar(small, fo.Tables(2, 3), "laplace", dirichlet=np.zeros(0, np.int64))
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), free["A"]) < FP_TOL
    ctx.bc_set(1, boundary_mask(small)[:, 0].copy())
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    fixed = fo.assemble_scalar(small, fo.Tables(2, 3), "laplace", dirichlet=small.boundary)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), fixed["A"]) < FP_TOL
    ctx.close()


def test_tables_end_with_the_element(lib):
    hex27 = fo.box_mesh([2, 2, 2], [0.0] * 3, [1.0] * 3, 3)
    quad4 = fo.box_mesh([3, 2], [0.0, 0.0], [1.0, 1.0], 2)
    ctx = make_ctx(lib, hex27, ngl=3)
    ctx.mesh_set(2, quad4.conn, quad4.xyz)                   # nn 27 -> 4: stale tables would be larger than needed
    ctx.csr_symbolic()
    A = ctx.mat_create(1, 1)
    with pytest.raises(lib.PynamaHipError, match="tables"):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    tables(ctx, 2, 2)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A)
    ref = fo.assemble_scalar(quad4, fo.Tables(2, 2), "laplace")
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    ctx.close()


def test_matrices_end_with_the_mesh(lib):
    a, b = q1_box(3), q1_box(2)
    ctx = make_ctx(lib, a, ngl=2)
    K = ctx.mat_create(1, 1)
    ctx.mesh_set(3, b.conn, b.xyz)
    with pytest.raises(lib.PynamaHipError, match="invalid matrix handle"):
        ctx.mat_destroy(K)                                   # (a host-side call: the dead handle reaches no kernel)
    ctx.csr_symbolic()
    assert ctx.mat_create(1, 1) >= 0
    ctx.close()


def test_operators_end_with_the_mesh(lib):
    ctx = _high_order_operators(lib)                         # 2-D ngl 4, 3 x 3 cells, both matrix-free KLE operators set
    mesh = fo.box_mesh([2, 2], [0.0, 0.0], [1.0, 1.0], 4)
    ctx.mesh_set(2, mesh.conn, mesh.xyz)                     # the same element: the tables stay
    x = np.random.default_rng(5).standard_normal(mesh.n_node * 2)
    vx, vy, va = ctx.vec_create(2), ctx.vec_create(2), ctx.vec_create(2)
    ctx.vec_set(vx, x)
    ops = (lib.MATFREE_KLE, lib.MATFREE_KLE_GENERAL)
    for op in ops:
        with pytest.raises(lib.PynamaHipError, match="pyn_matfree_set first"):
            ctx.matfree_apply(vx, vy, op)
    ctx.bc_set(2, boundary_mask(mesh))
    ctx.csr_symbolic()
    K = ctx.mat_create(2, 2)
    ctx.assemble_kle(1e3, 1e2, K)
    ctx.spmv(K, vx, va)
    for op in ops:
        ctx.matfree_set(op, 1e3, 1e2)
        ctx.matfree_apply(vx, vy, op)
        assert rel_err(ctx.vec_get(vy, 2), ctx.vec_get(va, 2)) < MF_TOL, op
    ctx.close()


def test_a_refused_mesh_leaves_nothing_of_the_old_one(lib):
    before = lib.alloc_live()
    empty = lib.Context(0)
    no_mesh = tuple(x - y for x, y in zip(lib.alloc_live(), before))   # what a context holds that never had a mesh
    empty.close()
    ctx = _high_order_operators(lib)                         # mask, tables, both operators and two vectors of 10 x 10 nodes x 2 ...
    K = ctx.mat_create(2, 2)                                 # ... and a matrix
    ctx.assemble_kle(1e3, 1e2, K)
    floor = (before[0] + no_mesh[0] + 2, before[1] + no_mesh[1] + 2 * 100 * 2 * 8)
    mesh = fo.box_mesh([2, 2], [0.0, 0.0], [1.0, 1.0], 4)
    bad = mesh.conn.copy()
    bad[1, 3] = mesh.n_node
    with pytest.raises(lib.PynamaHipError, match="out of range"):
        ctx.mesh_set(2, bad, mesh.xyz)
    refused = lib.alloc_live()
    ctx.mesh_set(2, mesh.conn, mesh.xyz)
    installed = lib.alloc_live()
    assert refused[0] <= installed[0] and refused[1] <= installed[1]
    assert refused[0] >= floor[0] and refused[1] >= floor[1]
    ctx.close()
    assert lib.alloc_live() == before


@pytest.mark.parametrize("owner", [_rowrun_and_ho3_operator, _high_order_operators, _tet_patch_plans, _ibm_markers])
def test_reinstalling_over_every_owner_is_idempotent(lib, owner):
    ctx = owner(lib)
    mesh = q1_box(4)
    _install_q1(lib, ctx, mesh)
    first = lib.alloc_live()
    _install_q1(lib, ctx, mesh)
    assert lib.alloc_live() == first
    ctx.close()
