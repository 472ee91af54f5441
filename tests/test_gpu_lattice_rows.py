"""The rows kernel of rectilinear lattices (assemble_q1_lattice_rows_kernel): every CSR entry is Kx[x][dx] a[dy][dz] + Mx[x][dx] b[dy][dz]
out of the 1-D P1 stiffness / mass tables of the three axes, one x-line's rows written as the one contiguous run they are.  Checked
here against the oracle: the matrix, Arhs and 1/diagonal on a graded mesh under four Dirichlet sets, the decode at the smallest and
at awkward lattice shapes, bit-reproducibility, a rank's z-slabs, a mesh replaced on the same context, and the switches.  Every
assembly under test runs with PYNAMA_LATTICE_ROWS_REQUIRE=1, which makes any other kernel an error.

Mesh: 17 x 13 x 11 elements = 18 x 14 x 12 nodes, graded differently per axis (an index slip in any table changes the matrix; a
uniform box would hide it)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.util import assert_assembled, mat_to_scipy, rel_err, sp_rel_err

pytestmark = pytest.mark.gpu

FP_TOL = 2e-13                        # the project's bar for FP64 sums in another order (tests/test_gpu_kernels.py)
NELEM = [17, 13, 11]
GRADING = (1.5, 1.25, 1.75)
KNOBS = ("PYNAMA_LATTICE_ROWS_REQUIRE", "PYNAMA_NO_LATTICE_ROWS", "PYNAMA_LATTICE_AXES_REQUIRE", "PYNAMA_NO_LATTICE_AXES",
         "PYNAMA_NO_LATTICE_TILEBC", "PYNAMA_LATTICE_TILE", "PYNAMA_NO_ASM_DINV")


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@contextmanager
def knobs(**kw):
    """the assembly switches are read per assembly call: set for the block, restored after it"""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in kw.items():
            os.environ["PYNAMA_" + k] = str(v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def graded_xyz(nelem, grading=GRADING, upper=(1.0, 1.0, 1.0)):
    """node (i, j, k) at (X[i], Y[j], Z[k]) with X_i = upper (i / n)^p: every coordinate is COPIED from a 1-D table, so equal bit
    for bit along every lattice line"""
    lat = [n + 1 for n in nelem]
    ax = [upper[d] * (np.arange(lat[d]) / nelem[d]) ** grading[d] for d in range(3)]
    ids = np.arange(lat[0] * lat[1] * lat[2])
    return np.stack([ax[0][ids % lat[0]], ax[1][(ids // lat[0]) % lat[1]], ax[2][ids // (lat[0] * lat[1])]], axis=1)


def graded_mesh(nelem, grading=GRADING, upper=(1.0, 1.0, 1.0)):
    mesh = fo.box_mesh(list(nelem), [0, 0, 0], [1, 1, 1], 2)
    mesh.xyz = graded_xyz(nelem, grading, upper)
    return mesh


def oracle(mesh, nodes):
    """nodes None: no Dirichlet set"""
    if nodes is None:
        return fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace")
    return fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=nodes)


@pytest.fixture(scope="module")
def graded():
    """the mesh and the oracle's matrices with Dirichlet faces: computed once, shared, never modified (tests copy xyz)"""
    mesh = graded_mesh(NELEM)
    return mesh, oracle(mesh, mesh.boundary)


def set_bc(ctx, mesh, nodes):
    if nodes is None:
        ctx.bc_set(1, None)
        return
    mask = np.zeros((mesh.n_node, 1), np.uint8)
    mask[nodes] = 1
    ctx.bc_set(1, mask)


def make_ctx(lib, mesh, xyz=None, bc_nodes="faces"):
    from pynama_amd.elements.spectral import Spectral
    ctx = lib.Context(0)
    ctx.mesh_set(3, mesh.conn, mesh.xyz if xyz is None else xyz)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    set_bc(ctx, mesh, mesh.boundary if isinstance(bc_nodes, str) else bc_nodes)
    ctx.csr_symbolic()
    return ctx


def jacobi_x(lib, ctx, A, n, seed=3):
    """one Jacobi-PCG iteration from x = 0 is x = alpha D^-1 b: every entry of the 1/diagonal the assembly wrote"""
    b = np.random.default_rng(seed).standard_normal(n)
    vb, vx = ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vb, b)
    ctx.solve(A, vb, vx, method=lib.KSP_CG, pc=lib.PC_JACOBI, fixed_iters=1)
    return b, ctx.vec_get(vx, 1)


def jacobi_step(lib, ctx, A, ref_A, seed=3):
    b, x = jacobi_x(lib, ctx, A, ref_A.shape[0], seed)
    z = b / ref_A.diagonal()
    return rel_err(x, (b @ z) / (z @ (ref_A @ z)) * z)


def check_against(lib, ctx, A, Arhs, want, dinv=1, **kn):
    """assemble with the rows kernel REQUIRED (Arhs None: not asked for) and compare A, Arhs and the 1/diagonal with the oracle"""
    with knobs(LATTICE_ROWS_REQUIRE=1, **kn):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1 if Arhs is None else Arhs)
        assert_assembled(ctx, lib.AK_LATTICE, shape=0, k_closed=1, dinv=dinv)
        e_A = sp_rel_err(mat_to_scipy(ctx, A, 1, 1), want["A"])
        e_R = 0.0 if Arhs is None else sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), want["Arhs"])
        e_D = jacobi_step(lib, ctx, A, want["A"])
    print(f"A {e_A:.2e}  Arhs {e_R:.2e}  1/diag {e_D:.2e} against the oracle")
    assert e_A < FP_TOL and e_R < FP_TOL and e_D < FP_TOL


def test_graded_mesh_equals_oracle_under_changing_dirichlet_sets(lib, graded):
    """faces, no set, a random interior set of n/7 nodes, faces again -- all on ONE context, so the set changes between assemblies;
    each with Arhs, without Arhs, and without the 1/diagonal (PYNAMA_NO_ASM_DINV: the separate diagonal pass must see the same matrix)"""
    mesh, ref = graded
    interior = np.setdiff1d(np.arange(mesh.n_node), mesh.boundary)
    inner = np.sort(np.random.default_rng(11).choice(interior, mesh.n_node // 7, replace=False))
    ctx = make_ctx(lib, mesh)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    for nodes, want in ((mesh.boundary, ref), (None, oracle(mesh, None)), (inner, oracle(mesh, inner)), (mesh.boundary, ref)):
        set_bc(ctx, mesh, nodes)
        if nodes is not None:
            check_against(lib, ctx, A, Arhs, want)
        check_against(lib, ctx, A, None, want)
        check_against(lib, ctx, A, Arhs if nodes is not None else None, want, dinv=0, NO_ASM_DINV=1)
    ctx.close()


@pytest.mark.parametrize("nelem", [[1, 1, 1], [2, 1, 3], [1, 5, 2], [3, 3, 1], [70, 2, 2]], ids=lambda n: "x".join(map(str, n)))
def test_decode_edge_shapes(lib, nelem):
    """[1,1,1]: nx = 2, every row a face row in every direction; [70,2,2]: a run (9 * 211 = 1899 values on the inner line) longer than
    one pass of the workgroup and no multiple of 64.  With the faces imposed and without a Dirichlet set."""
    mesh = graded_mesh(nelem, upper=(1.0, 0.8, 1.1))
    ctx = make_ctx(lib, mesh)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    check_against(lib, ctx, A, Arhs, oracle(mesh, mesh.boundary))
    set_bc(ctx, mesh, None)
    check_against(lib, ctx, A, None, oracle(mesh, None))
    ctx.close()


def test_two_assemblies_give_identical_bits(lib, graded):
    mesh, ref = graded
    inner = np.sort(np.random.default_rng(5).choice(mesh.n_node, mesh.n_node // 7, replace=False))
    ctx = make_ctx(lib, mesh, bc_nodes=inner)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    got = []
    with knobs(LATTICE_ROWS_REQUIRE=1):
        for _ in range(2):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
            assert_assembled(ctx, lib.AK_LATTICE, shape=0, k_closed=1, dinv=1)
            # (the solver's reductions have a fixed order: x = alpha D^-1 b repeats bit for bit iff the 1/diagonal does)
            got.append((ctx.mat_values(A, 1, 1), ctx.mat_values(Arhs, 1, 1), jacobi_x(lib, ctx, A, mesh.n_node)[1]))
    ctx.close()
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.abs(got[0][1]).max() > 0


def test_rank_slabs(lib, graded):
    """12 node planes cut in two: each rank's slab has a ghost plane (above for rank 0, below for rank 1) whose ids follow the owned
    ones, so the z tables must be indexed by the plane's position in the slab and the interface planes must get their ghost-side
    terms.  Owned rows == the serial rows."""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    mesh, ref = graded
    size = 2
    for r in range(size):
        dom = DMPlexDom(boxMesh={'nelem': NELEM, 'lower': [0, 0, 0], 'upper': [1, 1, 1]}, comm=Comm(r, size))
        dom.setFemIndexing(2)
        cols = dom._local2global(np.arange(dom.nLocal))
        ctx = lib.Context(0)
        ctx.comm_init(r, size, None)
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(3, dom.conn, mesh.xyz[cols])
        for t in Spectral(2, 3).deviceTables():
            ctx.tables_set(*t)
        ctx.bc_set(1, dom.boundaryMaskLocal())
        ctx.csr_symbolic()
        assert ctx.mesh_topology() == ("lattice", 18, 14, dom.nLocal // (18 * 14))
        A, Ar = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
        with knobs(LATTICE_ROWS_REQUIRE=1):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)
            assert_assembled(ctx, lib.AK_LATTICE, shape=0, k_closed=1)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Ar, 1, 1), ref["Arhs"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        ctx.close()


def test_mesh_replaced_on_the_same_context(lib, graded):
    """the 1-D tables belong to the coordinates they were built from: same topology, other gradings -- stale tables would
    reproduce the first matrix"""
    from pynama_amd.elements.spectral import Spectral
    mesh, ref = graded
    ctx = make_ctx(lib, mesh)
    A = ctx.mat_create(1, 1)
    check_against(lib, ctx, A, None, ref)
    mesh2 = graded_mesh(NELEM, (1.75, 1.5, 1.25), (1.0, 0.8, 1.1))
    ref2 = oracle(mesh2, mesh2.boundary)
    assert sp_rel_err(ref2["A"], ref["A"]) > 1e-3
    ctx.mesh_set(3, mesh2.conn, mesh2.xyz)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    set_bc(ctx, mesh2, mesh2.boundary)
    ctx.csr_symbolic()
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    check_against(lib, ctx, A, Arhs, ref2)
    ctx.close()


def declined(lib, mesh, xyz, ref, closed=True, **kn):
    """an assembly the rows kernel must decline: an error under REQUIRE, the tile kernel and the oracle's matrix without"""
    ctx = make_ctx(lib, mesh, xyz)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    with knobs(LATTICE_ROWS_REQUIRE=1, **kn):
        with pytest.raises(Exception, match="PYNAMA_LATTICE_ROWS_REQUIRE"):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
    with knobs(**kn):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
        if closed:
            assert_assembled(ctx, lib.AK_LATTICE, shape=int(kn.get("LATTICE_TILE", 0)), k_closed=1)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    assert jacobi_step(lib, ctx, A, ref["A"]) < FP_TOL
    ctx.close()


def test_sheared_lattice_declines(lib):
    M = np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]])
    box = fo.box_mesh(NELEM, [0, 0, 0], [1.0, 0.8, 1.1], 2)
    box.xyz = box.xyz @ M.T + np.array([0.5, -1.0, 2.0])    # parallelepipeds, not axis-aligned
    declined(lib, box, box.xyz, oracle(box, box.boundary))


def test_one_ulp_off_the_lattice_declines(lib, graded):
    mesh, ref = graded
    xyz = mesh.xyz.copy()
    nx, ny = NELEM[0] + 1, NELEM[1] + 1
    node = (5 * ny + 6) * nx + 8                             # an interior node
    xyz[node, 1] = np.nextafter(xyz[node, 1], 2.0)
    # (whether the eight cells around the node still count as parallelepipeds is the affine check's tolerance to decide: either way
    # the rows kernel must not run)
    declined(lib, mesh, xyz, ref, closed=False)


def test_tile_request_declines(lib, graded):
    mesh, ref = graded
    declined(lib, mesh, None, ref, LATTICE_TILE=3)


def test_switched_off_gives_the_tile_kernels_matrix(lib, graded):
    mesh, ref = graded
    ctx = make_ctx(lib, mesh)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    with knobs(NO_LATTICE_ROWS=1, LATTICE_ROWS_REQUIRE=1):
        with pytest.raises(Exception, match="PYNAMA_LATTICE_ROWS_REQUIRE"):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
    with knobs(NO_LATTICE_ROWS=1, LATTICE_AXES_REQUIRE=1):     # ... the table variant of the tile kernel, as before
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
        assert_assembled(ctx, lib.AK_LATTICE, shape=0, k_closed=1, dinv=1)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    assert jacobi_step(lib, ctx, A, ref["A"]) < FP_TOL
    ctx.close()
