"""The axis-table variant of the parallelepiped lattice tile kernel (assemble_q1_hex_lattice_kernel<.., AFF, AX>): on a RECTILINEAR
lattice -- node (i, j, k) at (X[i], Y[j], Z[k]) bit for bit -- an element's corners are six numbers out of three short tables read
through the scalar cache, not four coordinate loads.  Checked here: the matrix, Arhs and 1/diagonal against the oracle and, entry by
entry, against the coordinate-loading kernel of the same library (PYNAMA_NO_LATTICE_AXES); three tile shapes; the detector (one ulp,
a sheared lattice, a mesh replaced on the same context); a rank's z-slab; the per-tile Dirichlet map (a tile whose bit is clear
loads no flag bytes) across a change of the Dirichlet set.  PYNAMA_LATTICE_AXES_REQUIRE makes an assembly that would
load coordinates an error, so no case can compare the old path with itself.

Mesh: 17 x 13 x 11 elements = 18 x 14 x 12 nodes, graded differently per axis (an index slip in any table changes the matrix; a
uniform box would hide it).  With the default 7 x 5 x 4 tile it has exactly one plain tile and 26 tiles on faces, the last tile in x
and z is partial, and the guard entries of the tables are read on all six faces."""
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
KNOBS = ("PYNAMA_LATTICE_AXES_REQUIRE", "PYNAMA_NO_LATTICE_AXES", "PYNAMA_NO_LATTICE_TILEBC", "PYNAMA_LATTICE_TILE")


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


@pytest.fixture(scope="module")
def graded():
    """the mesh and the oracle's matrices with Dirichlet faces: computed once, shared, never modified (tests copy xyz)"""
    mesh = fo.box_mesh(NELEM, [0, 0, 0], [1, 1, 1], 2)
    mesh.xyz = graded_xyz(NELEM)
    ref = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=mesh.boundary)
    return mesh, ref


def make_ctx(lib, mesh, xyz=None, bc_nodes=None):
    from pynama_amd.elements.spectral import Spectral
    ctx = lib.Context(0)
    ctx.mesh_set(3, mesh.conn, mesh.xyz if xyz is None else xyz)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    mask = np.zeros((mesh.n_node, 1), np.uint8)
    mask[mesh.boundary if bc_nodes is None else bc_nodes] = 1
    ctx.bc_set(1, mask)
    ctx.csr_symbolic()
    return ctx


def ulps(a, b):
    """largest distance of two float64 arrays in units in the last place"""
    def ordered(v):
        i = np.ascontiguousarray(v, np.float64).view(np.int64)
        return np.where(i < 0, np.iinfo(np.int64).min - i, i)
    return int(np.abs(ordered(a) - ordered(b)).max())


def jacobi_step(lib, ctx, A, ref_A, seed=3):
    """one Jacobi-PCG iteration from x = 0 is x = alpha D^-1 b: every entry of the 1/diagonal the assembly wrote, against the oracle"""
    n = ref_A.shape[0]
    b = np.random.default_rng(seed).standard_normal(n)
    vb, vx = ctx.vec_create(1), ctx.vec_create(1)
    ctx.vec_set(vb, b)
    ctx.solve(A, vb, vx, method=lib.KSP_CG, pc=lib.PC_JACOBI, fixed_iters=1)
    z = b / ref_A.diagonal()
    return rel_err(ctx.vec_get(vx, 1), (b @ z) / (z @ (ref_A @ z)) * z)


@pytest.mark.parametrize("tile", [0, 3, 8])      # 7x5x4 (default), 8x6x6 (two elements per lane), 14x3x3: every extent differs
def test_axis_tables_equal_oracle_and_coordinate_loads(lib, graded, tile):
    mesh, ref = graded
    ctx = make_ctx(lib, mesh)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    with knobs(LATTICE_AXES_REQUIRE=1, LATTICE_TILE=tile):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
        assert_assembled(ctx, lib.AK_LATTICE, shape=tile, k_closed=1, dinv=1)
        e_A = sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"])
        e_R = sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"])
        e_D = jacobi_step(lib, ctx, A, ref["A"])
        v_new, r_new = ctx.mat_values(A, 1, 1), ctx.mat_values(Arhs, 1, 1)
    old = []
    with knobs(NO_LATTICE_AXES=1, LATTICE_TILE=tile):
        for _ in range(2):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
            assert_assembled(ctx, lib.AK_LATTICE, shape=tile, k_closed=1, dinv=1)
            old.append((ctx.mat_values(A, 1, 1), ctx.mat_values(Arhs, 1, 1)))
    ctx.close()
    d_new = max(ulps(v_new, old[0][0]), ulps(r_new, old[0][1]))
    d_self = max(ulps(old[1][0], old[0][0]), ulps(old[1][1], old[0][1]))
    print(f"tile {tile}: A {e_A:.2e}  Arhs {e_R:.2e}  1/diag {e_D:.2e} against the oracle; tables against coordinate loads "
          f"{d_new} ulp, coordinate loads twice {d_self} ulp")
    assert e_A < FP_TOL and e_R < FP_TOL and e_D < FP_TOL
    # the element matrices are the same bits by construction; the LDS sums may depend on the order of the adds (measured on an
    # MI355X, all three tiles: 2 ulp against the coordinate loads, 2 ulp between two runs of the coordinate loads)
    assert d_new <= d_self


def assemble_declined(lib, mesh, xyz, ref):
    """a mesh the detector must decline: an error under REQUIRE, the coordinate-loading kernels and the oracle's matrix without"""
    ctx = make_ctx(lib, mesh, xyz)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    with knobs(LATTICE_AXES_REQUIRE=1):
        with pytest.raises(Exception, match="PYNAMA_LATTICE_AXES_REQUIRE"):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
    with knobs():
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"]) < FP_TOL
    return ctx


def test_one_ulp_off_the_lattice_declines(lib, graded):
    mesh, ref = graded
    xyz = mesh.xyz.copy()
    nx, ny = NELEM[0] + 1, NELEM[1] + 1
    node = (5 * ny + 6) * nx + 8                             # interior, inside the plain tile
    xyz[node, 1] = np.nextafter(xyz[node, 1], 2.0)
    # (whether the eight cells around the node still count as parallelepipeds is the affine check's tolerance to decide: either way
    # the table variant must not run)
    assemble_declined(lib, mesh, xyz, ref).close()


def test_sheared_lattice_declines(lib):
    M = np.array([[1.0, 0.3, -0.2], [0.1, 0.9, 0.25], [-0.15, 0.2, 1.1]])
    box = fo.box_mesh(NELEM, [0, 0, 0], [1.0, 0.8, 1.1], 2)
    box.xyz = box.xyz @ M.T + np.array([0.5, -1.0, 2.0])    # parallelepipeds, not axis-aligned
    ref = fo.assemble_scalar(box, fo.Tables(2, 3), "laplace", dirichlet=box.boundary)
    ctx = assemble_declined(lib, box, box.xyz, ref)
    assert_assembled(ctx, lib.AK_LATTICE, shape=0, k_closed=1)    # still the closed form, with coordinate loads
    ctx.close()


def test_mesh_replaced_on_the_same_context(lib, graded):
    """the tables belong to the coordinates they were read from: a second pyn_mesh_set runs the check again"""
    from pynama_amd.elements.spectral import Spectral
    mesh, ref = graded
    ctx = make_ctx(lib, mesh)
    A = ctx.mat_create(1, 1)
    with knobs(LATTICE_AXES_REQUIRE=1):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]) < FP_TOL
    # same topology, other axes: stale tables would reproduce the first matrix
    xyz2 = graded_xyz(NELEM, (1.75, 1.5, 1.25), (1.0, 0.8, 1.1))
    mesh2 = fo.box_mesh(NELEM, [0, 0, 0], [1, 1, 1], 2)
    mesh2.xyz = xyz2
    ref2 = fo.assemble_scalar(mesh2, fo.Tables(2, 3), "laplace", dirichlet=mesh2.boundary)
    ctx.mesh_set(3, mesh2.conn, xyz2)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    mask = np.zeros((mesh2.n_node, 1), np.uint8)
    mask[mesh2.boundary] = 1
    ctx.bc_set(1, mask)
    ctx.csr_symbolic()
    A = ctx.mat_create(1, 1)
    with knobs(LATTICE_AXES_REQUIRE=1):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
    assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref2["A"]) < FP_TOL
    # ... and a sheared mesh after a rectilinear one declines
    xyz3 = mesh.xyz @ np.array([[1.0, 0.2, 0.0], [0.0, 1.0, 0.1], [0.0, 0.0, 1.0]]).T
    ctx.mesh_set(3, mesh.conn, xyz3)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    ctx.bc_set(1, mask)
    ctx.csr_symbolic()
    A = ctx.mat_create(1, 1)
    with knobs(LATTICE_AXES_REQUIRE=1):
        with pytest.raises(Exception, match="PYNAMA_LATTICE_AXES_REQUIRE"):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
    ctx.close()


def test_rank_slabs(lib, graded):
    """12 node planes cut in two: each rank's slab has a ghost plane (above for rank 0, below for rank 1) whose ids follow the owned
    ones, so Z must be indexed by the plane's position in the slab (lat_plane), not by its id.  Owned rows == the serial rows."""
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
        with knobs(LATTICE_AXES_REQUIRE=1):
            ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)
            assert_assembled(ctx, lib.AK_LATTICE, shape=0, k_closed=1)
        assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        assert sp_rel_err(mat_to_scipy(ctx, Ar, 1, 1), ref["Arhs"][dom.rStart:dom.rEnd][:, cols]) < FP_TOL
        ctx.close()


def test_dirichlet_set_changes_between_assemblies(lib, graded):
    """the per-tile map belongs to ONE Dirichlet set: faces only (the plain tile's bit is clear: no flag loads), then one interior
    node imposed inside the plain tile (its bit must be set now), back, then no Dirichlet set at all.  The oracle's matrices every
    time."""
    mesh, ref = graded
    nx, ny = NELEM[0] + 1, NELEM[1] + 1
    inner = (5 * ny + 7) * nx + 9                            # node (9, 7, 5): rows x 7..13, y 5..9, z 4..7 are the plain tile
    assert inner not in mesh.boundary
    more = np.sort(np.append(mesh.boundary, inner))
    ref2 = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace", dirichlet=more)
    ref0 = fo.assemble_scalar(mesh, fo.Tables(2, 3), "laplace")
    assert abs(ref2["A"] - ref["A"]).max() > 1e-3            # (the sets give different matrices: a stale map would show)
    ctx = make_ctx(lib, mesh)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    for nodes, want in ((mesh.boundary, ref), (more, ref2), (mesh.boundary, ref), (None, ref0)):
        if nodes is None:
            ctx.bc_set(1, None)
        else:
            mask = np.zeros((mesh.n_node, 1), np.uint8)
            mask[nodes] = 1
            ctx.bc_set(1, mask)
        for off in ({}, {"NO_LATTICE_TILEBC": 1}):          # with the map, and with the flag loads in every tile
            with knobs(LATTICE_AXES_REQUIRE=1, **off):
                ctx.assemble_scalar(lib.FORM_LAPLACE, A, Arhs if nodes is not None else -1)
                assert_assembled(ctx, lib.AK_LATTICE, shape=0, k_closed=1, dinv=1)
            assert sp_rel_err(mat_to_scipy(ctx, A, 1, 1), want["A"]) < FP_TOL
            if nodes is not None:
                assert sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), want["Arhs"]) < FP_TOL
            assert jacobi_step(lib, ctx, A, want["A"]) < FP_TOL
    ctx.close()
