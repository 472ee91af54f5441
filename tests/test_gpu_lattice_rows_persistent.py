"""The walking form of the rows kernel of rectilinear lattices (assemble_q1_lattice_rows_walk_kernel): workgroups that walk x-lines by
lat_rows_sched (a workgroup per line by default; PYNAMA_LATTICE_ROWS_MAX_GRID makes the loop turn, -1: the persistent launch), the x
axis' pairs staged once per workgroup, and a word per line (class + end flags) that lets lines without interior Dirichlet nodes skip
every flag read.  No entry's formula changed, so the reference is the one-shot form of the same library
(PYNAMA_LATTICE_ROWS_ONESHOT=1, whose parity with the oracle tests/test_gpu_lattice_rows.py pins) and every comparison is bit for
bit: the values of A, of a full-pattern Arhs, and the 1/diagonal (through one Jacobi-PCG step, x = alpha D^-1 b, whose reductions
have a fixed order).  Every assembly runs with PYNAMA_LATTICE_ROWS_REQUIRE=1, and the record of what ran is checked each time: form 2
(walking) with the expected grid, form 1 for the reference."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from tests.test_gpu_lattice_rows import NELEM, graded_mesh, graded_xyz, jacobi_x, make_ctx, set_bc

pytestmark = pytest.mark.gpu

KNOBS = ("PYNAMA_LATTICE_ROWS_REQUIRE", "PYNAMA_LATTICE_ROWS_ONESHOT", "PYNAMA_LATTICE_ROWS_MAX_GRID", "PYNAMA_LATTICE_ROWS_NO_CLASSES", "PYNAMA_LATTICE_ROWS_LINES", "PYNAMA_LATTICE_ROWS_THREADS",
         "PYNAMA_NO_LATTICE_ROWS", "PYNAMA_NO_STD_LATTICE")
GRIDS = (1, 2, 3, None)               # PYNAMA_LATTICE_ROWS_MAX_GRID; None: not set (a workgroup per line)
SHAPES = ([1, 1, 1], [2, 1, 3], [3, 3, 1], [4, 4, 4], [70, 2, 2], [260, 1, 1])


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@contextmanager
def knobs(**kw):
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ["PYNAMA_LATTICE_ROWS_REQUIRE"] = "1"
        for k, v in kw.items():
            if v is not None:
                os.environ["PYNAMA_" + k] = str(v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def bits(ctx, lib, A, Arhs, n):
    out = [ctx.mat_values(A, 1, 1).view(np.int64).copy(), jacobi_x(lib, ctx, A, n)[1].view(np.int64).copy()]
    if Arhs is not None:
        out.append(ctx.mat_values(Arhs, 1, 1).view(np.int64).copy())
    return out


def assemble(lib, ctx, A, Arhs, n, form, n_lines=None, **kn):
    """one assembly under the switches kn -> the bits of A, 1/diagonal (and Arhs); the record must name the form (and the grid)"""
    with knobs(**kn):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1 if Arhs is None else Arhs)
        last = ctx.assemble_last()
        assert last["kind"] == lib.AK_LATTICE and last["shape"] == 0 and last["k_closed"] == 1 and last["dinv"] == 1, last
        assert last["rows_form"] == form, last
        if n_lines is not None:
            grid = kn.get("LATTICE_ROWS_MAX_GRID")
            if form == 1 or grid is None:
                assert last["rows_grid"] == n_lines, last
            elif grid > 0:
                assert last["rows_grid"] == min(grid, n_lines), last
            else:                                                    # -1: what the device holds at once
                assert 1 <= last["rows_grid"] <= n_lines, last
        return bits(ctx, lib, A, Arhs, n)


def same(got, want, what):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("A", "1/diagonal", "Arhs")):
        assert np.array_equal(g, w), f"{what}: {name} differs from the one-shot form in {np.count_nonzero(g != w)} of {g.size} values"


def node_sets(nelem):
    """name -> node ids (None: no Dirichlet set); node (x, y, z) is x + nx (y + ny z)"""
    nx, ny, nz = (n + 1 for n in nelem)
    ids = np.arange(nx * ny * nz)
    x, y, z = ids % nx, (ids // nx) % ny, ids // (nx * ny)
    faces = ids[(x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1) | (z == 0) | (z == nz - 1)]
    mid = lambda i: i + nx * (ny // 2 + ny * (nz // 2))   # on the middle line (an interior one where the lattice has any)
    return {"none": None, "faces": faces, "one face": ids[y == 0], "x face": ids[x == 0],
            "one interior node": np.array([mid(nx // 2)]), "x = 1 and x = nx - 2": np.unique([mid(1), mid(nx - 2)])}


@pytest.mark.parametrize("nelem", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_same_bits_as_the_one_shot_form(lib, nelem):
    """every shape under every Dirichlet set and every grid, on ONE context per shape (so the set, and with it the map of the lines,
    changes from assembly to assembly), each with a full-pattern Arhs where there is a set"""
    mesh = graded_mesh(nelem, upper=(1.0, 0.8, 1.1))
    n_lines = (nelem[1] + 1) * (nelem[2] + 1)
    ctx = make_ctx(lib, mesh)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    for name, nodes in node_sets(nelem).items():
        set_bc(ctx, mesh, nodes)
        R = None if nodes is None else Arhs
        want = assemble(lib, ctx, A, R, mesh.n_node, 1, n_lines, LATTICE_ROWS_ONESHOT=1)
        for grid in GRIDS:
            got = assemble(lib, ctx, A, R, mesh.n_node, 2, n_lines, LATTICE_ROWS_MAX_GRID=grid)
            same(got, want, f"{name}, grid {grid}")
    ctx.close()


def test_levers_one_by_one(lib):
    """the switches tools/lattice_rows_ab.py alternates: each variant of the persistent form writes the one-shot form's bits"""
    nelem = [4, 4, 4]
    mesh = graded_mesh(nelem)
    ctx = make_ctx(lib, mesh)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    for name, nodes in node_sets(nelem).items():
        if nodes is None:
            continue
        set_bc(ctx, mesh, nodes)
        want = assemble(lib, ctx, A, Arhs, mesh.n_node, 1, 25, LATTICE_ROWS_ONESHOT=1)
        for kn in ({"LATTICE_ROWS_MAX_GRID": -1}, {"LATTICE_ROWS_NO_CLASSES": 1}, {"LATTICE_ROWS_NO_CLASSES": 1, "LATTICE_ROWS_MAX_GRID": 2},
                   {"NO_STD_LATTICE": 1}, {"NO_STD_LATTICE": 1, "LATTICE_ROWS_MAX_GRID": 3}):
            same(assemble(lib, ctx, A, Arhs, mesh.n_node, 2, 25, **kn), want, f"{name}, {kn}")
    ctx.close()


def test_map_follows_the_dirichlet_set(lib):
    """faces -> one interior node -> faces on one context, grid 2: a stale map would keep the interior line in class 1 (its flag
    ignored) or the others in class 2; the Arhs target is not clean after every change (zeros must overwrite the old columns) and
    clean on the repeat"""
    nelem = [6, 4, 4]
    mesh = graded_mesh(nelem)
    sets = node_sets(nelem)
    ctx = make_ctx(lib, mesh)
    A, Arhs, B, Brhs = (ctx.mat_create(1, 1) for _ in range(4))
    for name in ("faces", "one interior node", "one interior node", "faces", "x = 1 and x = nx - 2", "x face", "faces"):
        set_bc(ctx, mesh, sets[name])
        want = assemble(lib, ctx, B, Brhs, mesh.n_node, 1, LATTICE_ROWS_ONESHOT=1)     # (its own targets: clean / not clean alike)
        got = assemble(lib, ctx, A, Arhs, mesh.n_node, 2, LATTICE_ROWS_MAX_GRID=2)
        same(got, want, name)
        assert np.any(got[2] != 0)
    ctx.close()


def test_rank_slabs_with_ghost_planes(lib):
    """a rank's z-slab: the ghost plane's lines are neighbours of the interface plane's.  Dirichlet faces, then a single node ON THE
    GHOST PLANE only -- at an interior x (class 2 for the interface lines next to it) and at x = 0 (class 1)"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    nelem = [9, 4, 5]
    xyz = graded_xyz(nelem)
    nx, ny = nelem[0] + 1, nelem[1] + 1
    for r in range(2):
        dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0, 0, 0], 'upper': [1, 1, 1]}, comm=Comm(r, 2))
        dom.setFemIndexing(2)
        cols = dom._local2global(np.arange(dom.nLocal))
        ctx = lib.Context(0)
        ctx.comm_init(r, 2, None)
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(3, dom.conn, xyz[cols])
        for t in Spectral(2, 3).deviceTables():
            ctx.tables_set(*t)
        ctx.bc_set(1, dom.boundaryMaskLocal())
        ctx.csr_symbolic()
        n_own = (dom.rEnd - dom.rStart) // (nx * ny)
        assert ctx.mesh_topology() == ("lattice", nx, ny, n_own + 1)
        ghost0 = n_own * nx * ny                                  # the ghost plane's ids follow the owned ones
        masks = [dom.boundaryMaskLocal()]
        for x in (4, 0):
            m = np.zeros((dom.nLocal, 1), np.uint8)
            m[ghost0 + 2 * nx + x] = 1
            masks.append(m)
        A, Ar = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
        n = dom.rEnd - dom.rStart
        for m in masks:
            ctx.bc_set(1, m)
            with knobs(LATTICE_ROWS_ONESHOT=1):
                ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)
                assert ctx.assemble_last()["rows_form"] == 1
                want = [ctx.mat_values(A, 1, 1).copy(), ctx.mat_values(Ar, 1, 1).copy()]
            for grid in (3, None):
                with knobs(LATTICE_ROWS_MAX_GRID=grid):
                    ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)
                    assert ctx.assemble_last()["rows_form"] == 2
                    got = [ctx.mat_values(A, 1, 1), ctx.mat_values(Ar, 1, 1)]
                for g, w in zip(got, want):
                    assert np.array_equal(g.view(np.int64), w.view(np.int64))
        assert n == n_own * nx * ny
        ctx.close()


def test_mesh_replaced_on_the_same_context(lib):
    """another lattice on the same context under the SAME Dirichlet stamp history: the map of the first mesh's lines must not survive"""
    from pynama_amd.elements.spectral import Spectral
    first = graded_mesh([5, 3, 3])
    ctx = make_ctx(lib, first, bc_nodes=node_sets([5, 3, 3])["one interior node"])
    A = ctx.mat_create(1, 1)
    assemble(lib, ctx, A, None, first.n_node, 2, LATTICE_ROWS_MAX_GRID=2)
    nelem = [6, 4, 2]
    mesh = graded_mesh(nelem, (1.75, 1.5, 1.25), (1.0, 0.8, 1.1))
    ctx.mesh_set(3, mesh.conn, mesh.xyz)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    set_bc(ctx, mesh, mesh.boundary)
    ctx.csr_symbolic()
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    got = assemble(lib, ctx, A, Arhs, mesh.n_node, 2, 15, LATTICE_ROWS_MAX_GRID=2)
    same(got, assemble(lib, ctx, A, Arhs, mesh.n_node, 1, 15, LATTICE_ROWS_ONESHOT=1), "second mesh")
    ctx.close()


def test_the_record_names_the_walking_form(lib):
    """by default the walking form runs, not the tile kernel and not the one-shot form, and the record says with which grid"""
    mesh = graded_mesh(NELEM)
    ctx = make_ctx(lib, mesh)
    A = ctx.mat_create(1, 1)
    n_lines = (NELEM[1] + 1) * (NELEM[2] + 1)
    with knobs():
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
        last = ctx.assemble_last()
    assert (last["kind"], last["shape"], last["rows_form"], last["rows_grid"]) == (lib.AK_LATTICE, 0, 2, n_lines), last
    with knobs(LATTICE_ROWS_MAX_GRID=5):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
        assert ctx.assemble_last()["rows_grid"] == 5
    with knobs(LATTICE_ROWS_ONESHOT=1):
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
        assert (ctx.assemble_last()["rows_form"], ctx.assemble_last()["rows_grid"]) == (1, n_lines)
    with knobs(NO_LATTICE_ROWS=1, LATTICE_ROWS_REQUIRE=None):
        os.environ.pop("PYNAMA_LATTICE_ROWS_REQUIRE")
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
        assert ctx.assemble_last()["rows_form"] == 0 and ctx.assemble_last()["kind"] == lib.AK_LATTICE
    ctx.close()
