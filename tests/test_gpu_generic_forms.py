"""What the generic assembly kernels COMPUTE in every launch form (generic_pick, pynama_amd/csrc/pyn_assemble.hip), on cells whose
Jacobian varies from point to point, against the CPU oracle.  The rows are those of tests/generic_forms_cases.py (proved to reach
their form on the host by tests/test_generic_forms_host.py); every assembly asserts the form that ran, so a threshold that moves
cannot move a case onto another form.  All assemblies use variant=0: no lattice or row-run kernel is eligible.  (The operator rows
sit above ngl 3 and on bent cells, where the row-run view declines by itself: PYNAMA_NO_HO3_OPERATOR is not needed.)

Every free-slip and scalar case runs with two Dirichlet sets: the mesh boundary, and the boundary plus a few random interior nodes;
for KLE the second set is a per-DOF mask with nodes that have one component imposed only, where the ci / cj routing of the staged
and the matrix-core scatter differs per component.  The oracle's assemble_kle_freeslip takes node sets, so the per-DOF reference is
assembled here from fo.elem_kle_matrices with the same elimination rule.  The element matrices of a mesh are evaluated once per
module (3-D ngl 5 and 6 cost seconds) and shared by the forms and the Dirichlet sets.

Tolerance: FP_TOL = 2e-13 of the reference's largest entry, the project's bound for FP64 sums in another order.  Measured on an
MI355X: every matrix of every row lands between 4e-16 and 1.1e-14 (largest: Krhs of the 2-D ngl 12 mesh), so no case needs another
bound; each test prints its figures (-s)."""
import contextlib
import functools
import os
from concurrent.futures import ThreadPoolExecutor
from unittest import mock

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import fem_oracle as fo
from tests import generic_forms_cases as gc
from tests import ho_general_meshes as gm
from tests.test_gpu_kernels import FP_TOL, make_ctx
from tests.util import assert_assembled, mat_to_scipy, rel_err, sp_rel_err

pytestmark = pytest.mark.gpu

ALPHA = (1e3, 1e2)


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@contextlib.contextmanager
def switches(form):
    """the environment switches (read per assembly) that take a stageable KLE assembly to `form`"""
    names = ["PYNAMA_" + k.upper() for k in gc.KLE_KNOBS[form]]
    assert not any(n in os.environ for n in ("PYNAMA_NO_HO", "PYNAMA_NO_HO_MFMA"))
    for n in names:
        os.environ[n] = "1"
    try:
        yield
    finally:
        for n in names:
            os.environ.pop(n, None)


def block_shapes(dim):
    dw = 1 if dim == 2 else 3
    return {"K": (dim, dim), "Krhs": (dim, dim), "Rw": (dim, dw), "Rd": (dim, 1)}


# ---- references, once per module ---------------------------------------------------------------------------------------------------
_ELEM = {}


def elem_matrices(spec):
    """(K_e, Rw_e, Rd_e) of every cell of a table mesh from the oracle, cell by cell"""
    if spec not in _ELEM:
        mesh = gc.mesh_of(spec)
        tb, X = gm.tables(mesh.ngl, mesh.dim), mesh.corners()
        with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
            parts = list(ex.map(lambda e: fo.elem_kle_matrices(tb, X[e:e + 1], *ALPHA), range(mesh.n_elem)))
        _ELEM[spec] = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    return _ELEM[spec]


@functools.lru_cache(maxsize=None)
def ref_boundary(spec):
    """fo.assemble_kle_freeslip on the mesh boundary, its element matrices taken from the module's one evaluation"""
    mesh = gc.mesh_of(spec)
    mats = elem_matrices(spec)          # (evaluated BEFORE the name is patched: elem_matrices calls the oracle's function itself)
    with mock.patch.object(fo, "elem_kle_matrices", lambda tb, coords, alpha_d, alpha_w: mats):
        return fo.assemble_kle_freeslip(mesh, gm.tables(mesh.ngl, mesh.dim), *ALPHA, with_rd=True)


def ref_masked(spec, mask):
    """K, Krhs, Rw, Rd with a per-DOF mask [n_node, dim]: the lines of fo.assemble_kle_freeslip with is_bc per DOF (imposed rows
    dropped and set to identity in K and Krhs, imposed columns of free rows moved to Krhs with the opposite sign)"""
    mesh = gc.mesh_of(spec)
    dim, dw, n = mesh.dim, 1 if mesh.dim == 2 else 3, mesh.n_node
    Ke, Rwe, Rde = elem_matrices(spec)
    vdof, wdof = fo.dof_indices(mesh.conn, dim), fo.dof_indices(mesh.conn, dw)
    is_bc = np.asarray(mask, bool).reshape(-1)
    rfree, cbc = ~is_bc[vdof], is_bc[vdof]
    R, C = np.broadcast_to(vdof[:, :, None], Ke.shape), np.broadcast_to(vdof[:, None, :], Ke.shape)
    mff, mfb = rfree[:, :, None] & rfree[:, None, :], rfree[:, :, None] & cbc[:, None, :]
    bc_idx = np.nonzero(is_bc)[0]
    ident = sp.coo_matrix((np.ones(len(bc_idx)), (bc_idx, bc_idx)), shape=(n * dim, n * dim)).tocsr()
    out = {"K": (fo._scatter((n * dim, n * dim), R[mff], C[mff], Ke[mff]) + ident).tocsr(),
           "Krhs": (fo._scatter((n * dim, n * dim), R[mfb], C[mfb], -Ke[mfb]) + ident).tocsr()}
    mrow = np.broadcast_to(rfree[:, :, None], Rwe.shape)
    out["Rw"] = fo._scatter((n * dim, n * dw), np.broadcast_to(vdof[:, :, None], Rwe.shape)[mrow],
                            np.broadcast_to(wdof[:, None, :], Rwe.shape)[mrow], Rwe[mrow])
    mrow = np.broadcast_to(rfree[:, :, None], Rde.shape)
    out["Rd"] = fo._scatter((n * dim, n), np.broadcast_to(vdof[:, :, None], Rde.shape)[mrow],
                            np.broadcast_to(mesh.conn[:, None, :], Rde.shape)[mrow], Rde[mrow])
    return out


def extra_nodes(mesh):
    """a few random nodes off the boundary"""
    inner = np.setdiff1d(np.arange(mesh.n_node), mesh.boundary)
    return np.random.default_rng(3).choice(inner, min(6, len(inner)), replace=False)


def partial_mask(mesh):
    """the boundary, a few interior nodes with every component imposed, a few with ONE component imposed, and a few boundary nodes
    with one component left free"""
    rng = np.random.default_rng(4)
    mask = gm.boundary_mask(mesh)
    pick = extra_nodes(mesh)
    half = len(pick) // 2
    mask[pick[:half]] = 1
    mask[pick[half:], rng.integers(mesh.dim, size=len(pick) - half)] = 1
    wall = rng.choice(mesh.boundary, 3, replace=False)
    mask[wall, rng.integers(mesh.dim, size=3)] = 0
    return mask


def kle_sets(spec):
    """(name, per-DOF mask, reference) of the two Dirichlet sets"""
    mesh = gc.mesh_of(spec)
    pm = partial_mask(mesh)
    return [("boundary", gm.boundary_mask(mesh), ref_boundary(spec)), ("partial", pm, ref_masked(spec, pm))]


# ---- one assembly and what is asserted of it -----------------------------------------------------------------------------------------
def assemble_kle(lib, ctx, dim, targets, form, mats=None):
    """pyn_assemble_kle(variant=0) of `targets` under the switches of `form`; asserts the form that ran.  Returns the matrix ids."""
    shapes = block_shapes(dim)
    mats = mats or {t: ctx.mat_create(*shapes[t]) for t in targets}
    with switches(form):
        ctx.assemble_kle(*ALPHA, *[mats.get(t, -1) for t in gc.ALL4], variant=0)
    assert_assembled(ctx, lib.AK_GENERIC, generic=form, krhs_completed=0, dinv=0)
    return mats


def assert_symmetric_free_block(K, mask):
    free = ~np.asarray(mask, bool).reshape(-1)
    Kff = K[free][:, free]
    asym = abs(Kff - Kff.T)
    assert (asym.max() if asym.nnz else 0.0) <= 1e-12 * abs(Kff).max()


def check_kle(lib, ctx, spec, form, targets, mask, ref, label):
    """assembly == reference to FP_TOL; a second assembly into the same matrices gives the same values to 1e-14 (no stale scratch
    or LDS); K is symmetric on its free-free block"""
    dim = len(spec[1])
    shapes = block_shapes(dim)
    ctx.bc_set(dim, mask)
    mats = assemble_kle(lib, ctx, dim, targets, form)
    first = {t: ctx.mat_values(mats[t], *shapes[t]) for t in targets}
    errs = {t: sp_rel_err(mat_to_scipy(ctx, mats[t], *shapes[t]), ref[t]) for t in targets}
    print(f"{gc.tag(spec)} form {form} {label}: " + " ".join(f"{t} {e:.2e}" for t, e in errs.items()))
    for t in targets:
        assert errs[t] < FP_TOL, (label, t, errs[t])
    assert_symmetric_free_block(mat_to_scipy(ctx, mats["K"], dim, dim), mask)
    assemble_kle(lib, ctx, dim, targets, form, mats)
    for t in targets:
        assert rel_err(ctx.mat_values(mats[t], *shapes[t]), first[t]) < 1e-14, (label, t)
    return first


# ---- plain KLE targets: forms 5, 4, 3 and 2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,form,targets", [(s, f, t) for s, forms, t in gc.KLE_CASES for f in forms], ids=gc.case_id)
def test_kle_forms_vs_oracle(lib, spec, form, targets):
    mesh = gc.mesh_of(spec)
    ctx = make_ctx(lib, mesh, mesh.ngl)
    for label, mask, ref in kle_sets(spec):
        check_kle(lib, ctx, spec, form, targets, mask, ref, label)
    ctx.close()


@pytest.mark.parametrize("spec", gc.ONE_CELL, ids=gc.tag)
def test_one_cell_staged_equals_per_pair_bit_for_bit(lib, spec):
    """The staged path (form 4) sums every entry over the points in the order g = 0, 1, ... of the per-pair path (form 3), as its
    comment says: with one cell no atomic has a partner, so the two forms must give the same bits."""
    mesh = gc.mesh_of(spec)
    ctx = make_ctx(lib, mesh, mesh.ngl)
    for label, mask, ref in kle_sets(spec):
        v3 = check_kle(lib, ctx, spec, 3, gc.ALL4, mask, ref, label)
        v4 = check_kle(lib, ctx, spec, 4, gc.ALL4, mask, ref, label)
        differ = {t: int(np.count_nonzero(v3[t] != v4[t])) for t in gc.ALL4}
        print(f"{gc.tag(spec)} {label}: entries that differ between forms 3 and 4 {differ}")
        assert not any(differ.values()), (label, differ, {t: rel_err(v4[t], v3[t]) for t in gc.ALL4})
    ctx.close()


def test_grid_stride_staged_equals_matrix_cores(lib):
    """1080 cells on a grid of at most 1024 workgroups: some workgroups take a second cell with the scratch and LDS of the first.
    No oracle at this size: the staged form twice (1e-14), then against the matrix cores (FP_TOL)."""
    spec = gc.STRIDE_CASE
    mesh = gc.mesh_of(spec)
    assert mesh.n_elem > 1024
    dim, shapes = 2, block_shapes(2)
    ctx = make_ctx(lib, mesh, mesh.ngl, bc_ndof=dim, bc_nodes=mesh.boundary)
    m4 = assemble_kle(lib, ctx, dim, gc.ALL4, 4)
    first = {t: ctx.mat_values(m4[t], *shapes[t]) for t in gc.ALL4}
    assemble_kle(lib, ctx, dim, gc.ALL4, 4, m4)
    for t in gc.ALL4:
        assert rel_err(ctx.mat_values(m4[t], *shapes[t]), first[t]) < 1e-14, t
    assemble_kle(lib, ctx, dim, gc.ALL4, 5, m4)
    for t in gc.ALL4:
        err = rel_err(ctx.mat_values(m4[t], *shapes[t]), first[t])
        print(f"{gc.tag(spec)} form 5 vs form 4 {t} {err:.2e}")
        assert err < FP_TOL, (t, err)
    ctx.close()


def test_kle_forms_on_rank_slabs(lib):
    """the `row >= n_owned` skip of all three scatters with ghost rows present: each rank's slab in isolation (detached comm), its
    owned rows against those of the serial reference"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    spec, forms, targets = gc.SLAB_CASE
    mesh = gc.mesh_of(spec)
    dim, ngl, size = mesh.dim, mesh.ngl, 2
    shapes = block_shapes(dim)
    sets = kle_sets(spec)
    for r in range(size):
        dom = DMPlexDom(boxMesh={'nelem': list(spec[1]), 'lower': [0.0] * dim, 'upper': gm.UPPER[:dim]}, comm=Comm(r, size))
        dom.setFemIndexing(ngl)
        cols = dom._local2global(np.arange(dom.nLocal))           # lattice ids: the numbering of fo.box_mesh
        assert dom.nGhost > 0
        ctx = lib.Context(0)
        ctx.comm_init(r, size, None)                              # detached
        ctx.halo_set(*dom._halo_plan())
        ctx.mesh_set(dim, dom.conn, mesh.xyz[cols])
        for t in Spectral(ngl, dim).deviceTables():
            ctx.tables_set(*t)
        ctx.csr_symbolic()
        rows = fo.dof_indices(np.arange(dom.rStart, dom.rEnd), dim)
        for label, mask, ref in sets:
            ctx.bc_set(dim, mask[cols])
            for form in forms:
                mats = assemble_kle(lib, ctx, dim, targets, form)
                for t in targets:
                    want = ref[t][rows][:, fo.dof_indices(cols, shapes[t][1])]
                    err = sp_rel_err(mat_to_scipy(ctx, mats[t], *shapes[t]), want)
                    print(f"{gc.tag(spec)} rank {r} form {form} {label}: {t} {err:.2e}")
                    assert err < FP_TOL, (r, form, label, t, err)
        ctx.close()


# ---- scalar forms: never stageable, form 3 is their default above the LDS ------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCALAR_FORMS)
@pytest.mark.parametrize("spec,form", gc.SCALAR_CASES, ids=gc.case_id)
def test_scalar_forms_vs_oracle(lib, spec, form, name):
    mesh = gc.mesh_of(spec)
    tb = gm.tables(mesh.ngl, mesh.dim)
    lib_form = {"laplace": lib.FORM_LAPLACE, "mass_nodal": lib.FORM_MASS_NODAL, "mass_full": lib.FORM_MASS_FULL}[name]
    ctx = make_ctx(lib, mesh, mesh.ngl)
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    for label, nodes in (("boundary", mesh.boundary), ("interior", np.concatenate([mesh.boundary, extra_nodes(mesh)]))):
        if name == "mass_full":     # fo.assemble_scalar integrates the mass on the nodal rule: the same lines with the full rule
            with mock.patch.object(fo, "elem_mass", functools.partial(fo.elem_mass, rule="full")):
                ref = fo.assemble_scalar(mesh, tb, "mass", dirichlet=nodes)
        else:
            ref = fo.assemble_scalar(mesh, tb, "laplace" if name == "laplace" else "mass", dirichlet=nodes)
        mask = np.zeros((mesh.n_node, 1), np.uint8)
        mask[nodes] = 1
        ctx.bc_set(1, mask)
        first = None
        for _ in range(2):
            ctx.assemble_scalar(lib_form, A, Arhs, variant=0)
            assert_assembled(ctx, lib.AK_GENERIC, generic=form, krhs_completed=0, dinv=0)
            vals = [ctx.mat_values(A, 1, 1), ctx.mat_values(Arhs, 1, 1)]
            if first is not None:
                assert rel_err(vals[0], first[0]) < 1e-14 and rel_err(vals[1], first[1]) < 1e-14
            first = vals
        ea, er = sp_rel_err(mat_to_scipy(ctx, A, 1, 1), ref["A"]), sp_rel_err(mat_to_scipy(ctx, Arhs, 1, 1), ref["Arhs"])
        print(f"{gc.tag(spec)} {name} form {form} {label}: A {ea:.2e} Arhs {er:.2e}")
        assert ea < FP_TOL and er < FP_TOL, (label, ea, er)
    ctx.close()


# ---- first-order operators above ngl 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,form", gc.OPERATOR_CASES, ids=gc.case_id)
def test_operator_forms_vs_oracle(lib, spec, form):
    from pynama_amd.elements.spectral import Spectral
    mesh = gc.mesh_of(spec)
    dim, ngl = mesh.dim, mesh.ngl
    ref = fo.assemble_operators(mesh, gm.tables(ngl, dim))
    ctx = make_ctx(lib, mesh, ngl)
    ops = Spectral(ngl, dim).operatorTerms()
    mass = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_MASS_NODAL, mass, -1, 0)
    assert_assembled(ctx, lib.AK_GENERIC, generic=form)
    vw = ctx.vec_create(1)
    ctx.mat_diagonal(mass, vw)
    w = ctx.vec_get(vw, 1)
    assert rel_err(w, ref["weights"]) < FP_TOL
    for name in ("SrT", "DivSrT", "Curl"):
        br, bc, terms, coef = ops[name]
        m = ctx.mat_create(br, bc)
        ctx.assemble_operator(lib.Q_NODAL, terms, coef, m)
        assert_assembled(ctx, lib.AK_GENERIC, generic=form)
        raw = ctx.mat_values(m, br, bc)
        ctx.assemble_operator(lib.Q_NODAL, terms, coef, m)
        assert_assembled(ctx, lib.AK_GENERIC, generic=form)
        assert rel_err(ctx.mat_values(m, br, bc), raw) < 1e-14, name
        vs = ctx.vec_create(br)
        ctx.vec_set(vs, np.repeat(1.0 / w, br))
        ctx.mat_row_scale(m, vs)
        err = sp_rel_err(mat_to_scipy(ctx, m, br, bc), ref[name])
        print(f"{gc.tag(spec)} {name} form {form}: {err:.2e}")
        assert err < FP_TOL, (name, err)
    ctx.close()


# ---- no-slip / free-slip split: *fs targets are never staged -----------------------------------------------------------------------
@pytest.mark.parametrize("spec,form", gc.NOSLIP_CASES, ids=gc.case_id)
def test_noslip_forms_vs_oracle(lib, spec, form):
    mesh = gc.mesh_of(spec)
    dim = mesh.dim
    dw = 1 if dim == 2 else 3
    ns, dr = (["up", "down"], ["left"]) if dim == 2 else (["up", "left"], ["front"])
    cls = fo.noslip_classes(mesh, ns, dr)
    assert {0, 1, 2} <= set(np.unique(cls))
    ref = fo.assemble_kle_noslip(mesh, gm.tables(mesh.ngl, dim), cls, *ALPHA)
    ctx = make_ctx(lib, mesh, mesh.ngl)
    ctx.bc_set(dim, cls)
    shapes = [("K", dim, dim), ("Krhs", dim, dim), ("Rw", dim, dw), ("Rd", dim, 1),
              ("Kfs", dim, dim), ("Krhsfs", dim, dim), ("Rwfs", dim, dw), ("Rdfs", dim, 1)]
    ids = [ctx.mat_create(br, bc) for _, br, bc in shapes]
    first = None
    for _ in range(2):
        ctx.assemble_kle_noslip(*ALPHA, ids)
        assert_assembled(ctx, lib.AK_GENERIC, generic=form, krhs_completed=0, dinv=0)
        vals = [ctx.mat_values(mid, br, bc) for (_, br, bc), mid in zip(shapes, ids)]
        if first is not None:
            for (name, _, _), a, b in zip(shapes, vals, first):
                assert rel_err(a, b) < 1e-14, name
        first = vals
    for (name, br, bc), mid in zip(shapes, ids):
        err = sp_rel_err(mat_to_scipy(ctx, mid, br, bc), ref[name])
        print(f"{gc.tag(spec)} noslip form {form}: {name} {err:.2e}")
        assert err < FP_TOL, (name, err)
    ctx.close()
