"""Keeps the case table of tests/generic_forms_cases.py honest without a GPU: under the listed switches the chooser (asm_choose,
exported as pyn_assemble_choose) sends every row to the generic kernel in exactly the listed launch form, every mesh of the table
has det J > 0 at all points of the three rules in every cell, and every mesh holds a cell whose det J varies by more than 1 % over
the full rule (it is not affine).  tests/test_gpu_generic_forms.py asserts the same forms from Context.assemble_last()."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from pynama_amd._lib import AK_GENERIC, FORM_KLE, FORM_LAPLACE, FORM_MASS_FULL, FORM_MASS_NODAL, FORM_OPERATOR, Q_NODAL
from tests import generic_forms_cases as gc
from tests import ho_general_meshes as gm
from tests.test_assemble_choose_host import check, ho3

SCALAR_REQUEST = {"laplace": dict(form=FORM_LAPLACE, K=1, Krhs=1), "mass_nodal": dict(form=FORM_MASS_NODAL, K=1, Krhs=1),
                  "mass_full": dict(form=FORM_MASS_FULL, K=1, Krhs=1)}


def facts(spec):
    """what asm_facts reports for a table mesh: the row-run view exists on lattices up to ngl 3 only, and finds bent cells there"""
    kind, nelem, ngl = spec
    return ho3(len(nelem), ngl, ho3_valid=int(kind == "W" and ngl <= 3), ho3_affine=0)


def kle_request(targets):
    return dict(dict(form=FORM_KLE, variant=0), **{t: 1 for t in targets})


def knobs(form):
    return {k: 1 for k in gc.KLE_KNOBS[form]}


@pytest.mark.parametrize("spec,forms,targets", gc.KLE_CASES + [gc.SLAB_CASE] + [(s, (4, 3), gc.ALL4) for s in gc.ONE_CELL] +
                         [(gc.STRIDE_CASE, (4, 5), gc.ALL4)], ids=gc.case_id)
def test_kle_rows_reach_their_form(spec, forms, targets):
    for form in forms:
        check(kle_request(targets), facts(spec), knobs(form), AK_GENERIC, generic=form, krhs_completed=0, dinv=0)
    if 5 in forms:      # the switches are what moves the row, not the request
        check(kle_request(targets), facts(spec), {}, AK_GENERIC, generic=5)


@pytest.mark.parametrize("spec,form", gc.SCALAR_CASES, ids=gc.case_id)
def test_scalar_rows_reach_their_form(spec, form):
    for name in gc.SCALAR_FORMS:
        check(dict(SCALAR_REQUEST[name], variant=0), facts(spec), {}, AK_GENERIC, generic=form)


@pytest.mark.parametrize("spec,form", gc.OPERATOR_CASES, ids=gc.case_id)
def test_operator_rows_reach_their_form(spec, form):
    from pynama_amd.elements.spectral import Spectral
    ops = Spectral(spec[2], len(spec[1])).operatorTerms()
    for name in ("SrT", "DivSrT", "Curl"):
        check(dict(form=FORM_OPERATOR, K=1, op_rule=Q_NODAL, op_nterms=len(ops[name][3])), facts(spec), {}, AK_GENERIC, generic=form)
    check(dict(form=FORM_MASS_NODAL, K=1, variant=0), facts(spec), {}, AK_GENERIC, generic=form)      # the lumped weights


@pytest.mark.parametrize("spec,form", gc.NOSLIP_CASES, ids=gc.case_id)
def test_noslip_rows_reach_their_form(spec, form):
    # pyn_assemble_kle_noslip launches the generic kernel itself; its *fs targets make it not stageable, which is what
    # PYNAMA_NO_HO makes of a plain KLE request: the chooser under that switch names the split's form
    check(kle_request(gc.ALL4), facts(spec), dict(no_ho=1), AK_GENERIC, generic=form)


def _dets(mesh):
    """det J of every cell at the points of the full, reduced and nodal rule: [E, ngp] each (the oracle's _geom)"""
    tb = gm.tables(mesh.ngl, mesh.dim)
    X = mesh.corners().reshape(mesh.n_elem, tb.nc, mesh.dim)
    return [fo._geom(qg, q, X)[1] / q.w[None, :] for qg, q in ((tb.coo, tb.full), (tb.coo_red, tb.red), (tb.coo_op, tb.op))]


@pytest.mark.parametrize("spec", gc.all_meshes(), ids=gc.tag)
def test_table_meshes_are_valid_and_not_affine(spec):
    mesh = gc.mesh_of(spec)
    assert mesh.ngl == spec[2] and mesh.conn.shape == (int(np.prod(spec[1])), spec[2] ** len(spec[1]))
    full, red, nodal = _dets(mesh)
    for det in (full, red, nodal):
        assert det.min() > 0.0
    spread = (full.max(axis=1) - full.min(axis=1)) / full.min(axis=1)
    assert spread.max() > 0.01, spread.max()


def test_warped_lattice_moves_every_corner_and_keeps_the_sets():
    for dim, nelem, ngl in ((2, [1, 1], 7), (3, [2, 1, 2], 4)):
        box = fo.box_mesh(nelem, [0.0] * dim, gm.UPPER[:dim], ngl)
        mesh = gm.warped_lattice(dim, nelem, ngl)
        h = min(u / n for u, n in zip(gm.UPPER[:dim], nelem))
        corners = np.unique(box.conn[:, :2 ** dim])
        move = np.abs(mesh.xyz - box.xyz)
        assert (move[corners] > 0.0).all() and move.max() <= 0.15 * h * (1 + 1e-12)
        assert np.array_equal(mesh.conn, box.conn) and np.array_equal(mesh.boundary, box.boundary)
        assert all(np.array_equal(mesh.borders[k], box.borders[k]) for k in box.borders)
        # every node is the multilinear image of its cell's corners
        img = np.einsum("gc,ecd->egd", gm.tables(ngl, dim).coo_op.H, mesh.xyz[mesh.conn[:, :2 ** dim]])
        assert np.abs(mesh.xyz[mesh.conn] - img).max() < 1e-15
        # another seed is another mesh, the same seed the same
        assert np.array_equal(gm.warped_lattice(dim, nelem, ngl).xyz, mesh.xyz)
        assert not np.array_equal(gm.warped_lattice(dim, nelem, ngl, seed=1).xyz, mesh.xyz)
