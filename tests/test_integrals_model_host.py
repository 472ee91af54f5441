"""Host checks of the numpy model of the mesh integrals (tests/integrals_model.py), which the GPU tests take as their reference:
volumes against the shoelace area and the box volume on warped and bent meshes, constants, a polynomial of the element's own degree
against its closed form on an affine box, the nodal rule against the oracle's nodal mass diagonal, and how far the order of the
summation moves a moment (the figure behind the parity bar of tests/test_gpu_integrals.py)."""
import math

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import ho_general_meshes as gm
from tests import integrals_model as im

SHAPES_2D = [((5, 3), 2), ((5, 3), 3), ((3, 2), 6), ((2, 1), 12)]
SHAPES_3D = [((3, 2, 2), 2), ((2, 2, 3), 3), ((2, 1, 2), 5), ((1, 1, 2), 8)]


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("dim,ngl", [(2, 2), (2, 5), (3, 2), (3, 4)])
def test_model_tables_are_the_oracles(dim, ngl):
    nod, _ = fo.gauss_lobatto(ngl)
    pts, w = fo.gauss_legendre(ngl + 1)
    mine, ref = im.tensor_tables(nod, pts, w, dim), fo.tensor_tables(nod, pts, w, dim)
    for name in ("H", "Hrs", "pts", "w"):
        assert np.array_equal(getattr(mine, name), getattr(ref, name)), name


@pytest.mark.parametrize("nelem,ngl", SHAPES_2D)
def test_volume_is_the_shoelace_area_on_warped_meshes(nelem, ngl):
    mesh = gm.warped_lattice(2, list(nelem), ngl)
    for rule in (im.NODAL, im.GAUSS):
        vals, _ = im.moments(mesh, np.zeros(mesh.n_node), rule)
        assert _rel(vals[0], im.shoelace_area(mesh)) <= 1e-13


@pytest.mark.parametrize("nelem,ngl", SHAPES_2D + SHAPES_3D)
def test_bent_lattice_keeps_the_box_volume_and_constants(nelem, ngl):
    dim = len(nelem)
    mesh = gm.bent_lattice(dim, list(nelem), ngl, seed=2)
    box = math.prod(gm.UPPER[:dim])
    c = -1.75
    for rule in (im.NODAL, im.GAUSS):
        vals, _ = im.moments(mesh, np.full(mesh.n_node, c), rule, grad=True)
        m = im.named(vals, dim, 1, True)
        assert _rel(m["volume"], box) <= 1e-13
        assert _rel(m["value"][0], c * box) <= 1e-13 and _rel(m["square"][0], c * c * box) <= 1e-13
        assert abs(m["grad2"][0]) <= 1e-12 * c * c * box


@pytest.mark.parametrize("nelem,ngl", SHAPES_2D + SHAPES_3D)
def test_polynomial_of_the_elements_degree_on_an_affine_box(nelem, ngl):
    dim = len(nelem)
    box = fo.box_mesh(list(nelem), [0.0] * dim, gm.UPPER[:dim], ngl)
    for s in (0.0, 0.3):
        vals, _ = im.moments(im.sheared(box, s), im.poly_nodal(box), im.GAUSS, grad=True)
        m = im.named(vals, dim, 1, True)
        sq, g2 = im.poly_closed_form(ngl, gm.UPPER[:dim], s)
        assert _rel(m["square"][0], sq) <= 1e-12 and _rel(m["grad2"][0], g2) <= 1e-12


@pytest.mark.parametrize("nelem,ngl", [((5, 3), 3), ((2, 1), 12), ((2, 2, 3), 3), ((2, 1, 2), 5)])
def test_nodal_value_is_the_lumped_mass_diagonal(nelem, ngl):
    dim = len(nelem)
    mesh = gm.warped_lattice(dim, list(nelem), ngl)
    Me = fo.elem_mass(gm.tables(ngl, dim), mesh.corners(), "nodal")
    weights = np.bincount(mesh.conn.ravel(), np.einsum("eaa->ea", Me).ravel(), minlength=mesh.n_node)
    u = np.random.default_rng(0).uniform(-1.0, 1.0, mesh.n_node)
    vals, S = im.moments(mesh, u, im.NODAL)
    assert abs(vals[1] - weights @ u) <= 1e-13 * S[1]
    assert abs(vals[0] - weights.sum()) <= 1e-13 * S[0]


def test_summation_order_moves_a_moment_far_less_than_the_parity_bar():
    """flat numpy sum, sequential sum and exact sum of the same contributions: the spread against S, the scale of the GPU bar 2e-13 S"""
    worst = 0.0
    for nelem, ngl in (((5, 3), 3), ((2, 2, 3), 3)):
        dim = len(nelem)
        mesh = gm.warped_lattice(dim, list(nelem), ngl)
        u = np.random.default_rng(1).uniform(-1.0, 1.0, (mesh.n_node, dim))
        for t in im.contributions(mesh, u, im.GAUSS, grad=True):
            flat = t.ravel()
            seq = 0.0
            for v in flat:
                seq += v
            exact, S = math.fsum(flat), math.fsum(np.abs(flat))
            worst = max(worst, abs(flat.sum() - exact) / S, abs(seq - exact) / S)
    assert worst <= 2e-14          # a tenth of the bar: what the bar needs of the order of summation, not what was measured
    print(f"summation-order spread {worst:.2e} S")
