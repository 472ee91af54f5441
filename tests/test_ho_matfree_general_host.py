"""Host side of the general matrix-free KLE operator (PYN_MATFREE_KLE_GENERAL, pynama_amd/csrc/pyn_matfree_ho_general.hip), no GPU:
the numpy model of the kernel's cell product with a pointwise Jacobian -- built from the library's 1-D tables and local-lattice table
alone -- against the oracle's dense element matrix on bent and on rotated cells, and the mesh builders of tests/ho_general_meshes.py."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import ho_general_meshes as gm
from tests.util import rel_err

FP_TOL = 2e-13          # the bar of the GPU tests; this comparison measures <= 1e-14 (ngl 12), <= 3e-15 up to ngl 8
ORDERS = [(2, 4), (2, 5), (2, 8), (2, 12), (3, 4), (3, 5)]


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    _lib.load_library()
    return _lib


def _model_against_oracle(lib, mesh, cell):
    dim, ngl = mesh.dim, mesh.ngl
    t, loc = lib.ho_tables_1d(ngl), lib.ho_local_lattice(ngl, dim)
    x = np.random.default_rng(5).standard_normal((mesh.n_node, dim))
    nodes = mesh.conn[cell]
    worst = 0.0
    for alpha_d, alpha_w in ((1e3, 1e2), (0.0, 0.0)):
        Ke = fo.elem_kle_matrices(gm.tables(ngl, dim), mesh.corners()[cell:cell + 1], alpha_d, alpha_w)[0][0]
        yo = (Ke @ x[nodes].reshape(-1)).reshape(-1, dim)
        y = gm.cell_product_pointwise(t, loc, nodes, mesh.xyz, x, alpha_d, alpha_w)
        worst = max(worst, rel_err(y[nodes], yo))
    return worst


def test_operator_id(lib):
    assert lib.MATFREE_KLE_GENERAL == 3 and lib.MATFREE_KLE == 2


@pytest.mark.parametrize("dim,ngl", ORDERS)
def test_pointwise_jacobian_model_equals_the_oracle_on_a_bent_cell(lib, dim, ngl):
    """one cell, every corner moved by up to +-0.125 of the edge: the two-rule form with J at every point is the oracle's K_e"""
    mesh = fo.box_mesh([1] * dim, [0.0] * dim, [1.0] * dim, ngl)
    nc = 2 ** dim
    corners = mesh.xyz[mesh.conn[0, :nc]] + 0.125 * np.random.default_rng(dim + ngl).uniform(-1, 1, (nc, dim))
    mesh.xyz[mesh.conn[0]] = gm._corner_image(ngl, dim, corners[None])[0]
    err = _model_against_oracle(lib, mesh, 0)
    print(f"dim {dim} ngl {ngl}: bent cell, model vs oracle {err:.3e}")
    assert err < FP_TOL


@pytest.mark.parametrize("dim,ngl", ORDERS)
def test_pointwise_jacobian_model_on_rotated_imported_cells(lib, dim, ngl):
    """cells of an imported mesh through their connectivity: a_of_t and the corner mapping with rotated, renumbered cells"""
    mesh = gm.imported(dim, [2] * dim, ngl)
    err = max(_model_against_oracle(lib, mesh, e) for e in range(0, mesh.n_elem, 3))
    print(f"dim {dim} ngl {ngl}: imported cells, model vs oracle {err:.3e}")
    assert err < FP_TOL


def _assert_consistent(mesh):
    nc = 2 ** mesh.dim
    img = gm._corner_image(mesh.ngl, mesh.dim, mesh.xyz[mesh.conn[:, :nc]])
    assert np.abs(img - mesh.xyz[mesh.conn]).max() < 1e-13
    assert np.array_equal(np.unique(mesh.conn), np.arange(mesh.n_node))
    # positive Jacobian at the corners of every cell (reference orientation)
    J = np.einsum("gdc,ecx->egdx", gm.tables(mesh.ngl, mesh.dim).coo_op.Hrs, mesh.xyz[mesh.conn[:, :nc]])
    assert np.linalg.det(J).min() > 0


@pytest.mark.parametrize("dim,nelem,ngl", [(2, [5, 2], 4), (2, [3, 2], 12), (3, [3, 2, 3], 4), (3, [2, 2, 3], 6)])
def test_bent_lattice_and_imported_are_self_consistent(dim, nelem, ngl):
    """every cell's multilinear image of the GLL points equals the coordinates its connectivity points at"""
    box = fo.box_mesh(nelem, [0.0] * dim, gm.UPPER[:dim], ngl)
    bent = gm.bent_lattice(dim, nelem, ngl, seed=1)
    assert np.array_equal(bent.conn, box.conn) and np.array_equal(bent.boundary, box.boundary)
    moved = np.linalg.norm(bent.xyz - box.xyz, axis=1)
    assert moved[bent.boundary].max() < 1e-14 and moved.max() > 0.01          # the box keeps its faces; the inside is bent
    _assert_consistent(bent)
    imp = gm.imported(dim, nelem, ngl)
    assert imp.conn.shape == box.conn.shape and imp.n_node == box.n_node and len(imp.boundary) == len(box.boundary)
    assert not np.array_equal(imp.conn, box.conn)
    _assert_consistent(imp)


@pytest.mark.parametrize("k,ngl,layers", [(3, 4, 0), (5, 5, 0), (5, 8, 0), (3, 4, 2), (3, 5, 2)])
def test_star_has_the_stated_valences(k, ngl, layers):
    mesh = gm.star(k, ngl, layers)
    _assert_consistent(mesh)
    m = ngl - 1
    v = gm.valences(mesh)
    assert mesh.n_elem == k * max(layers, 1) and mesh.conn.shape[1] == ngl ** mesh.dim
    if not layers:
        assert mesh.n_node == 1 + 2 * k + 3 * k * (m - 1) + k * (m - 1) ** 2   # vertices, 3 k edges, k interiors
        assert v.max() == k and np.count_nonzero(v == k) == (1 if k != 2 else 0)          # the centre
        assert np.count_nonzero(v == 2) == k + k * (m - 1)                               # spoke ends and the spokes' edge nodes
        assert np.linalg.norm(mesh.xyz[np.argmax(v)]) < 1e-14
    else:
        assert v.max() == 2 * k                                                          # the centre line's interior vertex
        assert np.count_nonzero(v == 2 * k) == layers - 1
        assert np.count_nonzero(v == k) == 2 + layers * (m - 1)                          # its two ends and its edge nodes
