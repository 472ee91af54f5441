"""Host side of the general ngl 3 matrix-free KLE operator (PYN_MATFREE_KLE_NGL3_GENERAL, pynama_amd/csrc/pyn_matfree_ho3_general.hip),
no GPU: the numpy model of the kernel's cell product (tests/ho3_general_model.py: J from the corners in lattice orientation at every
point of the Gauss(3) and Gauss(2) rules, the library's own 1-D tables) against the oracle's dense element matrix on every cell of bent
lattices, imported meshes and stars; the models of the incidence list and of the set-time table check."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import ho3_general_model as hm
from tests import ho_general_meshes as gm

CELL_TOL = 1e-14        # per cell, relative to the largest entry of the cell's K_e x_e (measured: <= 4.5e-15); the bar of the ngl >= 4 host file
NELEM = {2: ([3, 2], [7, 4]), 3: ([2, 2, 2], [3, 2, 3])}


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    _lib.load_library()
    return _lib


def _meshes():
    out = []
    for dim in (2, 3):
        for nelem in NELEM[dim]:
            out.append((f"bent{dim}d{nelem}", lambda dim=dim, nelem=nelem: gm.bent_lattice(dim, nelem, 3, seed=3)))
            out.append((f"imported{dim}d{nelem}", lambda dim=dim, nelem=nelem: gm.imported(dim, nelem, 3)))
    out.append(("star5", lambda: gm.star(5, 3, 0)))
    out.append(("star5x2", lambda: gm.star(5, 3, 2)))
    return out


MESHES = _meshes()


def test_operator_id(lib):
    assert lib.MATFREE_KLE_NGL3_GENERAL == 4 and lib.MATFREE_KLE_GENERAL == 3 and lib.MATFREE_KLE == 2


def test_1d_tables(lib):
    """the Gauss(3) point bases on the Lobatto(3) nodes: partition of unity, exact derivative of x and x^2, a rule exact to degree 5"""
    t = hm.tables_1d(lib)
    assert np.allclose(t["xl"], [-1.0, 0.0, 1.0], atol=1e-15)
    for B, G, pts, w in ((t["Bf"], t["Gf"], t["xf"], t["wf"]), (t["Br"], t["Gr"], t["xr"], t["wr"])):
        assert np.abs(B.sum(axis=1) - 1).max() < 1e-15 and np.abs(G.sum(axis=1)).max() < 1e-15
        assert np.abs(B @ t["xl"] ** 2 - pts ** 2).max() < 1e-15 and np.abs(G @ t["xl"] ** 2 - 2 * pts).max() < 1e-15
        deg = 2 * len(pts) - 1
        for k in range(deg + 1):
            assert abs(w @ pts ** k - (0.0 if k % 2 else 2.0 / (k + 1))) < 1e-15


@pytest.mark.parametrize("name,make", MESHES, ids=[m[0] for m in MESHES])
def test_two_rule_model_equals_the_oracle_on_every_cell(lib, name, make):
    """every cell, penalties on and off: the model's y_e against the oracle's dense K_e x_e, relative to the cell's largest entry;
    det J > 0 at every point of both rules (the model asserts it)"""
    mesh = make()
    dim = mesh.dim
    t, loc = hm.tables_1d(lib), lib.ho_local_lattice(3, dim)
    x = np.random.default_rng(5).standard_normal((mesh.n_node, dim))
    tb, X = gm.tables(3, dim), mesh.corners()
    worst, dmin = 0.0, np.inf
    for alpha_d, alpha_w in ((1e3, 1e2), (0.0, 0.0)):
        Ke = fo.elem_kle_matrices(tb, X, alpha_d, alpha_w)[0]
        for e in range(mesh.n_elem):
            nodes = mesh.conn[e]
            yo = (Ke[e] @ x[nodes].reshape(-1)).reshape(-1, dim)
            y = hm.cell_product(t, loc, nodes, mesh.xyz, x, alpha_d, alpha_w)[nodes]
            worst = max(worst, np.abs(y - yo).max() / np.abs(yo).max())
    for e in range(mesh.n_elem):
        (_, df), (_, dr) = hm.cell_geometry(t, loc, mesh.conn[e], mesh.xyz)
        dmin = min(dmin, df.min(), dr.min())
    print(f"{name}: {mesh.n_elem} cells, model vs oracle {worst:.3e}, smallest det J {dmin:.3e}")
    assert dmin > 0
    assert worst <= CELL_TOL


INCIDENCE_MESHES = [m for m in MESHES if m[0] in ("bent2d[7, 4]", "imported3d[3, 2, 3]", "star5", "star5x2")]


@pytest.mark.parametrize("name,make", INCIDENCE_MESHES, ids=[m[0] for m in INCIDENCE_MESHES])   # (ids=str would print the builder's address)
def test_incidence_list(lib, name, make):
    """the node -> (cell, t) list: every entry once, ascending within a row, every entry of a row names that node, rows as long as
    the node's valence; on a lexicographic lattice an interior vertex has 2^dim entries"""
    mesh = make()
    aoft = hm.a_of_t(lib.ho_local_lattice(3, mesh.dim))
    ptr, inc = hm.incidence(mesh.conn, mesh.n_node, aoft)
    nn = mesh.conn.shape[1]
    assert ptr[0] == 0 and ptr[-1] == mesh.n_elem * nn and np.array_equal(np.sort(inc), np.arange(mesh.n_elem * nn))
    assert np.array_equal(np.diff(ptr), gm.valences(mesh))
    for n in range(mesh.n_node):
        row = inc[ptr[n]:ptr[n + 1]]
        assert np.all(np.diff(row) > 0)
        assert np.all(mesh.conn[row // nn, aoft[row % nn]] == n)
    if name.startswith("bent"):
        assert np.diff(ptr).max() == 2 ** mesh.dim


@pytest.mark.parametrize("dim", [2, 3])
def test_table_check_model(lib, dim):
    """the element tables of order 3 are the tensor products of the 1-D tables at both rules, in the reference order of points and
    nodes; the tables of the collocated Lobatto(3) rule are not (what the set-time check refuses)"""
    t, tb = hm.tables_1d(lib), gm.tables(3, dim)
    ln = np.array(fo.local_lattice(3, dim))
    assert hm.tensor_rule_error(tb.full, ln, ln, t["wf"], t["Bf"]) < 1e-14
    assert hm.tensor_rule_error(tb.red, np.array(fo.local_lattice(2, dim)), ln, t["wr"], t["Br"]) < 1e-14
    assert hm.tensor_rule_error(tb.op, ln, ln, t["wf"], t["Bf"]) > 1e-2
    # the geometry tables: the multilinear corner basis at the points of the full rule
    lc = np.array(fo.local_lattice(2, dim))
    B2 = np.stack([0.5 * (1 - t["xf"]), 0.5 * (1 + t["xf"])], axis=1)
    assert hm.tensor_rule_error(tb.coo, ln, lc, t["wf"], B2) < 1e-14
