"""Host side of the matrix-free KLE operator for orders ngl >= 4 (pynama_amd/csrc/pyn_matfree_ho.hip), no GPU: the 1-D tables the
library recomputes for the order, the local node order its lattice check assumes, and a numpy model of the sum-factorised cell
product built from those tables alone against the oracle's dense element matrix."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.util import rel_err


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    _lib.load_library()
    return _lib


@pytest.mark.parametrize("ngl", range(4, 13))
def test_tables_1d_reproduce_the_oracle(lib, ngl):
    """Lobatto(ngl) nodes / weights, Gauss(ngl - 1) points / weights, and the values / derivatives of the ngl Lagrange functions at
    both, against fo.gauss_lobatto / gauss_legendre / lagrange_1d.  Bar: 1e-13 absolute on entries of size O(ngl^2) at most -- the two
    sides run the same product formulas on nodes that agree to a few ulp."""
    t = lib.ho_tables_1d(ngl)
    xl, wl = fo.gauss_lobatto(ngl)
    xr, wr = fo.gauss_legendre(ngl - 1)
    assert np.max(np.abs(t["xl"] - xl)) < 1e-15 and np.max(np.abs(t["wl"] - wl)) < 1e-15
    assert np.max(np.abs(t["xr"] - xr)) < 1e-15 and np.max(np.abs(t["wr"] - wr)) < 1e-15
    h, dh = fo.lagrange_1d(xl, xl)
    assert np.max(np.abs(h - np.eye(ngl))) < 1e-14                      # collocated: the full rule needs no interpolation
    assert np.max(np.abs(t["Dl"] - dh)) < 1e-13
    h, dh = fo.lagrange_1d(xl, xr)
    assert np.max(np.abs(t["Br"] - h)) < 1e-13
    assert np.max(np.abs(t["Gr"] - dh)) < 1e-13


@pytest.mark.parametrize("dim,ngl", [(2, n) for n in range(2, 13)] + [(3, n) for n in range(2, 9)])
def test_local_lattice_is_the_box_mesh_order(lib, dim, ngl):
    """the closed form the connectivity of every order is verified against (ngl 2 and 3 included: the row-run assembly takes its tensor
    order from it too): the oracle's box mesh (cell 0) and the product's own DMPlexDom"""
    loc = lib.ho_local_lattice(ngl, dim)
    mesh = fo.box_mesh([2] * dim, [0.0] * dim, [1.0] * dim, ngl)
    lat = [(ngl - 1) * 2 + 1] * dim
    strides = np.array([int(np.prod(lat[:d])) for d in range(dim)])
    assert np.array_equal(mesh.conn[0], loc @ strides)
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    dom = DMPlexDom(boxMesh={'nelem': [2] * dim, 'lower': [0.0] * dim, 'upper': [1.0] * dim}, comm=Comm(0, 1))
    dom.setFemIndexing(ngl)
    assert np.array_equal(dom._loc, loc)


def test_limits(lib):
    assert lib.ho_matfree_max_ngl(2) == 12 and lib.ho_matfree_max_ngl(3) == 8
    with pytest.raises(lib.PynamaHipError, match="out of range"):
        lib.ho_tables_1d(40)


def _cell_product(t, dim, ngl, E, x, alpha_d, alpha_w):
    """y_e = K_e x_e as the kernel forms it: x [ngl]*dim + [dim] in LATTICE order (x fastest = last array axis), E[r] = the cell's edge
    along lattice axis r, tables from the library alone"""
    J = 0.5 * np.asarray(E)                       # J[r][x]
    Ji = np.linalg.inv(J)                         # Ji[x][r] = d xi_r / d x
    det = np.linalg.det(J)
    Dl, wl, Br, Gr, wr = t["Dl"], t["wl"], t["Br"], t["Gr"], t["wr"]
    ax = "kji"[-dim:]                             # array axes, slow to fast; lattice axis r = array axis dim - 1 - r

    def along(M, r, v):                           # contract lattice axis r of v (array axis dim-1-r) with M[out, in]
        return np.moveaxis(np.tensordot(M, v, axes=(1, dim - 1 - r)), 0, dim - 1 - r)

    y = np.zeros_like(x)
    # full rule: collocated Laplacian of every component
    w = wl
    for _ in range(dim - 1):
        w = np.multiply.outer(w, wl)
    Q = det * Ji.T @ Ji
    for p in range(dim):
        g = [along(Dl, r, x[..., p]) for r in range(dim)]
        for r in range(dim):
            f = w * sum(Q[r, s] * g[s] for s in range(dim))
            y[..., p] += along(Dl.T, r, f)
    # reduced rule
    w = wr
    for _ in range(dim - 1):
        w = np.multiply.outer(w, wr)

    def interp(v, r_der):
        for r in range(dim):
            v = along(Gr if r == r_der else Br, r, v)
        return v

    def interp_t(f, r_der):
        for r in range(dim):
            f = along((Gr if r == r_der else Br).T, r, f)
        return f

    D = np.zeros((dim, dim) + w.shape)            # D[q][d] = d u_q / d x_d
    for q in range(dim):
        g = [interp(x[..., q], r) for r in range(dim)]
        for d in range(dim):
            D[q, d] = sum(Ji[d, r] * g[r] for r in range(dim))
    tr = sum(D[q, q] for q in range(dim))
    for p in range(dim):
        W = [w * det * (alpha_d * tr if d == p else alpha_w * (D[p, d] - D[d, p])) for d in range(dim)]
        for r in range(dim):
            y[..., p] += interp_t(sum(Ji[d, r] * W[d] for d in range(dim)), r)
    return y


@pytest.mark.parametrize("dim,ngl", [(2, 4), (2, 5), (2, 8), (2, 12), (3, 4), (3, 5)])
@pytest.mark.parametrize("kind", ["unit", "stretched", "sheared"])
def test_sum_factorised_cell_equals_the_oracle(lib, dim, ngl, kind):
    """the operator of the kernel header, with the lattice-axis Jacobian and the library's tables, is the oracle's K_e (FP_TOL of the
    GPU tests; the issue's own figure for this comparison is <= 2.3e-15)"""
    t = lib.ho_tables_1d(ngl)
    up = [1.0, 0.8, 1.2][:dim] if kind == "stretched" else [1.0] * dim
    mesh = fo.box_mesh([1] * dim, [0.0] * dim, up, ngl)
    if kind == "sheared":
        A = np.eye(dim) + 0.25 * np.random.default_rng(3).standard_normal((dim, dim))
        mesh.xyz = mesh.xyz @ A.T + 0.3
    loc = lib.ho_local_lattice(ngl, dim)
    strides = np.array([ngl ** d for d in range(dim)])
    lat_of_local = loc @ strides                                          # lattice (tensor) index of every local node
    assert np.array_equal(mesh.conn[0], lat_of_local)
    m = ngl - 1
    E = [mesh.xyz[m * strides[r]] - mesh.xyz[0] for r in range(dim)]
    x = np.random.default_rng(5).standard_normal((ngl ** dim, dim))       # by lattice index
    for alpha_d, alpha_w in ((1e3, 1e2), (0.0, 0.0)):
        Ke = fo.elem_kle_matrices(fo.Tables(ngl, dim), mesh.corners(), alpha_d, alpha_w)[0][0]
        xe = x[lat_of_local].reshape(-1)                                  # element order, component fastest
        yo = (Ke @ xe).reshape(-1, dim)
        y = _cell_product(t, dim, ngl, E, x.reshape((ngl,) * dim + (dim,)), alpha_d, alpha_w).reshape(-1, dim)
        assert rel_err(y[lat_of_local], yo) < 2e-13, (alpha_d, rel_err(y[lat_of_local], yo))
