"""The multigrid hierarchy on box lattices of order ngl >= 4, restated in numpy (tests/mg_ho_model.py; no GPU needed): P0 from the GLL
node lattice to the Q1 lattice of the same cells is an interpolation (rows sum to 1, the vertex coordinates reproduce every node
coordinate), and PCG preconditioned with the model's V-cycle on the oracle's K converges in a quarter of Jacobi-PCG's iterations."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import mg_ho_model as mm

P0_CASES = [([3, 2], 4), ([3, 2], 5), ([3, 2], 9), ([2, 3, 2], 4)]


@pytest.mark.parametrize("nel,ngl", P0_CASES)
def test_p0_rows_sum_to_one(nel, ngl):
    dim = len(nel)
    mesh = fo.box_mesh(nel, [0.0] * dim, [1.0, 0.8, 1.2][:dim], ngl)
    nper, ids = mm.ho_lattice_of(mesh, nel, ngl)
    P = mm.interpolation_ho(ids, nel, ngl)
    assert P.shape == (mesh.n_node, int(np.prod([e + 1 for e in nel])))
    assert np.abs(np.asarray(P.sum(axis=1)).ravel() - 1.0).max() <= 4e-16
    assert P.min() >= 0.0 and np.diff(P.tocsr().indptr).max() <= 2 ** dim
    # a cell vertex has exactly one parent, weight exactly 1
    m = ngl - 1
    vert = ids[tuple(np.meshgrid(*[np.arange(0, n, m) for n in nper], indexing="ij"))].ravel()
    Pv = P.tocsr()[vert]
    Pv.eliminate_zeros()
    assert np.array_equal(np.diff(Pv.indptr), np.ones(len(vert), int)) and np.array_equal(Pv.data, np.ones(len(vert)))


@pytest.mark.parametrize("nel,ngl", P0_CASES)
def test_p0_reproduces_the_node_coordinates(nel, ngl):
    """P0 applied to the coarse vertex coordinates == the oracle mesh's node coordinates (1e-14)"""
    dim = len(nel)
    mesh = fo.box_mesh(nel, [0.0] * dim, [1.0, 0.8, 1.2][:dim], ngl)
    nper, ids = mm.ho_lattice_of(mesh, nel, ngl)
    m = ngl - 1
    corner = ids[tuple(np.meshgrid(*[np.arange(0, n, m) for n in nper], indexing="ij"))]   # [X, Y(, Z)] -> fine node id
    xc = mesh.xyz[corner.T.ravel()]                                                         # coarse nodes lexicographic, x fastest
    assert np.abs(mm.interpolation_ho(ids, nel, ngl) @ xc - mesh.xyz).max() <= 1e-14


def test_model_pcg_beats_jacobi():
    """2-D 8^2 ngl 5, oracle K (alpha_d 1e3, alpha_w 1e2, boundary imposed), degree 2, exact lambda: MG-PCG converges to 1e-10 in at
    most a quarter of Jacobi-PCG's iterations (44 against 333)"""
    nel, ngl, dim = [8, 8], 5, 2
    mesh = fo.box_mesh(nel, [0.0] * dim, [1.0] * dim, ngl)
    K = fo.assemble_kle_freeslip(mesh, fo.Tables(ngl, dim))["K"]
    nper, ids = mm.ho_lattice_of(mesh, nel, ngl)
    nlev = mm.ho_level_count(nel, ngl, dim, coarse_max_rows=100)
    assert nlev == 3
    levels = mm.ho_levels(K, ids, nel, ngl, dim, nlev)
    assert [l[0].shape[0] for l in levels] == [2178, 162, 50]
    lam = mm.exact_lambdas(levels)
    rhs = np.random.default_rng(0).standard_normal(K.shape[0])
    bc = np.zeros(mesh.n_node, bool)
    bc[mesh.boundary] = True
    rhs[np.repeat(bc, dim)] = 0.0
    xj, ij = mm.jacobi_pcg(K, rhs)
    xm, im = mm.mg_pcg(levels, lam, 2, rhs)
    print(f"Jacobi-PCG {ij}, MG-PCG {im}")
    for x in (xj, xm):
        assert np.linalg.norm(rhs - K @ x) <= 1e-10 * np.linalg.norm(rhs)
    assert 4 * im <= ij, (im, ij)
    assert np.abs(xm - xj).max() <= 1e-8 * np.abs(xj).max()
