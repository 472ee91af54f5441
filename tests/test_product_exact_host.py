"""Conditions on the INPUTS of the exact product tests (tests/product_exact.py), checked on the reference alone: no GPU."""
import numpy as np
import pytest

from tests import product_exact as pe
from tests.util import block_csr_to_scipy

_graphs = {}


def _graph(ngl, nelem):
    key = (ngl, tuple(nelem))
    if key not in _graphs:
        _graphs[key] = pe.host_graph(pe.mesh_of(ngl, nelem))
    return _graphs[key]


def _check(ex):
    S = block_csr_to_scipy(ex.rowptr, ex.colidx, ex.val.astype(np.float64), ex.br, ex.bc, n_cols_nodes=ex.n_cols_nodes)
    assert abs(S - ex.A.astype(np.float64)).max() == 0                    # the layout round-trips
    assert np.array_equal(S @ ex.x.astype(np.float64), ex.y.astype(np.float64))
    assert np.abs(ex.val).max() < 2 ** 40 and np.abs(ex.y).max() < 2 ** 40
    assert np.all(ex.x >= -4) and np.all(ex.x <= 4)
    if ex.b is not None:
        assert np.all(ex.b != 0) and np.abs(ex.b).max() <= 4
        assert 0 < ex.pap < 2 ** 40 and 0 < ex.bb < 2 ** 40
        assert np.abs(ex.Af @ ex.b).max() < 2 ** 40
        assert ex.pap == sum(int(u) * int(v) for u, v in zip(ex.b, ex.Af @ ex.b))      # Python ints: no overflow anywhere
        assert np.all(np.isfinite(ex.x1()))
    if ex.br == ex.bc and ex.n_cols_nodes == ex.rowptr.size - 1:
        assert abs(ex.A - ex.A.T).max() == 0                               # square shapes are symmetric


@pytest.mark.parametrize("case", pe.CASES, ids=lambda c: c.name)
def test_case_inputs(case):
    rp, ci = _graph(case.ngl, case.nelem)
    ex = pe.build(rp, ci, *case.block)
    _check(ex)
    assert (ex.b is not None) == (case.block[0] == case.block[1])
    assert case.solver is None or ex.b is not None


def test_row_widths_of_the_new_strips():
    """the two strips reach the W = 32 instantiations: scalar row width 28..32 (1x1) and 19..32 (2x2)"""
    rp, _ = _graph(4, (1, 40))
    assert 27 < np.diff(rp).max() <= 32
    rp, _ = _graph(3, (1, 40))
    assert 18 < 2 * np.diff(rp).max() <= 32


@pytest.mark.parametrize("hc", pe.HOLE_CASES, ids=lambda h: h[0])
def test_hole_inputs(hc):
    _, block, nelem, _, _ = hc
    cut, N, send, fold = pe.hole_mesh(nelem)
    rp, ci = pe.host_graph(cut, N)
    assert ci.max() >= N                                                   # ghost columns exist
    ex = pe.build(rp, ci, *block, n_cols_nodes=cut.n_node, fold=fold)
    _check(ex)
    assert ex.Af.shape[0] == ex.Af.shape[1] and ex.pap > 0
    # b.(Af b) > 0 for EVERY b: the symmetric part of the folded matrix is strictly diagonally dominant
    Sy = (ex.Af + ex.Af.T).tocsr().astype(np.float64)
    offsum = np.asarray(abs(Sy).sum(axis=1)).ravel() - np.abs(Sy.diagonal())
    assert np.all(Sy.diagonal() > offsum)


def test_detached_ghost_inputs():
    """ghost columns without a known owner: the product reference only"""
    cut, N, _, _ = pe.hole_mesh((4, 3, 6))
    rp, ci = pe.host_graph(cut, N)
    for block in ((1, 1), (3, 3)):
        ex = pe.build(rp, ci, *block, n_cols_nodes=cut.n_node)
        _check(ex)
        assert ex.b is None
