"""Conditions on the INPUTS of the exact product tests (tests/product_exact.py), checked on the reference alone, and the kernel family
the library's chooser (pyn_product_choose, a host function) picks for every one of them: no GPU."""
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


# ---- the chooser: facts from the host graph, knobs as arguments ------------------------------------------------------
KNOB_ARGS = {"PYNAMA_SELL_IMAGE": ("sell_image", bool), "PYNAMA_BLOCK_SELL": ("block_sell", bool), "PYNAMA_NO_CSRLB": ("no_csrlb", bool),
             "PYNAMA_NO_SELL": ("no_sell", bool), "PYNAMA_BCSR_MIN_AVG": ("bcsr_min_avg", float)}


def _facts(rp, ci, block, env):
    """what pyn_sell_ensure knows of the matrix: dictionary or not, longest scalar row, graph size"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    n, lens = rp.size - 1, np.diff(rp)
    npat = 0
    if lens.max() <= 32 and "PYNAMA_NO_PATTERNS" not in env:
        pats = {tuple(ci[rp[i]:rp[i + 1]] - i) for i in range(n)}
        npat = len(pats) if len(pats) <= 256 else 0
    return dict(br=block[0], bc=block[1], npat=npat, maxw=int(lens.max()) * block[1], nnzb=int(ci.size), n_owned=n)


def _knob_args(env):
    assert set(env) <= set(KNOB_ARGS) | {"PYNAMA_NO_PATTERNS"}
    return {KNOB_ARGS[k][0]: KNOB_ARGS[k][1](v) for k, v in env.items() if k in KNOB_ARGS}


def _bcsr_defaults(facts):
    """as tests/test_gpu_product_exact.py predicts them from the entries per scalar row"""
    avg = facts["nnzb"] * facts["bc"] / facts["n_owned"]
    return (16 if avg >= 56.0 else 8), (8 if avg >= 24.0 else 4)


IMAGE_KINDS = (pe.SELL, pe.SELLP, pe.SELLB_X, pe.SELLB_D)


def _choose(facts, expected, what, **kw):
    """The chooser's answer against (family, param) of product_last.  param is the chooser's W for csrl / csrlb; a block-CSR answer
    carries the default lanes and unroll; the image kinds have no width (their param, the block columns, is not the chooser's)."""
    from pynama_amd import _lib
    kind, W, lanes, unroll = _lib.product_choose(**facts, **kw)
    family, param = expected
    assert kind == family, f"{what}: chose {pe.FAMILY[kind]}, expected {pe.FAMILY[family]}"
    if kind == pe.BCSR:
        assert param is None and (W, lanes, unroll) == (0,) + _bcsr_defaults(facts), f"{what}: {(W, lanes, unroll)}"
    elif kind in (pe.CSRL, pe.CSRLB):
        assert (W, lanes, unroll) == (param, 0, 0), f"{what}: {(W, lanes, unroll)}"
    else:
        assert (W, lanes, unroll) == (0, 0, 0), f"{what}: {(W, lanes, unroll)}"
    return kind


@pytest.mark.parametrize("case", pe.CASES, ids=lambda c: c.name)
def test_chooser_single_rank(case):
    from pynama_amd import _lib
    facts = _facts(*_graph(case.ngl, case.nelem), case.block, case.env)
    kn = _knob_args(case.env)
    if case.one_off[0] in (pe.CSRL, pe.CSRLB, pe.SELLP, pe.SELLB_D):
        assert facts["npat"] > 0
    if case.one_off[0] in (pe.SELL, pe.SELLB_X):
        assert facts["npat"] == 0
    _choose(facts, case.one_off, case.name + " one-off", solver=False, image=False, **kn)
    if case.solver is not None:          # the solve follows the one-off product: an image exists only if that product built one
        image = case.one_off[0] in IMAGE_KINDS
        _choose(facts, case.solver, case.name + " solver", solver=True, image=image, **kn)
        if case.solver[0] in IMAGE_KINDS:   # ... and with the solver's image a later one-off keeps it
            _choose(facts, case.solver, case.name + " one-off after the solve", solver=False, image=True, **kn)
    if case.one_off[0] == pe.BCSR:       # the sweep of the lanes and unroll knobs: 16 shapes
        g0, u0 = _bcsr_defaults(facts)
        seen = set()
        for lanes in (None, 8, 16, 32, 64):
            for un in (None, 2, 3, 4, 8):
                got = _lib.product_choose(**facts, bcsr_lanes=lanes, bcsr_unroll=un, **kn)
                assert got == (pe.BCSR, 0, lanes or g0, un or u0), f"{case.name} lanes {lanes} unroll {un}: {got}"
                seen.add(got[2:])
        assert len(seen) == 16


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("gc", pe.GHOST_CASES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-ngl{g[1]}-{len(g[2])}d")
def test_chooser_ghost_columns(gc, rank):
    """the owned rows of rank `rank` of 2 in its local numbering, ghost columns included"""
    from types import SimpleNamespace
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    block, ngl, nelem, expected = gc
    dim = len(nelem)
    dom = DMPlexDom(boxMesh={'nelem': list(nelem), 'lower': [0.0] * dim, 'upper': [1.0] * dim}, comm=Comm(rank, 2))
    dom.setFemIndexing(ngl)
    rp, ci = pe.host_graph(SimpleNamespace(conn=dom.conn, n_node=dom.nLocal), dom.nOwned)
    assert ci.max() >= dom.nOwned
    _choose(_facts(rp, ci, block, {}), expected, f"ghost {gc} rank {rank}", solver=False, image=False)


@pytest.mark.parametrize("hc", pe.HOLE_CASES, ids=lambda h: h[0])
def test_chooser_hole(hc):
    """the whole product first (one-off: the test pins no family for it), then the solver, with the image that product left"""
    from pynama_amd import _lib
    name, block, nelem, env, expected = hc
    cut, N, _, _ = pe.hole_mesh(nelem)
    facts = _facts(*pe.host_graph(cut, N), block, env)
    one_off = _lib.product_choose(**facts, solver=False, image=False, **_knob_args(env))[0]
    assert one_off != 0
    _choose(facts, expected, f"hole {name}", solver=True, image=one_off in IMAGE_KINDS, **_knob_args(env))
