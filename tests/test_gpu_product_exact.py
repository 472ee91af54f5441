"""Exact-arithmetic tests of every product kernel family (run on a real MI355X with `-m gpu`).

Matrices and vectors hold small integers (tests/product_exact.py), so y = A x and the fused dot p.Ap have ONE correct bit pattern
whatever the summation order: every comparison is `==`.  Each case also asserts, from Context.product_last(), WHICH kernel ran, so
that a heuristic that moves cannot silently move a test onto another path.  The expected families were read off product_choose
(pyn_sell.hip; tests/test_product_exact_host.py asserts them on the host); PYNAMA_SPMV_MAX_GRID=1 makes one workgroup walk every
slice, i.e. the persistent loops (and their row-pointer prefetch) turn several times at these sizes."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from tests import product_exact as pe

pytestmark = pytest.mark.gpu

KNOBS = ("PYNAMA_SPMV_MAX_GRID", "PYNAMA_SELL_IMAGE", "PYNAMA_NO_PATTERNS", "PYNAMA_NO_SELL", "PYNAMA_NO_CSRLB", "PYNAMA_BLOCK_SELL",
         "PYNAMA_BCSR_MIN_AVG", "PYNAMA_BCSR_LANES", "PYNAMA_BCSR_UNROLL", "PYNAMA_OVERLAP_REQUIRE", "PYNAMA_NO_OVERLAP")


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@contextmanager
def knobs(**kv):
    """exactly these product knobs for the block, none afterwards"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        for k, v in kv.items():
            if v is not None:
                os.environ[k] = str(v)
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


_meshes = {}


def _mesh(ngl, nelem):
    key = (ngl, tuple(nelem))
    if key not in _meshes:
        _meshes[key] = pe.mesh_of(ngl, nelem)
    return _meshes[key]


def _setup(ctx, block, fold=None, host_graph=None):
    """graph -> integer matrix, uploaded row by row and read back bit-equal"""
    ctx.csr_symbolic()
    rp, ci = ctx.csr_get()
    if host_graph is not None:
        assert np.array_equal(rp, host_graph[0]) and np.array_equal(ci, host_graph[1])
    ex = pe.build(rp, ci, *block, n_cols_nodes=ctx.n_owned + ctx.n_ghost, fold=fold)
    mid = ctx.mat_create(*block)
    pe.upload(ctx, mid, ex)
    assert np.array_equal(ctx.mat_values(mid, *block), ex.val.astype(np.float64))
    return ex, mid


def _bcsr_defaults(ex):
    """lanes per node row and unroll that product_choose (pyn_sell.hip) picks without knobs, from the entries per scalar row"""
    avg = ex.colidx.size * ex.bc / (ex.rowptr.size - 1)
    return (16 if avg >= 56.0 else 8), (8 if avg >= 24.0 else 4)


def _expect(last, family, param, dot, what):
    assert last["family"] == family, f"{what}: ran {pe.FAMILY[last['family']]} {last}, expected {pe.FAMILY[family]}"
    if param is not None:
        assert last["param"] == param, f"{what}: {last}"
    assert last["dot"] == dot, f"{what}: {last}"


def _plain(ctx, mid, ex, vx, vy, family, param, what, grid1=False):
    before = ctx.product_last()["launches"]
    ctx.vec_fill(vy, 7.0)
    ctx.spmv(mid, vx, vy)
    got = ctx.vec_get(vy, ex.br)
    assert np.array_equal(got, ex.y.astype(np.float64)), f"{what}: {np.count_nonzero(got != ex.y)} of {got.size} entries differ"
    last = ctx.product_last()
    _expect(last, family, param, 0, what)
    assert last["launches"] == before + 1
    if grid1 and family != pe.RAW:
        assert last["grid"] == 1, f"{what}: {last}"
    return last


def _bcsr_sweep(ctx, mid, ex, vx, vy, what, grid1):
    g0, u0 = _bcsr_defaults(ex)
    seen = set()
    for lanes in (None, 8, 16, 32, 64):
        for un in (None, 2, 3, 4, 8):
            try:
                if lanes:
                    os.environ["PYNAMA_BCSR_LANES"] = str(lanes)
                if un:
                    os.environ["PYNAMA_BCSR_UNROLL"] = str(un)
                last = _plain(ctx, mid, ex, vx, vy, pe.BCSR, lanes or g0, f"{what} lanes {lanes} unroll {un}", grid1)
            finally:
                os.environ.pop("PYNAMA_BCSR_LANES", None)
                os.environ.pop("PYNAMA_BCSR_UNROLL", None)
            assert last["unroll"] == (un or u0), f"{what}: {last}"
            seen.add((last["param"], last["unroll"]))
    assert len(seen) == 16
    return seen


VARIANTS = [(c, g) for c in pe.CASES for g in ((None, 1) if c.max_grid1 else (None,))]


@pytest.mark.parametrize("case,max_grid", VARIANTS, ids=[c.name + ("-grid1" if g else "") for c, g in VARIANTS])
def test_single_rank(lib, case, max_grid):
    mesh = _mesh(case.ngl, case.nelem)
    br, bc = case.block
    what = case.name + (" max_grid 1" if max_grid else "")
    with knobs(PYNAMA_SPMV_MAX_GRID=max_grid, **case.env):
        ctx = lib.Context(0)
        try:
            ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
            ex, mid = _setup(ctx, case.block, host_graph=pe.host_graph(mesh))
            vx, vy = ctx.vec_create(bc), ctx.vec_create(br)
            ctx.vec_set(vx, ex.x.astype(np.float64))
            fam, par = case.one_off
            last = _plain(ctx, mid, ex, vx, vy, fam, par, what, grid1=bool(max_grid))      # (a) + (b)
            if fam in (pe.CSRL, pe.CSRLB, pe.SELLP, pe.SELLB_D):
                assert last["npat"] > 0, f"{what}: {last}"
            if fam in (pe.SELL, pe.SELLB_X):
                assert last["npat"] == 0, f"{what}: {last}"
            if fam == pe.BCSR:
                _bcsr_sweep(ctx, mid, ex, vx, vy, what, bool(max_grid))
            if case.solver is not None:                                                     # (c) the fused dot
                vb, v1 = ctx.vec_create(br), ctx.vec_create(br)
                ctx.vec_set(vb, ex.b.astype(np.float64))
                info = ctx.solve(mid, vb, v1, method=lib.KSP_CG, pc=lib.PC_NONE, fixed_iters=1, cg_variant=1)
                assert info.iters == 1
                got = ctx.vec_get(v1, br)
                assert np.array_equal(got, ex.x1()), \
                    f"{what}: alpha = {got[0] / ex.b[0]!r}, exact bb / pap = {ex.bb} / {ex.pap} = {ex.bb / ex.pap!r}"
                sfam, spar = case.solver
                last = ctx.product_last()
                _expect(last, sfam, spar, 1, what + " (solver)")
                if sfam == pe.BCSR:
                    g0, u0 = _bcsr_defaults(ex)
                    assert (last["param"], last["unroll"]) == (g0, u0)
                if max_grid and sfam != pe.RAW:
                    assert last["grid"] == 1
            elif br != bc:                                                                  # rectangular: the SELL image as well
                for extra, fam2, npat in (({}, pe.SELLB_D, True), ({"PYNAMA_NO_PATTERNS": "1"}, pe.SELLB_X, False)):
                    with knobs(PYNAMA_SPMV_MAX_GRID=max_grid, PYNAMA_BLOCK_SELL=1, **extra):
                        c2 = lib.Context(0)
                        try:
                            c2.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
                            ex2, m2 = _setup(c2, case.block)
                            wx, wy = c2.vec_create(bc), c2.vec_create(br)
                            c2.vec_set(wx, ex2.x.astype(np.float64))
                            last = _plain(c2, m2, ex2, wx, wy, fam2, bc, what + f" image {extra}")
                            assert (last["npat"] > 0) == npat
                        finally:
                            c2.close()
        finally:
            ctx.close()


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("gc", pe.GHOST_CASES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-ngl{g[1]}-{len(g[2])}d")
def test_ghost_columns(lib, gc, rank):
    """rank `rank` of 2, detached: the ghost entries of x are supplied by the caller; plain product and family"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    block, ngl, nelem, (fam, par) = gc
    dim = len(nelem)
    with knobs():
        dom = DMPlexDom(boxMesh={'nelem': list(nelem), 'lower': [0.0] * dim, 'upper': [1.0] * dim}, comm=Comm(rank, 2))
        dom.setFemIndexing(ngl)
        ctx = lib.Context(0)
        try:
            ctx.comm_init(rank, 2, None)
            ctx.halo_set(*dom._halo_plan())
            ctx.mesh_set(dim, dom.conn, dom.xyz)
            assert ctx.n_ghost > 0
            ex, mid = _setup(ctx, block)
            assert ex.colidx.max() >= ctx.n_owned                   # ghost columns are in the graph
            vx, vy = ctx.vec_create(block[1]), ctx.vec_create(block[0])
            ctx.vec_set_local(vx, ex.x.astype(np.float64))
            _plain(ctx, mid, ex, vx, vy, fam, par, f"ghost {gc} rank {rank}")
        finally:
            ctx.close()


@pytest.mark.parametrize("hc", pe.HOLE_CASES, ids=lambda h: h[0])
def test_hole(lib, hc):
    """pyn_sell_spmv_range2 with the hole cut out: one rank that is its own RCCL neighbour; single-reduction CG multiplies the
    interior slices while the halo is in flight, then the bottom and top slices in ONE launch.  With x0 = 0 and no preconditioner
    the first Chronopoulos-Gear step is alpha = gamma / delta = b.b / b.(Af b) on the folded matrix and x1 = alpha b."""
    name, block, nelem, env, (fam, par) = hc
    cut, N, send, fold = pe.hole_mesh(nelem)
    ng = cut.n_node - N
    with knobs(PYNAMA_OVERLAP_REQUIRE=1, **env):
        ctx = lib.Context(0)
        try:
            ctx.comm_init(0, 1, lib.Context.unique_id())
            ctx.halo_set(N, ng, [0], [0, ng], send, [0, ng])
            ctx.mesh_set(cut.dim, cut.conn, cut.xyz)
            ex, mid = _setup(ctx, block, fold=fold, host_graph=pe.host_graph(cut, N))
            br = block[0]
            # the whole product after a real halo exchange: ghosts = x[send]
            vx, vy = ctx.vec_create(br), ctx.vec_create(br)
            xo = ex.x[:N * br]
            ctx.vec_set(vx, xo.astype(np.float64))
            ctx.spmv(mid, vx, vy)
            assert np.array_equal(ctx.vec_get(vy, br), (ex.Af @ xo).astype(np.float64))
            vb, v1 = ctx.vec_create(br), ctx.vec_create(br)
            ctx.vec_set(vb, ex.b.astype(np.float64))
            before = ctx.product_last()["launches"]
            info = ctx.solve(mid, vb, v1, method=lib.KSP_CG, pc=lib.PC_NONE, fixed_iters=1, cg_variant=2)
            assert info.iters == 1
            got = ctx.vec_get(v1, br)
            assert np.array_equal(got, ex.x1()), \
                f"hole {name}: alpha = {got[0] / ex.b[0]!r}, exact gamma / delta = {ex.bb} / {ex.pap} = {ex.bb / ex.pap!r}"
            last = ctx.product_last()
            _expect(last, fam, par, 1, f"hole {name}")
            # w = A u_0 and w = A u_1 (whose scalars end the run), each as interior launch + boundary launch
            assert last["launches"] == before + 4, last
        finally:
            ctx.close()
