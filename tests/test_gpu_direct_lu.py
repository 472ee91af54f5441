"""Pivoting and block-edge tests of the two direct solvers, pyn_solve_direct (pyn_direct.hip) and pyn_solve_direct_band
(pyn_direct_band.hip), on a real MI355X (`-m gpu`).

The systems of tests/lu_cases.py hold random values on every stored entry, so most columns interchange, at distances up to kl and
across the sub-block (8) and panel (64) borders; the sizes sit on the edges of the index arithmetic (n below, at and just above a
panel, a last panel that is no multiple of 8, kl + ku below a panel, kl at 63 / 64 / 65 and above the 1,024 threads of the panel
kernel).  Every system goes through BOTH solvers on one matrix handle, dense first, so both factor caches live side by side.
The reference is LAPACK's dgbtrf / dgbtrs and the measure the normwise backward error eta of lu_cases: the uploaded values are
read back bit-equal first, so a small eta means that this exact matrix was solved.  `pytest -s` prints eta(x_dev) / eta(x_ref) per
case and solver (direct solve, holds the table).

A context needs mesh_set and csr_symbolic only: no element tables, no assembly.  Meshes and contexts are built once per module, the
main systems are uploaded once per case and kind; the tests that change values do so on handles of their own."""
import math
import re

import numpy as np
import pytest

from tests import lu_cases as lc
from tests import product_exact as pe

pytestmark = pytest.mark.gpu

SOLVERS = ("dense", "band")
SENTINEL = 7.0            # x before every solve: a solver that writes nothing does not inherit the other one's solution


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


class Bench:
    def __init__(self, lib):
        self.lib = lib
        self.ctxs, self.mains = {}, {}

    def ctx_of(self, case):
        """(context with the case's graph, b vector, x vector)"""
        if case not in self.ctxs:
            mesh, rp, ci = lc.graph(case)
            ctx = self.lib.Context(0)
            self.ctxs[case] = (ctx,)
            ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
            ctx.csr_symbolic()
            drp, dci = ctx.csr_get()
            assert np.array_equal(drp, rp) and np.array_equal(dci, ci)
            self.ctxs[case] = (ctx, ctx.vec_create(case.b), ctx.vec_create(case.b))
        return self.ctxs[case]

    def upload(self, case, s):
        """a new matrix handle with the values of s, read back bit-equal"""
        ctx = self.ctx_of(case)[0]
        mid = ctx.mat_create(s.br, s.bc)
        pe.upload(ctx, mid, s)
        assert np.array_equal(ctx.mat_values(mid, s.br, s.bc), s.val)
        return mid

    def main(self, case, kind):
        """the case's system, uploaded once; read-only"""
        if (case, kind) not in self.mains:
            self.mains[(case, kind)] = self.upload(case, lc.build(case, kind))
        return self.mains[(case, kind)]

    def close(self):
        for c in self.ctxs.values():
            if c is not None:
                c[0].close()


@pytest.fixture(scope="module")
def bench(lib):
    b = Bench(lib)
    yield b
    b.close()


def _run(ctx, which, mid, vb, vx):
    return ctx.solve_direct(mid, vb, vx) if which == "dense" else ctx.solve_direct_band(mid, vb, vx)


def _judge(ctx, s, ref, mid, vb, vx, what):
    """both solvers on the handle against the bar of the reference; returns the misses"""
    assert ref.info == 0 and ref.eta <= 16 * lc.EPS, f"{what}: the reference itself: info {ref.info}, eta {ref.eta / lc.EPS:.2f} eps"
    ctx.vec_set(vb, s.b)
    bad = []
    for which in SOLVERS:
        ctx.vec_fill(vx, SENTINEL)
        info = _run(ctx, which, mid, vb, vx)
        x = ctx.vec_get(vx, s.br)
        e = lc.eta(s, x)
        tag = f"{what} {which}"
        print(f"{tag}: eta(x_dev) {e / lc.EPS:.2f} eps, eta(x_ref) {ref.eta / lc.EPS:.2f} eps, "
              f"ratio {e / max(ref.eta, lc.EPS):.2f} of at most {lc.MARGIN:g}; true_resid {info.true_resid:.2e}")
        if not e <= ref.bar:
            bad.append(f"{tag}: eta(x_dev) = {e / lc.EPS:.3g} eps above {lc.MARGIN:g} max(eta(x_ref), eps) = {ref.bar / lc.EPS:.3g} eps")
            continue
        if (info.iters, info.reason) != (1, 4):
            bad.append(f"{tag}: iters {info.iters}, reason {info.reason}")
        if s.exact_rhs:
            bi = np.rint(s.b).astype(np.int64)
            want = math.sqrt(float(int((bi * bi).sum())))
            if info.rnorm0 != want:
                bad.append(f"{tag}: rnorm0 {info.rnorm0!r} != {want!r}")
        elif not abs(info.rnorm0 - np.linalg.norm(s.b)) <= 1e-14 * np.linalg.norm(s.b) * math.sqrt(s.n):
            bad.append(f"{tag}: rnorm0 {info.rnorm0!r}, ||b|| {np.linalg.norm(s.b)!r}")
        bound = lc.true_resid_bound(s, ref.bar, x)
        if not info.true_resid <= bound:
            bad.append(f"{tag}: true_resid {info.true_resid:.3e} above {bound:.3e}")
    return bad


@pytest.mark.parametrize("case,kind", lc.MAIN, ids=lc.MAIN_IDS)
def test_backward_error_of_both_solvers(bench, case, kind):
    s, ref = lc.build(case, kind), lc.reference_of(case, kind)
    ctx, vb, vx = bench.ctx_of(case)
    mid = bench.main(case, kind)
    kl, ku, nbytes = ctx.direct_band_info(mid)
    assert (kl, ku) == (case.kl, case.kl) == (s.kl, s.ku)
    assert nbytes >= s.n * (2 * kl + ku + 1) * 8
    assert s.n <= ctx.direct_max_rows()
    bad = _judge(ctx, s, ref, mid, vb, vx, f"{case.name}-{kind}")
    assert not bad, "\n".join(bad)
    assert np.array_equal(ctx.mat_values(mid, s.br, s.bc), s.val)          # a solve leaves the matrix alone


def _column_of(msg):
    m = re.search(r"zero pivot in column (\d+)", msg)
    assert m, msg
    return int(m.group(1))


@pytest.mark.parametrize("k", lc.ZERO_COLUMNS)
def test_zero_column_names_the_first_singular_column(bench, lib, k):
    """every stored entry of column k zeroed: LAPACK's info is k + 1 (tests/test_lu_cases_host.py); both solvers name column k --
    the first zero pivot, not a later column that the division by zero filled with NaN -- and leave no factors marked valid;
    with the column restored both meet the bar again"""
    case = lc.SINGULAR_CASE
    s, ref = lc.build(case, "int"), lc.reference_of(case, "int")
    ctx, vb, vx = bench.ctx_of(case)
    mid = bench.upload(case, s)
    bad = _judge(ctx, s, ref, mid, vb, vx, f"before column {k}")            # both caches hold factors of the regular matrix
    assert not bad, "\n".join(bad)
    rows, vals = lc.column_entries(s, k)
    ctx.mat_add_values(mid, rows, [k], np.zeros(rows.size), insert=True)
    zeroed = s.val.copy()
    zeroed[s.C == k] = 0.0
    assert np.array_equal(ctx.mat_values(mid, 1, 1), zeroed)
    for attempt in (1, 2):                                                  # the second call must not find a "valid" cache
        for which in SOLVERS:
            with pytest.raises(lib.PynamaHipError, match="zero pivot") as ei:
                _run(ctx, which, mid, vb, vx)
            assert _column_of(str(ei.value)) == k, f"{which}, attempt {attempt}: {ei.value}"
    ctx.mat_add_values(mid, rows, [k], vals, insert=True)
    assert np.array_equal(ctx.mat_values(mid, 1, 1), s.val)
    bad = _judge(ctx, s, ref, mid, vb, vx, f"column {k} restored")
    assert not bad, "\n".join(bad)
    ctx.mat_destroy(mid)


def test_nan_entry_is_never_a_converged_solve(bench, lib):
    """one NaN in the matrix: each solver raises or reports PYN_DIVERGED_NANORINF (-9), never a positive reason"""
    case = lc.SINGULAR_CASE
    s, ref = lc.build(case, "int"), lc.reference_of(case, "int")
    ctx, vb, vx = bench.ctx_of(case)
    mid = bench.upload(case, s)
    ctx.vec_set(vb, s.b)
    for r, c in lc.NAN_ENTRIES:
        old = s.A[r, c]
        assert np.any((s.R == r) & (s.C == c))
        ctx.mat_add_values(mid, [r], [c], [np.nan], insert=True)
        for which in SOLVERS:
            ctx.vec_fill(vx, SENTINEL)
            try:
                info = _run(ctx, which, mid, vb, vx)
            except lib.PynamaHipError as e:
                print(f"NaN at ({r}, {c}) {which}: raises: {e}")
                continue
            print(f"NaN at ({r}, {c}) {which}: reason {info.reason}")
            assert info.reason == -9, f"NaN at ({r}, {c}) {which}: reason {info.reason}, true_resid {info.true_resid}"
        ctx.mat_add_values(mid, [r], [c], [old], insert=True)
        assert np.array_equal(ctx.mat_values(mid, 1, 1), s.val)
    bad = _judge(ctx, s, ref, mid, vb, vx, "NaN entries restored")
    assert not bad, "\n".join(bad)
    ctx.mat_destroy(mid)


def _put_rows(ctx, mid, s, nodes, val, insert):
    """the node rows `nodes` of the header-layout array val into the matrix (one call per node row, as product_exact.upload)"""
    b = s.br
    pr = np.arange(b, dtype=np.int32)
    for i in nodes:
        lo, hi = int(s.rowptr[i]), int(s.rowptr[i + 1])
        cols = (s.colidx[lo:hi, None] * b + pr[None, :]).ravel()
        ctx.mat_add_values(mid, i * b + pr, cols, val[lo * b * b:hi * b * b], insert=insert)


def _rows_mask(s, nodes):
    m = np.zeros(s.val.size, bool)
    for i in nodes:
        m[int(s.rowptr[i]) * s.br * s.br:int(s.rowptr[i + 1]) * s.br * s.br] = True
    return m


CACHE = [(c, k) for c in lc.CACHE_CASES for k in c.kinds]


@pytest.mark.parametrize("case,kind", CACHE, ids=[f"{c.name}-{k}" for c, k in CACHE])
def test_factor_caches_follow_the_values(bench, lib, case, kind):
    """after every way the values can change, both solvers solve the NEW matrix (reference rebuilt from mat_values); a second
    right-hand side without a change in between is solved as well"""
    s, ref = lc.build(case, kind), lc.reference_of(case, kind)
    ctx, vb, vx = bench.ctx_of(case)
    b = case.b
    mid = bench.upload(case, s)
    rng = np.random.default_rng(1000 + case.seed)
    bad = _judge(ctx, s, ref, mid, vb, vx, f"{case.name}-{kind} first")
    s2 = lc.with_values(s, s.val, lc.draw_solution(s.n, rng))
    bad += _judge(ctx, s2, lc.reference(s2), mid, vb, vx, f"{case.name}-{kind} second right-hand side")
    assert not bad, "\n".join(bad)

    n_nodes = s.rowptr.size - 1
    nodes = sorted({0, n_nodes // 2, n_nodes - 1})
    mask = _rows_mask(s, nodes)
    delta = 8.0 * lc.draw_values(kind, s.val.size, rng)          # large enough to move the pivots of those rows
    fresh_rows = lc.draw_values(kind, s.val.size, rng)
    other = lc.draw_values(kind, s.val.size, rng)
    other_s = lc.with_values(s, other)
    scale = rng.uniform(0.5, 2.0, s.n) * rng.choice([-1.0, 1.0], s.n)
    final = lc.draw_values(kind, s.val.size, rng)
    xmat = bench.upload(case, other_s)
    vs = ctx.vec_create(b)
    ctx.vec_set(vs, scale)

    def add(v):
        _put_rows(ctx, mid, s, nodes, delta, insert=False)
        return np.where(mask, v + delta, v)

    def insert(v):
        _put_rows(ctx, mid, s, nodes, fresh_rows, insert=True)
        return np.where(mask, fresh_rows, v)

    def axpy(v):
        ctx.mat_axpy(mid, 0.5, xmat)
        return v + 0.5 * other

    def row_scale(v):
        ctx.mat_row_scale(mid, vs)
        return v * scale[s.R]

    def zero_upload(v):
        ctx.mat_zero(mid)
        assert not ctx.mat_values(mid, b, b).any()
        _put_rows(ctx, mid, s, range(n_nodes), final, insert=True)
        return final

    want = s.val
    for step in (add, insert, axpy, row_scale, zero_upload):
        want = step(want)
        got = ctx.mat_values(mid, b, b)
        assert np.array_equal(got, want), f"{step.__name__}: {np.count_nonzero(got != want)} values differ"
        m = lc.with_values(s, got, lc.draw_solution(s.n, rng))
        bad = _judge(ctx, m, lc.reference(m), mid, vb, vx, f"{case.name}-{kind} after {step.__name__}")
        assert not bad, "\n".join(bad)
    assert np.array_equal(ctx.mat_values(xmat, b, b), other)     # the X argument of mat_axpy is unchanged
    ctx.vec_destroy(vs)
    ctx.mat_destroy(xmat)
    ctx.mat_destroy(mid)


def test_refusals_of_block_size_and_shape(bench, lib):
    case = lc.BY_NAME["9x6-b2"]
    ctx, vb, vx = bench.ctx_of(case)
    mid = bench.main(case, "int")
    v1 = ctx.vec_create(1)
    rect = ctx.mat_create(2, 1)
    for which in SOLVERS:
        for args in ((mid, v1, vx), (mid, vb, v1)):
            with pytest.raises(lib.PynamaHipError, match="block size"):
                _run(ctx, which, *args)
        with pytest.raises(lib.PynamaHipError, match="square"):
            _run(ctx, which, rect, vb, vx)
    with pytest.raises(lib.PynamaHipError, match="square"):
        ctx.direct_band_info(rect)
    ctx.mat_destroy(rect)
    ctx.vec_destroy(v1)
