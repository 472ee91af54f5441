"""The pivoting LU cases of tests/lu_cases.py against their own claims (no GPU): bandwidths, LAPACK's verdict, how much the
reference interchanges and how small its backward error is.  These conditions are about the reference alone; a seed that misses
one is changed, not the condition.  `pytest -s` prints the table."""
import numpy as np
import pytest

from tests import lu_cases as lc


def test_table_is_consistent():
    assert len({c.name for c in lc.CASES}) == len(lc.CASES)
    assert [c.name for c in lc.CASES if c.main_only] == ["1100x2-b1", "30x43-b3"]
    assert all(c.kinds == (("uni",) if c.main_only else ("int", "uni")) for c in lc.CASES)


@pytest.mark.parametrize("case", lc.CASES, ids=[c.name for c in lc.CASES])
def test_bandwidths_from_the_graph(case):
    mesh, rp, ci = lc.graph(case)
    assert mesh.n_node * case.b == case.n
    lat = mesh.lattice
    dist = sum(int(np.prod(lat[:d])) for d in range(mesh.dim))      # the diagonal neighbour, x fastest
    assert lc.graph_bandwidths(rp, ci, case.b) == (dist * case.b + case.b - 1,) * 2 == (case.kl, case.kl)


@pytest.mark.parametrize("case,kind", lc.MAIN, ids=lc.MAIN_IDS)
def test_reference(case, kind):
    s = lc.build(case, kind)
    assert (s.n, s.kl, s.ku) == (case.n, case.kl, case.kl)
    lo, hi = (-8, 8) if kind == "int" else (-1, 1)
    assert lo <= s.val.min() and s.val.max() <= hi and s.exact_rhs == (kind == "int")
    assert np.abs(s.xs).max() <= 4
    dense = s.A.toarray() if s.n <= 512 else None
    if dense is not None:                                            # the band image is the matrix
        ab = lc.band_storage(s)
        i, j = np.nonzero(dense)
        assert np.array_equal(ab[s.kl + s.ku + i - j, j], dense[i, j]) and np.count_nonzero(ab) == i.size
    ref = lc.reference_of(case, kind)
    st = lc.pivot_stats(ref.ipiv)
    what = (f"{case.name}-{kind}: n {s.n} kl {s.kl} info {ref.info} share {st['share']:.2f} dist {st['dist']} "
            f"({st['dist'] / s.kl:.2f} kl) sub-block border {st['cross_sub']} panel border {st['cross_panel']} "
            f"eta(x_ref) {ref.eta / lc.EPS:.2f} eps")
    print(what)
    assert ref.info == 0, what
    assert st["share"] >= 0.6, what
    assert st["dist"] >= 0.75 * s.kl, what
    if s.n > lc.SUB:                       # no row beyond the first sub-block otherwise (n = 4)
        assert st["cross_sub"], what
    if s.n > lc.PANEL:
        assert st["cross_panel"], what
    assert ref.eta <= 16 * lc.EPS, what
    if dense is not None:                                            # the measure itself: same figure from a dense longdouble residual
        L = np.longdouble
        r = np.abs(s.b.astype(L) - dense.astype(L) @ ref.x.astype(L)).max()
        assert abs(float(r) / lc.scale_of(s, ref.x) - ref.eta) <= 1e-3 * lc.EPS
        want = np.abs(dense).sum(axis=1).max() * np.abs(ref.x).max() + np.abs(s.b).max()
        assert abs(lc.scale_of(s, ref.x) - want) <= 8 * lc.EPS * want


@pytest.mark.parametrize("name", ["4x12-b1", "9x6-b2"])
def test_both_residual_paths_agree(name):
    """longdouble and exact-product fsum give the same eta to well below eps"""
    s = lc.build(lc.BY_NAME[name], "uni")
    x = lc.reference_of(lc.BY_NAME[name], "uni").x
    a, b = lc.eta(s, x, longdouble=False), lc.eta(s, x, longdouble=True)
    if lc.LONGDOUBLE_OK:
        assert abs(a - b) <= 1e-3 * lc.EPS, (a, b)
    bad = x.copy()
    bad[3] += 1e-6
    assert lc.eta(s, bad, longdouble=False) > 1e6 * lc.EPS
    bad[3] = np.nan
    assert np.isnan(lc.eta(s, bad))


def test_integer_systems_are_exact():
    s = lc.build(lc.SINGULAR_CASE, "int")
    assert s.exact_rhs and np.array_equal(s.b, np.rint(s.b))
    assert lc.residual_inf(s, s.xs.astype(np.float64)) == 0.0 == lc.residual_inf(s, s.xs.astype(np.float64), longdouble=False)


@pytest.mark.parametrize("k", lc.ZERO_COLUMNS)
def test_zero_column_is_reported_by_lapack(k):
    s = lc.build(lc.SINGULAR_CASE, "int")
    rows, vals = lc.column_entries(s, k)
    assert rows.size >= 4 and np.all(np.abs(rows - k) <= s.kl)
    val = s.val.copy()
    val[s.C == k] = 0.0
    z = lc.with_values(s, val)
    assert lc.lapack_factor(z)[2] == k + 1
    assert lc.reference(z).x is None
    assert np.array_equal(lc.with_values(z, s.val).A.toarray(), s.A.toarray())


def test_mutated_systems_keep_a_small_reference_error():
    """what the cache tests do to the values (scaled rows, replaced rows, sums of two draws) leaves LAPACK's eta at a few eps"""
    for case in lc.CACHE_CASES:
        for kind in case.kinds:
            s = lc.build(case, kind)
            rng = np.random.default_rng(77)
            other = lc.draw_values(kind, s.val.size, rng)
            scale = rng.uniform(0.5, 2.0, s.n) * rng.choice([-1.0, 1.0], s.n)
            for val in (s.val + 0.5 * other, s.val * scale[s.R], other):
                m = lc.with_values(s, val, lc.draw_solution(s.n, rng))
                ref = lc.reference(m)
                assert ref.info == 0 and ref.eta <= 16 * lc.EPS, (case.name, kind, ref.eta / lc.EPS)
