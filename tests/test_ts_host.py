"""TsSolver on the host: Butcher order conditions in exact rationals, the TSADAPTBASIC controller, the step loop driven by a
numpy stand-in for the two device passes, option parsing and the reference layout.  No GPU."""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

from pynama_amd.common.options import Options
from pynama_amd.solver import ts_solver
from pynama_amd.solver.ts_solver import TABLEAUX, TsSolver, adapt_basic


# ---- order conditions ----------------------------------------------------------------------------------------------------
def rooted_trees(order):
    """all rooted trees with `order` nodes, a tree = sorted tuple of its subtrees"""
    if order == 1:
        return [()]
    out = set()

    def forests(n, min_tree=None):
        # multisets of trees with n nodes in total, in non-decreasing order (by (size, repr))
        if n == 0:
            yield ()
            return
        for k in range(1, n + 1):
            for t in rooted_trees(k):
                key = (k, repr(t))
                if min_tree is not None and key < min_tree:
                    continue
                for rest in forests(n - k, key):
                    yield (t,) + rest
    for f in forests(order - 1):
        out.add(tuple(sorted(f, key=lambda t: (size(t), repr(t)))))
    return sorted(out, key=repr)


def size(t):
    return 1 + sum(size(c) for c in t)


def gamma(t):
    g = size(t)
    for c in t:
        g *= gamma(c)
    return g


def stage_weights(A, t):
    """Phi_i(t) = prod over children of sum_j a_ij Phi_j(child)"""
    s = len(A)
    phi = [Fr(1)] * s
    for c in t:
        pc = stage_weights(A, c)
        phi = [phi[i] * sum(A[i][j] * pc[j] for j in range(s)) for i in range(s)]
    return phi


def order_conditions_hold(A, b, p):
    n = 0
    for q in range(1, p + 1):
        for t in rooted_trees(q):
            if sum(bi * ph for bi, ph in zip(b, stage_weights(A, t))) != Fr(1, gamma(t)):
                return False, n
            n += 1
    return True, n


def test_tree_counts():
    assert [len(rooted_trees(q)) for q in range(1, 6)] == [1, 1, 2, 4, 9]        # 17 conditions up to order 5


@pytest.mark.parametrize("name", sorted(TABLEAUX))
def test_order_conditions(name):
    tab = TABLEAUX[name]
    ok, n = order_conditions_hold(tab.A, tab.b, tab.order)
    assert ok and n == sum(len(rooted_trees(q)) for q in range(1, tab.order + 1))
    # not one order more
    assert not order_conditions_hold(tab.A, tab.b, tab.order + 1)[0]
    if tab.embedded:
        assert order_conditions_hold(tab.A, tab.bhat, tab.embedded_order)[0]
        assert not order_conditions_hold(tab.A, tab.bhat, tab.embedded_order + 1)[0]


@pytest.mark.parametrize("name", sorted(TABLEAUX))
def test_tableau_structure(name):
    tab = TABLEAUX[name]
    assert len(tab.A) == tab.s == len(tab.c) and tab.s <= 8
    for i in range(tab.s):
        assert sum(tab.A[i]) == tab.c[i]                                   # row sums = c
        assert all(tab.A[i][j] == 0 for j in range(i, tab.s))               # explicit
    if tab.fsal:
        assert tab.A[-1] == tab.b and tab.c[-1] == 1                        # last row is b: its stage is f at the new state
    assert [float(v) for v in tab.b] == tab.b_f                             # doubles converted once from the rationals


def test_5bs_coefficients_as_given():
    tab = TABLEAUX["5bs"]
    assert tab.c == [0, Fr(1, 6), Fr(2, 9), Fr(3, 7), Fr(2, 3), Fr(3, 4), 1, 1]
    assert tab.A[6][5] == Fr(482048, 414219) and tab.bhat[7] == Fr(3293, 556956)
    assert (tab.order, tab.embedded_order, TABLEAUX["3bs"].order, TABLEAUX["3bs"].embedded_order) == (5, 4, 3, 2)
    assert not TABLEAUX["4"].embedded and not TABLEAUX["4"].fsal


# ---- controller ------------------------------------------------------------------------------------------------------------
def test_adapt_factor_and_clip():
    acc, h = adapt_basic(0.2, 0.5, 5, False)
    assert acc and h == pytest.approx(0.2 * 0.9 * 0.5 ** (-1 / 5), rel=1e-15)
    assert adapt_basic(0.2, 1.0, 5, False)[0]                         # e = 1 is accepted
    acc, h = adapt_basic(0.2, 0.0, 5, False)
    assert acc and h == pytest.approx(2.0, rel=1e-15)                  # e = 0: factor 10
    acc, h = adapt_basic(0.2, 1e-30, 5, False)
    assert acc and h == pytest.approx(2.0, rel=1e-15)                  # clipped at 10
    acc, h = adapt_basic(0.2, 1e30, 5, False)
    assert not acc and h == pytest.approx(0.02, rel=1e-15)             # clipped at 0.1
    acc, h = adapt_basic(0.1, 3.0, 3, False)
    assert not acc and h == pytest.approx(0.1 * 0.9 * 3.0 ** (-1 / 3), rel=1e-15)


def test_adapt_consecutive_reject_safety():
    _, h1 = adapt_basic(0.1, 3.0, 5, False)
    _, h2 = adapt_basic(0.1, 3.0, 5, True)
    assert h2 == pytest.approx(0.5 * h1, rel=1e-15)
    _, h3 = adapt_basic(0.1, 0.5, 5, True)                               # an accepted attempt keeps the plain safety
    assert h3 == pytest.approx(0.1 * 0.9 * 0.5 ** (-1 / 5), rel=1e-15)


@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_adapt_nan_rejects(bad):
    acc, h = adapt_basic(0.4, bad, 5, False)
    assert not acc and h == pytest.approx(0.04, rel=1e-15)


# ---- the step loop on a numpy stand-in of the device passes -----------------------------------------------------------------
class _NpVec:
    def __init__(self, a):
        self.a = np.array(a, dtype=float)


class _NpStages:
    def __init__(self, u, s):
        self.K = [_NpVec(np.zeros_like(u.a)) for _ in range(s)]
        self.Y = _NpVec(np.zeros_like(u.a))
        self.u = u

    def fits(self, u, s):
        return u is self.u and len(self.K) == s

    def maxpy(self, y, x, vecs, w):
        r = x.a.copy()
        for v, wj in zip(vecs, w):
            r = r + wj * v.a
        y.a[:] = r

    def finish(self, x, vecs, hb, hd, atol, rtol):
        d = np.zeros_like(x.a)
        for j, v in enumerate(vecs):
            x.a += hb[j] * v.a
            if hd is not None:
                d += hd[j] * v.a
        if hd is None:
            return None
        tol = atol + rtol * np.maximum(np.abs(x.a), np.abs(x.a + d))
        return float(np.sqrt(np.mean((np.abs(d) / tol) ** 2)))


class _HostTs(TsSolver):
    def _stages_for(self, u, s):
        if self._stages is None or not self._stages.fits(u, s):
            self._stages = _NpStages(u, s)
        return self._stages


@pytest.fixture
def clean_options():
    saved = Options._db
    Options(argv=[])
    yield
    Options._db = saved


def _decay(ts, t, X, F, lam):
    F.a[:] = lam * X.a


def test_loop_matchstep_lands_on_max_time(clean_options):
    lam = np.array([-1.0, -0.5, -2.0])
    ts = _HostTs()
    ts.setRHSFunction(_decay, args=(lam,))
    ts.setTimeStep(0.3)
    ts.setMaxTime(1.0)
    ts.setTolerances(rtol=1e-6, atol=1e-6)
    seen = []
    ts.setPostStep(lambda t: seen.append((t.getStepNumber(), t.getTime())))
    u = _NpVec(np.ones(3))
    ts.solve(u)
    assert ts.getConvergedReason() == 1 and ts.getTime() == 1.0
    assert [s for s, _ in seen] == list(range(1, len(seen) + 1)) and seen[-1][1] == 1.0
    assert all(b > a for (_, a), (_, b) in zip(seen, seen[1:]))
    assert np.abs(u.a - np.exp(lam)).max() < 1e-5
    # FSAL: 8 evaluations on the first attempt, 7 on every later one
    assert ts.rhs_evals == 8 + 7 * (ts.getStepNumber() + ts.getStepRejections() - 1)


def test_loop_fixed_steps_and_max_steps(clean_options):
    ts = _HostTs()
    ts.setRKType("4")
    assert ts.getAdaptType() == "none"
    ts.setRHSFunction(_decay, args=(np.array([-1.0]),))
    ts.setTimeStep(0.1)
    ts.setMaxSteps(4)
    u = _NpVec([1.0])
    ts.solve(u)
    assert ts.getConvergedReason() == 2 and ts.getStepNumber() == 4 and ts.getTime() == pytest.approx(0.4)
    r = 1 - 0.1 + 0.1 ** 2 / 2 - 0.1 ** 3 / 6 + 0.1 ** 4 / 24                 # RK4 amplification factor on y' = -y
    assert u.a[0] == pytest.approx(r ** 4, rel=1e-14) and ts.rhs_evals == 16


def test_loop_gives_up_after_max_reject(clean_options):
    def blow_up(ts, t, X, F):
        F.a[:] = np.inf
    ts = _HostTs()
    ts.setRHSFunction(blow_up)
    calls = []
    ts.setPostStep(lambda t: calls.append(1))
    ts.setMaxStepRejections(3)
    with np.errstate(invalid="ignore"):
        ts.solve(_NpVec(np.ones(4)))
    assert ts.getConvergedReason() == -2 and ts.getStepRejections() == 4 and ts.getStepNumber() == 0 and not calls
    assert ts.getTimeStep() == pytest.approx(0.1 * 1e-4)                   # factor 0.1 per NaN rejection


def test_loop_rejection_rolls_back(clean_options):
    lam = np.array([-50.0, -1.0])
    ts = _HostTs()
    ts.setRHSFunction(_decay, args=(lam,))
    ts.setTimeStep(0.5)
    ts.setMaxTime(0.5)
    ts.setTolerances(1e-8, 1e-8)
    u = _NpVec([1.0, 1.0])
    ts.solve(u)
    assert ts.getStepRejections() >= 1 and ts.getConvergedReason() == 1
    assert np.abs(u.a - np.exp(lam * 0.5)).max() < 1e-6


# ---- options and layout ------------------------------------------------------------------------------------------------------
def test_defaults(clean_options):
    ts = TsSolver()
    assert (ts.getType(), ts.getRKType(), ts.getTimeStep(), ts.getMaxTime(), ts.getMaxSteps()) == ("rk", "5bs", 0.1, 5.0, 5000)
    assert ts.getTolerances() == (1e-4, 1e-4) and ts.max_reject == 10 and ts.getAdaptType() == "basic"
    assert ts.exact_final_time == TsSolver.ExactFinalTime.MATCHSTEP
    assert (ts.getTime(), ts.step_number, ts.getStepRejections(), ts.getConvergedReason()) == (0.0, 0, 0, 0)


def test_options_parsed(clean_options):
    Options(argv=["-ts_type", "rk", "-ts_rk_type", "3bs", "-ts_dt", "0.02", "-ts_max_time", "2.5", "-ts_max_steps", "7",
                  "-ts_adapt_type", "none", "-ts_rtol", "1e-7", "-ts_atol", "1e-9", "-ts_max_reject", "4",
                  "-ts_exact_final_time", "stepover"])
    ts = TsSolver()
    assert (ts.getRKType(), ts.getTimeStep(), ts.getMaxTime(), ts.getMaxSteps()) == ("3bs", 0.02, 2.5, 7)
    assert ts.getAdaptType() == "none" and ts.getTolerances() == (1e-7, 1e-9) and ts.max_reject == 4
    assert ts.exact_final_time == TsSolver.ExactFinalTime.STEPOVER


def test_rk4_forces_no_adaptivity(clean_options):
    Options(argv=["-ts_rk_type", "4", "-ts_adapt_type", "basic"])
    assert TsSolver().getAdaptType() == "none"


@pytest.mark.parametrize("argv", [["-ts_type", "beuler"], ["-ts_rk_type", "8vr"], ["-ts_adapt_type", "dsp"],
                                  ["-ts_exact_final_time", "interpolate"]])
def test_unsupported_options_raise(clean_options, argv):
    Options(argv=argv)
    with pytest.raises(ValueError):
        TsSolver()


def test_setters_refuse_other_types(clean_options):
    ts = TsSolver()
    with pytest.raises(ValueError):
        ts.setType("theta")
    ts.setRKType("4")
    assert ts.getRKType() == "4"


def test_solve_needs_rhs(clean_options):
    with pytest.raises(RuntimeError):
        _HostTs().solve(_NpVec([1.0]))


def test_reference_layout_import():
    import pynama_amd
    pynama_amd.install_reference_layout()
    from solver.ts_solver import TsSolver as T
    assert T is TsSolver and ts_solver.TsSolver is T


def test_base_problem_time_solver_settings(clean_options):
    """setUpTimeSolver without a mesh: yaml block, then constructor kwargs, then options"""
    from pynama_amd.cases.base_problem import BaseProblem

    class _P(BaseProblem):
        def __init__(self, config, **kw):          # only what setUpTimeSolver reads
            self.config, self.opts = config, kw
            from pynama_amd.common.comm import get_world
            self.comm = get_world()

    cfg = {"time-solver": {"start-time": 0.25, "end-time": 2.0, "max-steps": 11}, "save-n-steps": 3}
    p = _P(cfg)
    p.setUpTimeSolver()
    assert (p.ts.getTime(), p.ts.getMaxTime(), p.ts.getMaxSteps(), p._saveEvery) == (0.25, 2.0, 11, 3)
    assert p.ts._rhs[0] == p.evalRHS and p.ts._post[0] == p.convergedStepFunction
    p = _P(cfg, endTime=0.5, maxSteps=20)
    p.setUpTimeSolver()
    assert (p.ts.getTime(), p.ts.getMaxTime(), p.ts.getMaxSteps()) == (0.25, 0.5, 20)
    Options(argv=["-ts_max_time", "0.75"])
    p.setUpTimeSolver()
    assert (p.ts.getMaxTime(), p.ts.getMaxSteps()) == (0.75, 20)
    p = _P({})
    p.setUpTimeSolver()
    assert (p.ts.getTime(), p.ts.getMaxTime(), p.ts.getMaxSteps()) == (0.0, 0.75, 5000)

