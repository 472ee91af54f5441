"""Explicit Runge-Kutta time integrator with the petsc4py ``TS`` surface the reference uses.

The reference's ``TsSolver(PETSc.TS)`` sets ``rk`` / ``5bs`` and ``MATCHSTEP`` and then reads the options; ``BaseProblem`` gives it
``evalRHS`` as the right-hand side and ``convergedStepFunction`` as the post-step callback.  Here the state stays on the device:
the stage vectors ``K_0 .. K_{s-1}`` and one stage state ``Y`` are ``Vec``s of the state's block size, allocated once per solver,
and every vector pass of a step is one of two library calls (``pyn_vec_maxpy``, ``pyn_ts_step_finish``).  The weighted error
norm is the only device->host read of a step; no field is copied to the host inside ``solve``.

One step of ``h`` (TSStep_RK):
  1. for each stage i: ``Y = X + sum_{j<i} h a_ij K_j`` and ``K_i = f(t + c_i h, Y)``.  The callback may write into ``X``
     (``CustomFuncCase.applyBoundaryConditions`` resets the boundary vorticity of the state), so ``X`` is re-read by every pass;
  2. FSAL tableaux (``5bs``, ``3bs``): ``K_0`` is evaluated on the first step only, later it is the last ``K`` of the previous
     accepted step (the vectors are swapped, not copied); a rejected attempt keeps its ``K_0``;
  3. ``X += sum_j h b_j K_j`` in place, with the weighted RMS norm of ``d = sum_j h (bhat_j - b_j) K_j`` when adaptive.

Controller (TSADAPTBASIC, scalar tolerances): accept when the norm ``e <= 1``; the next step is
``h clip(safety e^(-1/p), 0.1, 10)`` with ``p`` the order of the scheme, safety 0.9, halved when the previous attempt at the
same step was rejected as well; ``e = 0`` gives the factor 10, a NaN or Inf norm is a rejection with the factor 0.1.  A
rejection rolls ``X`` back (``X -= sum_j h b_j K_j``, the same maxpy with negated weights) and retries; more than
``max_reject`` rejections of one step end the solve with reason -2 (``TS_DIVERGED_STEP_REJECTED``).  ``MATCHSTEP`` shortens
the step that would pass ``max_time`` and lands on it exactly.  Reasons: 1 ``TS_CONVERGED_TIME``, 2 ``TS_CONVERGED_ITS``.
The post-step callback runs once per accepted step.  A callback that changes the state (the immersed-boundary correction does) calls
``restartStep()`` -- the role of PETSc's ``TSRestartStep`` -- and the next step evaluates stage 0 at the changed state instead of
taking the FSAL stage of the step before; ``getPrevTime()`` is the time before the last accepted step.

Options (PETSc names): ``-ts_type rk`` (any other type raises), ``-ts_rk_type 5bs|3bs|4``, ``-ts_dt``, ``-ts_max_time``,
``-ts_max_steps``, ``-ts_adapt_type basic|none`` (default ``basic`` for a tableau with an embedded pair; ``4`` has none and always
runs with ``none``), ``-ts_rtol``, ``-ts_atol``, ``-ts_max_reject``, ``-ts_exact_final_time matchstep|stepover``.
Defaults: dt 0.1, rtol = atol = 1e-4, max_time 5.0, max_steps 5000, max_reject 10 -- PETSc 3.11-3.13's documented defaults as
recalled, not checked against a PETSc installation.
"""
import logging
from fractions import Fraction as Fr

import numpy as np

from pynama_amd.common.options import Options
from pynama_amd.vectors import Vec


class Tableau:
    """Butcher tableau kept in exact rationals (``A``, ``b``, ``bhat``, ``c``) and converted to double once."""

    def __init__(self, name, order, A, b, c, bhat=None, embedded_order=None, fsal=False):
        self.name, self.order, self.embedded_order, self.fsal = name, order, embedded_order, fsal
        self.s = len(b)
        self.A = [[Fr(v) for v in row] + [Fr(0)] * (self.s - len(row)) for row in A]
        self.b, self.c = [Fr(v) for v in b], [Fr(v) for v in c]
        self.bhat = [Fr(v) for v in bhat] if bhat is not None else None
        self.a_f = [[float(v) for v in row] for row in self.A]
        self.b_f, self.c_f = [float(v) for v in self.b], [float(v) for v in self.c]
        self.d_f = [float(bh - bb) for bh, bb in zip(self.bhat, self.b)] if self.bhat is not None else None

    @property
    def embedded(self):
        return self.bhat is not None


def _f(s):
    return Fr(s)


TABLEAUX = {
    # Bogacki-Shampine 5(4), 8 stages, FSAL (PETSc TSRK5BS)
    "5bs": Tableau(
        "5bs", 5,
        A=[[],
           [_f("1/6")],
           [_f("2/27"), _f("4/27")],
           [_f("183/1372"), _f("-162/343"), _f("1053/1372")],
           [_f("68/297"), _f("-4/11"), _f("42/143"), _f("1960/3861")],
           [_f("597/22528"), _f("81/352"), _f("63099/585728"), _f("58653/366080"), _f("4617/20480")],
           [_f("174197/959244"), _f("-30942/79937"), _f("8152137/19744439"), _f("666106/1039181"), _f("-29421/29068"),
            _f("482048/414219")],
           [_f("587/8064"), 0, _f("4440339/15491840"), _f("24353/124800"), _f("387/44800"), _f("2152/5985"), _f("7267/94080")]],
        b=[_f("587/8064"), 0, _f("4440339/15491840"), _f("24353/124800"), _f("387/44800"), _f("2152/5985"), _f("7267/94080"), 0],
        c=[0, _f("1/6"), _f("2/9"), _f("3/7"), _f("2/3"), _f("3/4"), 1, 1],
        bhat=[_f("2479/34992"), 0, _f("123/416"), _f("612941/3411720"), _f("43/1440"), _f("2272/6561"), _f("79937/1113912"),
              _f("3293/556956")],
        embedded_order=4, fsal=True),
    # Bogacki-Shampine 3(2), 4 stages, FSAL (PETSc TSRK3BS; scipy's RK23)
    "3bs": Tableau(
        "3bs", 3,
        A=[[], [_f("1/2")], [0, _f("3/4")], [_f("2/9"), _f("1/3"), _f("4/9")]],
        b=[_f("2/9"), _f("1/3"), _f("4/9"), 0],
        c=[0, _f("1/2"), _f("3/4"), 1],
        bhat=[_f("7/24"), _f("1/4"), _f("1/3"), _f("1/8")],
        embedded_order=2, fsal=True),
    # classic fourth-order Runge-Kutta (PETSc TSRK4), no embedded pair
    "4": Tableau(
        "4", 4,
        A=[[], [_f("1/2")], [0, _f("1/2")], [0, 0, 1]],
        b=[_f("1/6"), _f("1/3"), _f("1/3"), _f("1/6")],
        c=[0, _f("1/2"), _f("1/2"), 1]),
}

SAFETY, REJECT_SAFETY, CLIP = 0.9, 0.5, (0.1, 10.0)       # TSADAPTBASIC defaults


def adapt_basic(h, wnorm, order, prev_rejected):
    """TSADAPTBASIC on the weighted error norm of an attempt of size h: (accept, next h)."""
    if not np.isfinite(wnorm):
        return False, h * CLIP[0]
    accept = wnorm <= 1.0
    safety = SAFETY * (REJECT_SAFETY if (not accept and prev_rejected) else 1.0)
    fac = CLIP[1] if wnorm == 0.0 else min(max(safety * wnorm ** (-1.0 / order), CLIP[0]), CLIP[1])
    return accept, h * fac


class _DeviceStages:
    """K_0 .. K_{s-1} and Y on the device, and the two passes of a step"""

    def __init__(self, u, s):
        self.ctx, self.bs = u.ctx, u.bs
        self.K = [Vec(u.ctx, u.bs) for _ in range(s)]
        self.Y = Vec(u.ctx, u.bs)

    def fits(self, u, s):
        return u.ctx is self.ctx and u.bs == self.bs and len(self.K) == s

    def maxpy(self, y, x, vecs, w):
        self.ctx.vec_maxpy(y.id, x.id, [v.id for v in vecs], w)

    def finish(self, x, vecs, hb, hd, atol, rtol):
        return self.ctx.ts_step_finish(x.id, [v.id for v in vecs], hb, hd, atol, rtol)


class TsSolver(object):
    class Type:
        RK = "rk"

    class RKType:
        RK5BS, RK3BS, RK4 = "5bs", "3bs", "4"

    class ExactFinalTime:
        UNSPECIFIED, STEPOVER, INTERPOLATE, MATCHSTEP = 0, 1, 2, 3

    class ConvergedReason:
        CONVERGED_ITERATING, CONVERGED_TIME, CONVERGED_ITS = 0, 1, 2
        DIVERGED_STEP_REJECTED = -2

    def __init__(self, comm=None):
        self.comm = comm
        self.logger = logging.getLogger("TsSolver")
        self.ts_type, self.rk_type = "rk", "5bs"
        self.dt, self.t = 0.1, 0.0
        self.max_time, self.max_steps, self.max_reject = 5.0, 5000, 10
        self.rtol, self.atol = 1e-4, 1e-4
        self.adapt_type = None                  # None: basic when the tableau has an embedded pair
        self.exact_final_time = self.ExactFinalTime.UNSPECIFIED
        self.steps, self.rejects, self.rhs_evals, self.reason = 0, 0, 0, 0
        self._rhs, self._post = None, None
        self._stages = None
        self._restart = False                   # restartStep() since the last stage 0
        self.t_prev = self.t
        self.setType("rk")
        self.setRKType("5bs")
        self.setExactFinalTime(self.ExactFinalTime.MATCHSTEP)
        self.setFromOptions()

    # -- setters
    def setType(self, ts_type):
        if str(ts_type).lower() != "rk":
            raise ValueError(f"TS type '{ts_type}' is not supported: only the explicit 'rk' family is built")
        self.ts_type = "rk"

    def setRKType(self, rk_type):
        rk_type = str(rk_type).lower()
        if rk_type not in TABLEAUX:
            raise ValueError(f"RK type '{rk_type}' is not supported (one of {', '.join(TABLEAUX)})")
        self.rk_type = rk_type

    def setTime(self, t):
        self.t = float(t)

    def setMaxTime(self, max_time):
        self.max_time = float(max_time)

    def setMaxSteps(self, max_steps):
        self.max_steps = int(max_steps)

    def setTimeStep(self, dt):
        self.dt = float(dt)

    def setExactFinalTime(self, option):
        if isinstance(option, str):
            option = {"matchstep": self.ExactFinalTime.MATCHSTEP, "stepover": self.ExactFinalTime.STEPOVER}.get(option.lower(), option)
        if option not in (self.ExactFinalTime.MATCHSTEP, self.ExactFinalTime.STEPOVER):
            raise ValueError(f"exact final time '{option}' is not supported (matchstep or stepover)")
        self.exact_final_time = option

    def setTolerances(self, rtol=None, atol=None):
        if rtol is not None:
            self.rtol = float(rtol)
        if atol is not None:
            self.atol = float(atol)

    def setMaxStepRejections(self, n):
        self.max_reject = int(n)

    def setAdaptType(self, adapt_type):
        if adapt_type not in ("basic", "none"):
            raise ValueError(f"adapt type '{adapt_type}' is not supported (basic or none)")
        self.adapt_type = adapt_type

    def setRHSFunction(self, function, f=None, args=None, kargs=None):
        """function(ts, t, X, F, *args, **kargs) writes the right-hand side at (t, X) into F; `f` is not needed here"""
        self._rhs = (function, tuple(args or ()), dict(kargs or {}))

    def setPostStep(self, function, args=None, kargs=None):
        self._post = (function, tuple(args or ()), dict(kargs or {}))

    # the reference's TsSolver helpers
    def setUpTimes(self, sTime, eTime, steps):
        self.setTime(sTime)
        self.setMaxTime(eTime)
        self.setMaxSteps(steps)

    def initSolver(self, rhsFunction, convergedStepFunction):
        self.setRHSFunction(rhsFunction)
        self.setPostStep(convergedStepFunction)

    def setFromOptions(self):
        opt = Options()
        if opt.hasName("ts_type"):
            self.setType(opt.getString("ts_type"))
        if opt.hasName("ts_rk_type"):
            self.setRKType(opt.getString("ts_rk_type"))
        self.dt = opt.getReal("ts_dt", self.dt)
        self.max_time = opt.getReal("ts_max_time", self.max_time)
        self.max_steps = opt.getInt("ts_max_steps", self.max_steps)
        self.rtol = opt.getReal("ts_rtol", self.rtol)
        self.atol = opt.getReal("ts_atol", self.atol)
        self.max_reject = opt.getInt("ts_max_reject", self.max_reject)
        if opt.hasName("ts_adapt_type"):
            self.setAdaptType(opt.getString("ts_adapt_type"))
        if opt.hasName("ts_exact_final_time"):
            self.setExactFinalTime(opt.getString("ts_exact_final_time"))

    # -- getters
    def getType(self):
        return self.ts_type

    def getRKType(self):
        return self.rk_type

    def getTime(self):
        return self.t

    time = property(getTime, setTime)

    def getPrevTime(self):
        """time before the last accepted step (TSGetPrevTime): getTime() - getPrevTime() is the step a post-step callback just saw"""
        return self.t_prev

    def restartStep(self):
        """the state was changed from outside (TSRestartStep): the next step evaluates stage 0 again, no FSAL stage is reused"""
        self._restart = True

    def getTimeStep(self):
        return self.dt

    time_step = property(getTimeStep, setTimeStep)

    def getMaxTime(self):
        return self.max_time

    def getMaxSteps(self):
        return self.max_steps

    def getStepNumber(self):
        return self.steps

    step_number = property(getStepNumber)

    def getStepRejections(self):
        return self.rejects

    def getConvergedReason(self):
        return self.reason

    def getTolerances(self):
        return self.rtol, self.atol

    def getAdaptType(self):
        """the controller in effect: 'none' for a tableau without an embedded pair"""
        if not TABLEAUX[self.rk_type].embedded:
            return "none"
        return self.adapt_type or "basic"

    # -- integration
    def _stages_for(self, u, s):
        if self._stages is None or not self._stages.fits(u, s):
            self._stages = _DeviceStages(u, s)
        return self._stages

    def solve(self, u):
        """integrate u in place from the current time to max_time (or max_steps steps)"""
        if self._rhs is None:
            raise RuntimeError("TsSolver.solve: setRHSFunction first")
        tab = TABLEAUX[self.rk_type]
        adapt = self.getAdaptType() == "basic"
        match = self.exact_final_time == self.ExactFinalTime.MATCHSTEP
        st = self._stages_for(u, tab.s)
        rhs, rargs, rkw = self._rhs
        K, Y = st.K, st.Y
        self.reason = 0
        have_k0 = False                      # K[0] holds the FSAL stage of the current state
        h = self.dt
        while True:
            if self.steps >= self.max_steps:
                self.reason = self.ConvergedReason.CONVERGED_ITS
                break
            if self.t >= self.max_time:
                self.reason = self.ConvergedReason.CONVERGED_TIME
                break
            if self._restart:
                have_k0, self._restart = False, False
            rejected = 0
            while True:
                hh, last = h, False
                if match and self.t + h >= self.max_time:
                    hh, last = self.max_time - self.t, True
                for i in range(tab.s):
                    if i == 0 and have_k0:
                        continue
                    js = [j for j in range(i) if tab.a_f[i][j] != 0.0]
                    st.maxpy(Y, u, [K[j] for j in js], [hh * tab.a_f[i][j] for j in js])
                    rhs(self, self.t + tab.c_f[i] * hh, Y, K[i], *rargs, **rkw)
                    self.rhs_evals += 1
                have_k0 = tab.fsal
                js = [j for j in range(tab.s) if tab.b_f[j] != 0.0 or (adapt and tab.d_f[j] != 0.0)]
                hb = [hh * tab.b_f[j] for j in js]
                hd = [hh * tab.d_f[j] for j in js] if adapt else None
                wnorm = st.finish(u, [K[j] for j in js], hb, hd, self.atol, self.rtol)
                if not adapt:
                    accept, h_next = True, h
                else:
                    accept, h_next = adapt_basic(hh, wnorm, tab.order, rejected > 0)
                if accept:
                    break
                back = [(K[j], -w) for j, w in zip(js, hb) if w != 0.0]      # roll back
                st.maxpy(u, u, [k for k, _ in back], [w for _, w in back])
                self.rejects += 1
                rejected += 1
                h = h_next
                if rejected > self.max_reject:
                    self.reason = self.ConvergedReason.DIVERGED_STEP_REJECTED
                    self.dt = h
                    self.logger.warning(f"step {self.steps} at t = {self.t:.6e}: {rejected} rejections, giving up (reason -2)")
                    return
            self.t_prev = self.t
            self.t = self.max_time if last else self.t + hh
            self.steps += 1
            h = h_next
            self.dt = h
            if tab.fsal:
                K[0], K[-1] = K[-1], K[0]
            if self._post is not None:
                fn, pargs, pkw = self._post
                fn(self, *pargs, **pkw)
