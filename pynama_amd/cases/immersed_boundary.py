"""Immersed-boundary cases (the reference's ``src/cases/immersed_boundary.py``: ``ImmersedBoundaryStatic`` /
``ImmersedBoundaryDynamic`` with ``buildIBMMatrix`` and ``computeVelocityCorrection``): a uniform stream ``e_x U`` on the external
boundary and a body of Lagrangian markers inside, imposed by the implicit velocity correction of Wu & Shu.

After every accepted time step (``convergedStepFunction``, a fractional step):
  1. ``solveKLE(t, vort)`` gives the velocity of the transported vorticity;
  2. ``computeVelocityCorrection(t)``: ``A q = U_B(t) - H vel`` per component and ``vel += S q`` -- one library call, on the device
     (``pyn_ibm_correct``); afterwards the interpolated velocity at the markers is the body's;
  3. ``vort = Curl vel``, and the integrator is told that its state changed (``TsSolver.restartStep``);
  4. the force on the body over the step ``dt`` is recorded: ``F = -(rho / dt) sum_k dl_k q_k`` -- the force the FLUID exerts on the
     BODY, so a body at rest in the stream ``+e_x`` has ``F_x > 0`` (drag points downstream) -- with the coefficients
     ``C = 2 F / (rho U^2 L)``, ``L`` the body's length scale (the diameter of a circle).
The right-hand-side evaluations inside a step are unchanged: there is no correction inside the stages.

The grid must be a uniform node lattice: box mesh, ngl 2 or 3 (the GLL nodes of ngl 3 are -1, 0, 1), no jitter, one rank; the body's
stencils must stay clear of the outermost node layer.  ``ImmersedBoundaryDynamic`` moves the body (``body: motion:`` in the yaml) and
rebuilds stencils, matrix and factors at the new position before every correction."""
import numpy as np

from pynama_amd.cases.base_problem import FreeSlip
from pynama_amd.domain.immersed_body import body_from_config


class ImmersedBoundaryStatic(FreeSlip):
    def setUp(self):
        if self.comm.size > 1:
            raise NotImplementedError("immersed-boundary cases run on one rank: the marker stencils, the dense force matrix and its "
                                      f"factors are not distributed (this run has {self.comm.size} ranks)")
        if self.dim not in (2, 3):
            raise Exception("Wrong dim")
        self.U_ref = float((self.config.get("free-stream") or {}).get("velocity", 1.0))
        self.cteValue = (self.U_ref * np.eye(self.dim)[0]).tolist()
        super().setUp()
        self.h = [(self.upper[d] - self.lower[d]) / ((self.ngl - 1) * self.nelem[d]) for d in range(self.dim)]
        self.body = self.createBody()
        self.forces, self.lastCorrection = [], None
        self.buildIBMMatrix()

    def createBody(self):
        return body_from_config(self.config.get("body"), min(self.h))

    # -- boundary conditions and initial state: UniformFlow's
    def computeInitialCondition(self, startTime):
        self.vort.set(0.0)

    def applyBoundaryConditions(self, time):
        self.vel.set(0.0)
        self.vel = self.dom.applyValuesToVec(self.bcNodeSet, self.cteValue, self.vel)

    # -- the body on the device
    def buildIBMMatrix(self, time=0.0):
        """stencils, spreading lists, A = H S and its LU factors for the body's position at `time` (pyn_ibm_set)"""
        self.dom.ctx.ibm_set(self.body.getKernelId(), self.body.getPositions(time), self.body.getElementLength(), self.lower, self.h)

    def computeVelocityCorrection(self, time=0.0):
        """vel += S q with A q = U_B(time) - H vel; returns q [markers, dim]"""
        self.lastCorrection = self.dom.ctx.ibm_correct(self.vel.id, self.body.getVelocity(time))
        return self.lastCorrection

    def interpolatedVelocity(self):
        """H vel at the markers, [markers, dim]"""
        return self.dom.ctx.ibm_interp(self.vel.id)

    def convergedStepFunction(self, ts):
        time = ts.getTime()
        dt = time - ts.getPrevTime()
        self.solveKLE(time, self.vort)
        q = self.computeVelocityCorrection(time)
        self.operator.Curl.mult(self.vel, self.vort)
        ts.restartStep()
        self.recordForces(time, dt, q)
        super().convergedStepFunction(ts)

    def recordForces(self, time, dt, q):
        force = -(self.rho / dt) * (self.body.getElementLength()[:, None] * q).sum(axis=0)
        coef = 2.0 * force / (self.rho * self.U_ref ** 2 * self.body.getLengthScale())
        self.forces.append((time, force, coef))

    def getForces(self):
        """[(t, F, C)] per accepted step: force of the fluid on the body and its coefficients (C[0] drag, C[1] lift)"""
        return list(self.forces)


class ImmersedBoundaryDynamic(ImmersedBoundaryStatic):
    def computeVelocityCorrection(self, time=0.0):
        self.buildIBMMatrix(time)
        return super().computeVelocityCorrection(time)
