"""Analytic-field cases (API of src/cases/custom_func.py:14-83; Taylor-Green fields :173-193, 196-272; the sinusoidal
field of the operator study :276-310): boundary velocity and interior vorticity come from closed-form functions, and
`OperatorsTests` (:132-153) measures the Curl / convective / diffusive operator chains against their exact fields."""
from math import cos, exp, pi, sin, sqrt

from pynama_amd.cases.base_problem import FreeSlip


class CustomFuncCase(FreeSlip):
    def setUp(self):
        self.setUpGeneral()
        self.setUpBoundaryConditions()
        self.setUpEmptyMats()
        self.buildKLEMats()
        self.buildOperators()
        self.nu = self.mu / self.rho
        # the fields as objects: callable like the static methods below (the same functions), and evaluable on the device
        from pynama_amd.cases import fields
        if self.case == 'taylor-green':
            if self.dim == 2:
                self.velFunction = fields.taylorGreenVel_2D
                self.vortFunction = fields.taylorGreenVort_2D
            else:
                self.velFunction = fields.taylorGreenVel_3D
                self.vortFunction = fields.taylorGreenVort_3D
                self.diffusiveFunction = fields.taylorGreen3dDiffusive
                self.convectiveFunction = fields.taylorGreen3dConvective
        elif self.case == 'senoidal':
            if self.dim != 2:
                raise Exception("not defined func")
            self.velFunction = fields.senoidalVel_2D
            self.vortFunction = fields.senoidalVort_2D
            self.diffusiveFunction = fields.senoidalDiffusive
            self.convectiveFunction = fields.senoidalConvective
        else:
            raise Exception("Case not found")

    def _at(self, function, time):
        """function(., nu, t=time) for the apply*ToVec helpers: a field object binds (they may then evaluate it on the device,
        -pynama_device_fields), any other callable is wrapped as before"""
        if hasattr(function, "bind"):
            return function.bind(self.nu, time)
        return lambda coords: function(coords, self.nu, t=time)

    def computeInitialCondition(self, startTime):
        self.vort = self.dom.applyFunctionVecToVec(self.allNodeSet, self._at(self.vortFunction, startTime), self.vort, self.dim_w)

    def generateExactVecs(self, time):
        exactVel = self.mat.K.createVecRight()
        exactVort = self.mat.Rw.createVecRight()
        exactVel = self.dom.applyFunctionVecToVec(self.allNodeSet, self._at(self.velFunction, time), exactVel, self.dim)
        exactVort = self.dom.applyFunctionVecToVec(self.allNodeSet, self._at(self.vortFunction, time), exactVort, self.dim_w)
        return exactVel, exactVort

    def applyBoundaryConditions(self, time):
        self.vel.set(0.0)
        self.vel = self.dom.applyFunctionVecToVec(self.bcNodeSet, self._at(self.velFunction, time), self.vel, self.dim)
        self.vort = self.dom.applyFunctionVecToVec(self.bcNodeSet, self._at(self.vortFunction, time), self.vort, self.dim_w)

    @staticmethod
    def taylorGreenVel_2D(coord, nu, t=None):
        Lx = Ly = 1
        x_, y_ = 2 * pi * coord[0] / Lx, 2 * pi * coord[1] / Ly
        decay = exp(-4 * (pi ** 2) * nu * t * (1.0 / Lx ** 2 + 1.0 / Ly ** 2))
        return [cos(x_) * sin(y_) * decay, -sin(x_) * cos(y_) * decay]

    @staticmethod
    def taylorGreenVort_2D(coord, nu, t=None):
        Lx = Ly = 1
        x_, y_ = 2 * pi * coord[0] / Lx, 2 * pi * coord[1] / Ly
        decay = exp(-4 * (pi ** 2) * nu * t * (1.0 / Lx ** 2 + 1.0 / Ly ** 2))
        return [-2 * pi * (1.0 / Lx + 1.0 / Ly) * cos(x_) * cos(y_) * decay]

    # ---- operator known-answer study (custom_func.py:110-170; `run_case.py -test operators`) ----------------------------
    def _fieldVec(self, like, function, time, dof, name):
        vec = like.duplicate()
        vec.setName(f"{self.caseName}-exact-{name}")
        return self.dom.applyFunctionVecToVec(self.allNodeSet, self._at(function, time), vec, dof)

    def generateExactOperVecs(self, time):
        vel0, vort0 = self.mat.K.createVecRight(), self.mat.Rw.createVecRight()
        return (self._fieldVec(vel0, self.velFunction, time, self.dim, "vel"),
                self._fieldVec(vort0, self.vortFunction, time, self.dim_w, "vort"),
                self._fieldVec(vort0, self.convectiveFunction, time, self.dim_w, "convective"),
                self._fieldVec(vort0, self.diffusiveFunction, time, self.dim_w, "diffusive"))

    def getConvective(self, exactVel, exactConv):
        """Curl( Div( v (x) v ) ) of the field held in self.vel (custom_func.py:155-161)."""
        self.computeVtensV()
        flux = self.vel.duplicate()
        self.operator.DivSrT.mult(self._VtensV, flux)
        out = exactConv.duplicate()
        self.operator.Curl.mult(flux, out)
        return out

    def getDiffusive(self, exactVel, exactDiff):
        """Curl( Div( 2 mu S(v) ) / rho ) of exactVel (custom_func.py:163-171)."""
        self.operator.SrT.mult(exactVel, self._Aux1)
        self._Aux1 *= (2.0 * self.mu)
        flux = self.vel.duplicate()
        self.operator.DivSrT.mult(self._Aux1, flux)
        flux.scale(1 / self.rho)
        out = exactDiff.duplicate()
        self.operator.Curl.mult(flux, out)
        return out

    def OperatorsTests(self, viscousTime=1):
        """Lumped-mass L2 errors of the convective, diffusive and Curl chains against the exact fields at
        t = tau^2 / (4 nu) (custom_func.py:132-153).  The velocity is the KLE solution with the exact vorticity and the
        exact boundary velocity, as in the reference; nothing is written to disk."""
        time = (viscousTime ** 2) / (4 * self.nu)
        self.applyBoundaryConditions(time)
        exactVel, exactVort, exactConv, exactDiff = self.generateExactOperVecs(time)
        self.solver(self.mat.Rw * exactVort + self.mat.Krhs * self.vel, self.vel)
        convective = self.getConvective(exactVel, exactConv)
        diffusive = self.getDiffusive(exactVel, exactDiff)
        self.operator.Curl.mult(exactVel, self.vort)
        wei = self.operator.lumpedWeights(self.dim_w)
        l2 = lambda a, b: sqrt(((a - b) * (a - b)).dot(wei))
        return l2(convective, exactConv), l2(diffusive, exactDiff), l2(self.vort, exactVort)

    # ---- fields -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _tg3(coord, nu, t):
        """phases and decay of the unit-box 3-D Taylor-Green vortex (custom_func.py:196-272 with Lx = Ly = Lz = Uref = 1)"""
        k = 2 * pi
        return k * coord[0], k * coord[1], k * coord[2], exp(-12 * (pi ** 2) * nu * t)

    @staticmethod
    def taylorGreenVel_3D(coord, nu, t=None):
        x, y, z, e = CustomFuncCase._tg3(coord, nu, t)
        return [cos(x) * sin(y) * sin(z) * e, sin(x) * cos(y) * sin(z) * e, -2 * sin(x) * sin(y) * cos(z) * e]

    @staticmethod
    def taylorGreenVort_3D(coord, nu, t=None):
        x, y, z, e = CustomFuncCase._tg3(coord, nu, t)
        k = 2 * pi * e
        return [-3 * k * sin(x) * cos(y) * cos(z), 3 * k * cos(x) * sin(y) * cos(z), 0.0]

    @staticmethod
    def taylorGreen3dConvective(coord, nu, t=None):
        x, y, z, e = CustomFuncCase._tg3(coord, nu, t)
        a = 6 * (2 * pi * e) ** 2
        return [-a * sin(y) * cos(y) * sin(z) * cos(z), a * sin(x) * cos(x) * sin(z) * cos(z), 0.0]

    @staticmethod
    def taylorGreen3dDiffusive(coord, nu, t=None):
        x, y, z, e = CustomFuncCase._tg3(coord, nu, t)
        a = 9 * nu * e * (2 * pi) ** 3
        return [a * sin(x) * cos(y) * cos(z), -a * cos(x) * sin(y) * cos(z), 0.0]

    @staticmethod
    def senoidalVel_2D(coord, nu, t=None):
        return [sin(2 * pi * coord[1]), sin(4 * pi * coord[0])]

    @staticmethod
    def senoidalVort_2D(coord, nu, t=None):
        return [4 * pi * cos(4 * pi * coord[0]) - 2 * pi * cos(2 * pi * coord[1])]

    @staticmethod
    def senoidalConvective(coord, nu, t=None):
        """(v . grad) w of the field above"""
        return [((2 * pi) ** 2 - (4 * pi) ** 2) * sin(2 * pi * coord[1]) * sin(4 * pi * coord[0])]

    @staticmethod
    def senoidalDiffusive(coord, nu, t=None):
        """nu lap(w).  (The reference's senoidalDiffusive, custom_func.py:301-308, leaves the factor nu out while its
        getDiffusive applies 2 mu / rho: its study compares fields that differ by nu.  The chain is what is pinned here.)"""
        return [nu * ((2 * pi) ** 3 * cos(2 * pi * coord[1]) - (4 * pi) ** 3 * cos(4 * pi * coord[0]))]
