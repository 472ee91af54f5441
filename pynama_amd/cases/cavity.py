"""Lid-driven cavity (mirrors ``src/cases/cavity.py:5-82``): no-slip walls from the ``boundary-conditions``
block of the YAML (moving walls carry a tangential velocity), optional free-slip (Dirichlet) faces."""
import numpy as np

from pynama_amd.cases.base_problem import NoSlipFreeSlip
from pynama_amd.common.nswalls import NoSlipWalls


class Cavity(NoSlipFreeSlip):
    def setUp(self):
        super().setUp()
        self.collectCornerNodes()
        # one node set per wall, built once: applyBoundaryConditions / applyBoundaryConditionsFS rebuild no index array
        self.wallNodeSets = {wall: self.dom.nodeSet(self.dom.getBorderNodes(wall)) for wall in self.nsWalls.getWallsNames()}

    def collectCornerNodes(self):
        cornerNodes = set()
        allWalls = list(self.nsWalls.getWallsNames())
        while len(allWalls) > 0:
            currentNodes = set(self.dom.getBorderNodes(allWalls.pop(0)))
            for wall in allWalls:
                cornerNodes |= currentNodes & set(self.dom.getBorderNodes(wall))
        self.cornerDofs = [self.dim * node + dof for node in sorted(cornerNodes) for dof in range(self.dim)]

    def readBoundaryCondition(self, inputData):
        try:
            self.nsWalls = NoSlipWalls(self.lower, self.upper, exclude=inputData['free-slip'].keys())
        except Exception:
            self.nsWalls = NoSlipWalls(self.lower, self.upper)
        if 'no-slip' in inputData:
            for wallName, wallVelocity in inputData['no-slip'].items():
                self.nsWalls.setWallVelocity(wallName, wallVelocity)

    def setUpBoundaryConditions(self):
        self.dom.setLabelToBorders()
        bc = self.config.get("boundary-conditions")
        fsFaces = list(bc['free-slip'].keys()) if 'free-slip' in bc else list()
        nsFaces = list(self.nsWalls.getWallsNames())
        self.dom.setBoundaryCondition(fsFaces, nsFaces)
        self._nsFaces, self._dirFaces = nsFaces, fsFaces

    def computeInitialCondition(self, startTime):
        self.vort.set(0.0)

    def _setWallValues(self, vec, walls, static):
        for wallName in walls:
            if static:
                velDofs = self.nsWalls.getStaticDofsByName(wallName)
                vel = np.zeros(len(velDofs))
            else:
                vel, velDofs = self.nsWalls.getWallVelocity(wallName)
            if len(velDofs) == 0:
                continue
            values, flags = np.zeros(self.dim), np.zeros(self.dim, dtype=np.uint8)
            values[velDofs], flags[velDofs] = np.asarray(vel, dtype=float), 1
            self.dom.ctx.vec_set_nodes(vec.id, self.wallNodeSets[wallName].id, values, flags)

    def applyBoundaryConditions(self, time=None):
        self.vel.set(0.0)
        self._setWallValues(self.vel, self.nsWalls.getWallsWithVelocity(), static=False)

    def applyBoundaryConditionsFS(self):
        self._setWallValues(self.velFS, self.nsWalls.getWallsWithVelocity(), static=False)
        self._setWallValues(self.velFS, self.nsWalls.getStaticWalls(), static=True)

    def centerlines(self, n=65):
        """the velocity profiles of the two centre lines (the Ghia comparison): (y, u(xc, y)) and (x, v(x, yc)) at n points each,
        from two probe sets built on first use"""
        xc, yc = (0.5 * (lo + up) for lo, up in zip(self.lower[:2], self.upper[:2]))
        if self.dim != 2:
            raise ValueError("centerlines: the cavity's centre lines are those of a 2-D case")
        cached = getattr(self, "_centerProbes", None)
        if cached is None or cached[0] != int(n):
            for probe in (cached[3:] if cached else ()):
                probe.destroy()
            y = np.linspace(self.lower[1], self.upper[1], int(n))
            x = np.linspace(self.lower[0], self.upper[0], int(n))
            cached = (int(n), y, x, self.dom.createProbe(np.column_stack([np.full(int(n), xc), y])),
                      self.dom.createProbe(np.column_stack([x, np.full(int(n), yc)])))
            self._centerProbes = cached
        _, y, x, vertical, horizontal = cached
        return (y, vertical.sample(self.vel)[:, 0]), (x, horizontal.sample(self.vel)[:, 1])
