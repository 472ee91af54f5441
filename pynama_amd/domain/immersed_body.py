"""Immersed bodies: sets of Lagrangian markers with a weight each (the role of the reference's ``src/domain/immersed_body.py``).

``Body(positions, dl)`` is the generic set -- markers ``X_k`` in R^dim and the arc-length (2-D) or area (3-D) element ``dl_k`` each
one stands for.  ``Circle`` places ``M = round(2 pi r / (spacing h))`` markers on a circle, ``dl = 2 r sin(pi / M)`` (the side of the
inscribed polygon, so ``sum dl`` is its perimeter).  A marker spacing below about ``h`` makes the interpolation / spreading matrix
``A = H S`` ill-conditioned (cond 652 at spacing ``h`` against 7.4 at ``1.5 h`` for the 4-point delta), hence the default 1.5.

A body may carry a prescribed rigid motion ``center(t) = c0 + amp sin(2 pi f t) e_axis``; ``getVelocity(t)`` is its derivative at
every marker.  The discrete delta is chosen with ``setKernel("four" | "three")`` (Peskin's 4-point, the reference's ``fourGrid`` and
the default; Roma's 3-point, ``threeGrid``).  The stencils, the matrix and its factors live on the device (``Context.ibm_set``)."""
import math

import numpy as np

KERNELS = {"four": 0, "three": 1}


class Body(object):
    def __init__(self, positions, dl, kernel="four"):
        self.positions0 = np.array(positions, dtype=float)
        if self.positions0.ndim != 2:
            raise ValueError("Body: positions must be [markers, dim]")
        self.dl = np.broadcast_to(np.asarray(dl, dtype=float), (self.positions0.shape[0],)).copy()
        self.dim = self.positions0.shape[1]
        self.amplitude, self.frequency, self.axis = 0.0, 0.0, 0
        self.setKernel(kernel)

    # -- delta kernel
    def setKernel(self, name):
        if name not in KERNELS:
            raise ValueError(f"delta kernel '{name}' is not supported (one of {', '.join(KERNELS)})")
        self.kernel = name

    def getKernel(self):
        return self.kernel

    def getKernelId(self):
        return KERNELS[self.kernel]

    # -- geometry
    def getTotalNodes(self):
        return self.positions0.shape[0]

    def getElementLength(self):
        return self.dl

    def getLengthScale(self):
        """reference length of the force coefficients: the extent of the markers along the axes, at most"""
        return float((self.positions0.max(axis=0) - self.positions0.min(axis=0)).max())

    # -- prescribed rigid motion
    def setMotion(self, amplitude=0.0, frequency=0.0, axis=0):
        if not 0 <= int(axis) < self.dim:
            raise ValueError(f"motion axis {axis} outside 0..{self.dim - 1}")
        self.amplitude, self.frequency, self.axis = float(amplitude), float(frequency), int(axis)

    def isMoving(self):
        return self.amplitude != 0.0 and self.frequency != 0.0

    def getDisplacement(self, t):
        d = np.zeros(self.dim)
        d[self.axis] = self.amplitude * math.sin(2.0 * math.pi * self.frequency * t)
        return d

    def getPositions(self, t=0.0):
        return self.positions0 + self.getDisplacement(t)[None, :]

    def getVelocity(self, t=0.0):
        """[markers, dim]: d/dt of getPositions (rigid translation: the same for every marker)"""
        v = np.zeros(self.dim)
        w = 2.0 * math.pi * self.frequency
        v[self.axis] = self.amplitude * w * math.cos(w * t)
        return np.tile(v, (self.getTotalNodes(), 1))


class Circle(Body):
    def __init__(self, center, radius, h, spacing=1.5, kernel="four"):
        self.center0 = np.array(center, dtype=float)
        self.radius = float(radius)
        self.spacing = float(spacing)
        if self.center0.size != 2 or not self.radius > 0.0 or not self.spacing > 0.0 or not float(h) > 0.0:
            raise ValueError("Circle: needs a 2-D centre and positive radius, spacing and h")
        M = max(3, int(round(2.0 * math.pi * self.radius / (self.spacing * float(h)))))
        ang = 2.0 * math.pi * np.arange(M) / M
        pos = self.center0[None, :] + self.radius * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        super().__init__(pos, 2.0 * self.radius * math.sin(math.pi / M), kernel)

    def getLengthScale(self):
        return 2.0 * self.radius

    def getCenter(self, t=0.0):
        return self.center0 + self.getDisplacement(t)

    center = property(getCenter)


def body_from_config(block, h):
    """the yaml ``body:`` block -> a body.  ``type: circle`` with ``center``, ``radius``, optional ``spacing`` (marker spacing in
    units of h, default 1.5), ``kernel`` (four | three) and ``motion: {amplitude, frequency, axis}``; ``h`` is the lattice spacing
    the marker spacing refers to (the smallest over the axes)."""
    if not block or "type" not in block:
        raise ValueError("body: block with a 'type' is needed")
    kind = str(block["type"]).lower()
    if kind != "circle":
        raise ValueError(f"body type '{kind}' is not supported (circle)")
    body = Circle(block["center"], block["radius"], h, spacing=block.get("spacing", 1.5), kernel=block.get("kernel", "four"))
    motion = block.get("motion")
    if motion:
        axis = motion.get("axis", 0)
        axis = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
        body.setMotion(motion.get("amplitude", 0.0), motion.get("frequency", 0.0), axis)
    return body
