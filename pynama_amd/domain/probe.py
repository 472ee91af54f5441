"""Point probes: a set of points located once in the domain's mesh on the device (pyn_probe_create) and sampled as often as wanted
(pyn_probe_sample): the finite-element interpolant of a nodal vector at the points.  Belongs to the domain's current device context;
a domain that is indexed again takes its probe sets with it."""
import numpy as np


def line_points(start, end, n):
    """n points from `start` to `end`, both included"""
    start, end = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    if start.shape != end.shape or start.ndim != 1 or int(n) < 2:
        raise ValueError(f"line: from {start.tolist()} to {end.tolist()} with n = {n} is not a segment of at least 2 points")
    t = np.linspace(0.0, 1.0, int(n))[:, None]
    return start[None, :] + t * (end - start)[None, :]


class Probe:
    def __init__(self, dom, points):
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim == 1:
            pts = pts.reshape(-1, dom.dim)
        self.dom, self.points = dom, pts
        self._ctx = dom.ctx
        self._id = self._ctx.probe_create(pts)
        self._located = None

    def __len__(self):
        return int(self.points.shape[0])

    def _live(self):
        if self._id is None or self._ctx is not self.dom._ctx or not self._ctx.h:
            raise RuntimeError("the probe set was destroyed, or the domain was indexed again")
        return self._ctx

    @property
    def info(self):
        """{'n', 'found', 'path' (0 rectilinear lattice, 1 search), 'max_newton', 'max_candidates'}"""
        return self._live().probe_info(self._id)

    def _get(self):
        if self._located is None:
            self._located = self._live().probe_get(self._id)
        return self._located

    @property
    def cells(self):
        """cell of every point, -1 where it lies in no cell"""
        return self._get()[0]

    @property
    def xi(self):
        """reference position of every point in its cell [n, dim], NaN where it lies in no cell"""
        return self._get()[1]

    @property
    def found(self):
        return self.cells >= 0

    def sample(self, vec):
        """the interpolant of `vec` at the points, [n, vec.bs]; NaN rows where a point lies in no cell"""
        return self._live().probe_sample(self._id, vec.id, vec.bs)

    def destroy(self):
        if self._id is not None and self._ctx is self.dom._ctx and self._ctx.h:
            self._ctx.probe_destroy(self._id)
        self._id = None
