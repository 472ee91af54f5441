"""Immersed boundary on the device against the dense numpy model of tests/ibm_model.py: interpolation, spreading, the matrix
A = H S, the fused velocity correction, determinism, refusals, and the two case classes end to end."""
import numpy as np
import pytest

import pynama_amd
from pynama_amd._lib import PynamaHipError
from pynama_amd.common.options import Options
from pynama_amd.vectors import Vec
from tests import ibm_model as im

pytestmark = pytest.mark.gpu
pynama_amd.install_reference_layout()
EPS = np.finfo(float).eps
KERNELS = ("four", "three")
KID = {"four": 0, "three": 1}

# name -> (cells, ngl, lower, upper): anisotropic h in 2-D, first order, 13^3 nodes in 3-D, and the circle's grid (h = 1/32)
GRIDS = {
    "2d-ngl3": ([8, 8], 3, [0.0, 0.0], [2.0, 1.0]),
    "2d-ngl2": ([16, 16], 2, [0.0, 0.0], [1.0, 1.0]),
    "3d-ngl3": ([6, 6, 6], 3, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]),
    "circle": ([16, 16], 3, [0.0, 0.0], [1.0, 1.0]),
}


class Grid:
    def __init__(self, name, **kw):
        from pynama_amd.domain.dmplex import DMPlexDom
        nelem, ngl, lower, upper = GRIDS[name]
        self.dom = DMPlexDom(boxMesh={"nelem": nelem, "lower": lower, "upper": upper}, **kw)
        self.dom.setFemIndexing(ngl)
        self.ctx, self.dim = self.dom.ctx, len(nelem)
        self.lower, self.upper = np.array(lower), np.array(upper)
        self.n = (ngl - 1) * np.array(nelem) + 1
        self.h = (self.upper - self.lower) / (self.n - 1)
        self.nodes = int(np.prod(self.n))
        idx = np.stack(np.unravel_index(np.arange(self.nodes), self.n[::-1]), axis=1)[:, ::-1]
        self.xyz = self.lower + idx * self.h                     # node = ix + n_x (iy + n_y iz)

    def markers(self, count, seed, shift_room=0):
        """random markers whose 4-point (and 3-point) support lies in lines 1 .. n - 2: s = (X - lower) / h in [2, n - 4)"""
        rng = np.random.default_rng(seed)
        hi = self.n - 4.0
        hi[0] -= shift_room
        X = self.lower + self.h * rng.uniform(2.0, hi, size=(count, self.dim))
        return X, rng.uniform(0.5, 1.5, count) * self.h.min() ** (self.dim - 1)

    def interp(self, values):
        v = self.vec(values)                                     # the handle lives until the call returns
        return self.ctx.ibm_interp(v.id)

    def vec(self, values=None, bs=None):
        v = Vec(self.ctx, self.dim if bs is None else bs)
        v.set(0.0) if values is None else v.setArray(values)
        return v


@pytest.fixture(scope="module")
def grids():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Grid(name)
        return cache[name]
    return get


# ---- 1. identities and the dense model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["2d-ngl3", "2d-ngl2", "3d-ngl3"])
def test_interp_and_spread_identities(grids, name, kernel):
    g = grids(name)
    ctx, dim = g.ctx, g.dim
    X, dl = g.markers(31, seed=7 + dim)                        # 31: the last lane group / block is partly idle
    ctx.ibm_set(KID[kernel], X, dl, g.lower, g.h)
    info = ctx.ibm_info()
    assert info["markers"] == 31 and info["width"] == (4 if kernel == "four" else 3)
    extent = (g.upper - g.lower).max()
    one = g.interp(np.ones((g.nodes, dim)))
    assert np.abs(one - 1.0).max() <= 1e-13                                              # mass
    xd = g.interp(g.xyz)
    assert np.abs(xd - X).max() <= 1e-13 * extent                                        # first moment: interp of x_d is X_kd
    H, S, _ = im.operators(X, dl, g.lower, g.h, g.n, kernel)
    assert info["affected_nodes"] == int((H != 0).any(axis=0).sum())
    rng = np.random.default_rng(3)
    u, q = rng.standard_normal((g.nodes, dim)), rng.standard_normal((31, dim))
    Hu, Sq = H @ u, S @ q
    got_Hu = g.interp(u)
    assert np.abs(got_Hu - Hu).max() <= 1e-13 * np.abs(Hu).max()
    uv = g.vec()
    ctx.ibm_spread(q, uv.id)
    got_Sq = uv.getArray().reshape(g.nodes, dim)
    assert np.abs(got_Sq - Sq).max() <= 1e-13 * np.abs(Sq).max()
    assert not got_Sq[~(H != 0).any(axis=0)].any()                                       # nothing outside the stencils
    # adjointness and momentum on the DEVICE results.  Bound of each: both sides are numpy sums of N terms t_i whose factors carry
    # the 1e-13 relative error allowed above -> (N eps + 1e-13) sum |t_i| per side
    c = dl / np.prod(g.h)
    lhs, rhs = c[:, None] * q * got_Hu, u * got_Sq
    tol = (lhs.size * EPS + 1e-13) * np.abs(lhs).sum() + (rhs.size * EPS + 1e-13) * np.abs(rhs).sum()
    assert abs(lhs.sum() - rhs.sum()) <= tol                                             # sum_k c_k q_k (H u)_k = sum_j u_j (S q)_j
    for d in range(dim):
        lhs, rhs = np.prod(g.h) * got_Sq[:, d], dl * q[:, d]
        tol = (lhs.size * EPS + 1e-13) * np.abs(lhs).sum() + rhs.size * EPS * np.abs(rhs).sum()
        assert abs(lhs.sum() - rhs.sum()) <= tol                                         # prod h sum_j (S q)_j = sum_k dl_k q_k
    # u += S q adds to what the vector holds
    uv.setArray(u)
    ctx.ibm_spread(q, uv.id)
    assert np.abs(uv.getArray().reshape(g.nodes, dim) - (u + Sq)).max() <= 1e-13 * np.abs(u + Sq).max()


# ---- 2. the matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["2d-ngl3", "2d-ngl2", "3d-ngl3"])
def test_matrix_against_dense_and_translation(grids, name, kernel):
    g = grids(name)
    X, dl = g.markers(26, seed=11 + g.dim, shift_room=1)
    g.ctx.ibm_set(KID[kernel], X, dl, g.lower, g.h)
    A = g.ctx.ibm_matrix()
    ref = im.operators(X, dl, g.lower, g.h, g.n, kernel)[2]
    assert A.shape == (26, 26) and np.abs(A - ref).max() <= 1e-13 * np.abs(ref).max()
    Xs = X.copy()
    Xs[:, 0] += g.h[0]                                           # h is a power of two on every grid here
    g.ctx.ibm_set(KID[kernel], Xs, dl, g.lower, g.h)
    assert np.abs(g.ctx.ibm_matrix() - A).max() <= 1e-12 * np.abs(A).max()


# ---- 3. the fused correction ------------------------------------------------------------------------------------------------------
def _circle(spacing):
    return im.circle((0.5, 0.47), 0.2, 1.0 / 32, spacing)


@pytest.mark.parametrize("kernel, spacing", [("four", 1.5), ("three", 1.5), ("four", 1.0)])
def test_correct_on_the_circle(grids, kernel, spacing):
    g = grids("circle")
    ctx = g.ctx
    X, dl = _circle(spacing)
    M = X.shape[0]
    ctx.ibm_set(KID[kernel], X, dl, g.lower, g.h)
    H, S, A = im.operators(X, dl, g.lower, g.h, g.n, kernel)
    rng = np.random.default_rng(5)
    u0, ub = rng.standard_normal((g.nodes, 2)), rng.standard_normal((M, 2))
    uv = g.vec(u0)
    before = uv.getArray().copy()
    q = ctx.ibm_correct(uv.id, ub)
    r = ub - H @ u0
    norm_A = np.abs(A).sum(axis=1).max()
    back = np.abs(A @ q - r).max()
    print(f"{kernel} spacing {spacing}: M {M}, cond {np.linalg.cond(A):.3g}, backward error {back:.2e}, max|q| {np.abs(q).max():.3g}")
    assert q.shape == (M, 2) and back <= 1e-12 * (norm_A * np.abs(q).max() + np.abs(r).max())
    after = ctx.ibm_interp(uv.id)
    print(f"  max|interp(u) - U_B| {np.abs(after - ub).max():.2e}")
    assert np.abs(after - ub).max() <= 1e-12 * (norm_A * np.abs(q).max() + np.abs(ub).max())
    got = uv.getArray()
    changed = (got.view(np.uint64) != before.view(np.uint64)).reshape(g.nodes, 2).any(axis=1)
    affected = (H != 0).any(axis=0)
    assert changed.any() and not (changed & ~affected).any()          # everything outside the model's stencils is bit-identical
    ref = u0 + S @ q
    assert np.abs(got.reshape(g.nodes, 2) - ref).max() <= 1e-13 * np.abs(ref).max()
    assert int(affected.sum()) <= ctx.ibm_info()["affected_nodes"] <= M * 16


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, kernel", [("circle", "four"), ("3d-ngl3", "three")])
def test_bit_identical_repeats(grids, name, kernel):
    g = grids(name)
    ctx = g.ctx
    X, dl = _circle(1.5) if name == "circle" else g.markers(29, seed=2)
    rng = np.random.default_rng(8)
    u0, ub = rng.standard_normal((g.nodes, g.dim)), rng.standard_normal((X.shape[0], g.dim))
    ctx.ibm_set(KID[kernel], X, dl, g.lower, g.h)
    A1 = ctx.ibm_matrix()
    runs = []
    for _ in range(2):
        uv = g.vec(u0)
        q = ctx.ibm_correct(uv.id, ub)
        runs.append((uv.getArray(), q))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    ctx.ibm_set(KID[kernel], X, dl, g.lower, g.h)
    assert np.array_equal(ctx.ibm_matrix(), A1)
    X2 = X + 0.37 * g.h
    ctx.ibm_set(KID[kernel], X2, dl, g.lower, g.h)
    assert not np.array_equal(ctx.ibm_matrix(), A1)
    ctx.ibm_set(KID[kernel], X, dl, g.lower, g.h)
    assert np.array_equal(ctx.ibm_matrix(), A1)
    uv = g.vec(u0)
    q = ctx.ibm_correct(uv.id, ub)
    assert np.array_equal(uv.getArray(), runs[0][0]) and np.array_equal(q, runs[0][1])
    assert ctx.ibm_info()["builds"] >= 4


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(grids):
    g = Grid("2d-ngl3")
    ctx = g.ctx
    X, dl = g.markers(5, seed=1)
    uv = g.vec(np.ones((g.nodes, 2)))
    for call in (lambda: ctx.ibm_interp(uv.id), lambda: ctx.ibm_spread(np.zeros((5, 2)), uv.id), ctx.ibm_matrix, ctx.ibm_info,
                 ctx.ibm_clear, lambda: ctx.ibm_correct(uv.id, np.zeros((5, 2)))):
        with pytest.raises(PynamaHipError, match="pyn_ibm_set first"):
            call()
    edge = X.copy()
    edge[2, 1] = g.lower[1] + 1.5 * g.h[1]                      # 4-point stencil would start at line 0
    with pytest.raises(PynamaHipError, match="outermost node layer"):
        ctx.ibm_set(0, edge, dl, g.lower, g.h)
    edge[2, 1] = g.upper[1] - 1.4 * g.h[1]                      # 3-point stencil would end at line n - 1
    with pytest.raises(PynamaHipError, match="outermost node layer"):
        ctx.ibm_set(1, edge, dl, g.lower, g.h)
    with pytest.raises(PynamaHipError, match="no markers"):
        ctx.ibm_set(0, np.zeros((0, 2)), np.zeros(0), g.lower, g.h)
    bad = X.copy()
    bad[3, 0] = np.nan
    with pytest.raises(PynamaHipError, match="non-finite"):
        ctx.ibm_set(0, bad, dl, g.lower, g.h)
    with pytest.raises(PynamaHipError, match="not finite"):
        ctx.ibm_set(0, X, np.where(np.arange(5) == 1, np.inf, dl), g.lower, g.h)
    with pytest.raises(PynamaHipError, match="uniform lattice"):
        ctx.ibm_set(0, X, dl, g.lower, g.h * 1.001)             # a spacing that is not the mesh's
    with pytest.raises(PynamaHipError, match="pyn_ibm_set first"):
        ctx.ibm_interp(uv.id)                                   # a refused set leaves no marker set
    ctx.ibm_set(0, X, dl, g.lower, g.h)                         # the context is still good
    assert np.abs(ctx.ibm_interp(uv.id) - 1.0).max() <= 1e-13
    v1, v3 = g.vec(bs=1), g.vec(bs=3)
    with pytest.raises(PynamaHipError, match="block size"):
        ctx.ibm_interp(v1.id)
    with pytest.raises(PynamaHipError, match="block size"):
        ctx.ibm_correct(v3.id, np.zeros((5, 2)))
    ctx.ibm_clear()
    with pytest.raises(PynamaHipError, match="pyn_ibm_set first"):
        ctx.ibm_interp(uv.id)
    # meshes without a uniform lattice
    j = Grid("2d-ngl2", jitter=0.2)
    Xj, dlj = j.markers(5, seed=1)
    with pytest.raises(PynamaHipError, match="uniform lattice"):
        j.ctx.ibm_set(0, Xj, dlj, j.lower, j.h)
    from pynama_amd.domain.dmplex import DMPlexDom
    dom = DMPlexDom(boxMesh={"nelem": [4, 4], "lower": [0.0, 0.0], "upper": [1.0, 1.0]})
    dom.setFemIndexing(4)
    with pytest.raises(PynamaHipError, match="kind 0"):
        dom.ctx.ibm_set(0, np.full((1, 2), 0.5), np.ones(1), np.zeros(2), np.ones(2) / 12)


# ---- 6. / 7. the case classes ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def fixed_step_options():
    saved = Options._db
    Options(argv=["-ts_adapt_type", "none", "-ts_dt", "1e-3", "-ts_rk_type", "3bs"])
    yield
    Options._db = saved


def _config(motion=None):
    body = {"type": "circle", "center": [0.5, 0.5], "radius": 0.15, "spacing": 1.5}
    if motion:
        body["motion"] = motion
    return {"name": "ibm-test", "save-dir": "ibm-test", "material-properties": {"rho": 1.0, "mu": 0.01},
            "free-stream": {"velocity": 1.0}, "body": body,
            "domain": {"ngl": 3, "box-mesh": {"nelem": [16, 16], "lower": [0.0, 0.0], "upper": [1.0, 1.0]}}}


def _solve(fem):
    """a fresh time solver on `fem`, from the initial condition; after every step: state, residual of the no-slip condition, its
    bound, the build count"""
    fem.ts = None
    fem.forces = []
    fem.setUpTimeSolver()
    ctx, log, post = fem.dom.ctx, [], fem.convergedStepFunction

    def step(ts):
        post(ts)
        t = ts.getTime()
        A, q, ub = ctx.ibm_matrix(), fem.lastCorrection, fem.body.getVelocity(t)
        log.append(dict(t=t, vel=fem.vel.getArray(), vort=fem.vort.getArray(), curl=(fem.operator.Curl * fem.vel).getArray(),
                        resid=np.abs(ctx.ibm_interp(fem.vel.id) - ub).max(),
                        bound=1e-12 * (np.abs(A).sum(axis=1).max() * np.abs(q).max() + np.abs(ub).max()),
                        builds=ctx.ibm_info()["builds"], q=q.copy()))
    fem.ts.setPostStep(step)
    builds0 = ctx.ibm_info()["builds"]
    fem.startSolver()
    return fem, log, builds0


def _run_case(cls, steps, motion=None):
    fem = cls(_config(motion), case="ibm-test", maxSteps=steps)
    fem.setUp()
    fem.setUpSolver()
    return _solve(fem)


@pytest.fixture(scope="module")
def static_run():
    from cases.immersed_boundary import ImmersedBoundaryStatic
    saved = Options._db
    Options(argv=["-ts_adapt_type", "none", "-ts_dt", "1e-3", "-ts_rk_type", "3bs"])
    try:
        return _run_case(ImmersedBoundaryStatic, 3)
    finally:
        Options._db = saved


def test_facade_static(static_run):
    fem, log, builds0 = static_run
    assert fem.ts.getStepNumber() == 3 and len(log) == 3 and fem.ts.rhs_evals == 4 * 3
    assert fem.body.getTotalNodes() == int(round(2 * np.pi * 0.15 * 32 / 1.5)) and builds0 == 1
    for rec in log:
        print(f"t {rec['t']:.3e}: max|H vel - U_B| {rec['resid']:.2e} (bound {rec['bound']:.2e})")
        assert rec["resid"] <= rec["bound"]
        assert np.abs(rec["vort"] - rec["curl"]).max() <= 4 * EPS * np.abs(rec["curl"]).max()
        assert rec["builds"] == 1                                   # a static body is built once
    forces = fem.getForces()
    assert len(forces) == 3 and [f[0] for f in forces] == [rec["t"] for rec in log]
    for (t, F, C), rec in zip(forces, log):
        assert np.isfinite(F).all() and np.isfinite(C).all() and F.shape == C.shape == (2,)
        assert F[0] > 0.0                                           # force of the fluid on the body: drag points downstream
        dl = fem.body.getElementLength()
        assert np.allclose(F, -(1.0 / 1e-3) * (dl[:, None] * rec["q"]).sum(axis=0), rtol=1e-9, atol=0)
        assert np.allclose(C, 2 * F / 0.3, rtol=1e-12, atol=0)
    # the external boundary keeps the imposed stream
    vel = log[-1]["vel"].reshape(-1, 2)
    bc = np.array(sorted(fem.bcNodes), dtype=np.int64)
    assert np.abs(vel[bc] - [1.0, 0.0]).max() <= 1e-12


def test_facade_dynamic(fixed_step_options):
    from cases.immersed_boundary import ImmersedBoundaryDynamic
    motion = {"amplitude": 0.05, "frequency": 2.0, "axis": "y"}
    fem, log, builds0 = _run_case(ImmersedBoundaryDynamic, 2, motion)
    assert builds0 == 1 and [rec["builds"] for rec in log] == [2, 3] and fem.ts.rhs_evals == 8
    ctx = fem.dom.ctx
    for rec in log:
        ub = fem.body.getVelocity(rec["t"])
        assert ub[0, 1] == pytest.approx(0.05 * 4 * np.pi * np.cos(4 * np.pi * rec["t"])) and rec["resid"] <= rec["bound"]
    # the device holds the stencils of the LAST position: interp there gives the body's velocity there
    H = im.weights(fem.body.getPositions(log[-1]["t"]), np.zeros(2), np.ones(2) / 32, np.array([33, 33]), "four")
    got = H @ log[-1]["vel"].reshape(-1, 2)
    vel = log[-1]["vel"].reshape(-1, 2)
    assert np.abs(got - fem.body.getVelocity(log[-1]["t"])).max() <= log[-1]["bound"] + 1e-13 * (np.abs(H) @ np.abs(vel)).max()
    assert not np.array_equal(fem.body.getPositions(log[-1]["t"]), fem.body.getPositions(0.0))
    # zero amplitude: the static run, bit for bit.  Both runs share ONE problem (the same K, operators and factors): two problems
    # assembled apart already differ in the last bits of K (2.3e-13 absolute on entries of 1e3 between two set-ups of this very case),
    # so their velocities differ at 1e-14 whatever the body does.  The static run takes ImmersedBoundaryStatic's correction on that
    # problem, the dynamic run the class's own (pyn_ibm_set at the unchanged position before every correction).
    import types
    from cases.immersed_boundary import ImmersedBoundaryStatic
    still = ImmersedBoundaryDynamic(_config({"amplitude": 0.0, "frequency": 2.0, "axis": "y"}), case="ibm-test", maxSteps=2)
    still.setUp()
    still.setUpSolver()
    still.computeVelocityCorrection = types.MethodType(ImmersedBoundaryStatic.computeVelocityCorrection, still)
    _, ref, b0 = _solve(still)
    assert [rec["builds"] for rec in ref] == [b0, b0] and still.ts.rhs_evals == 8
    del still.computeVelocityCorrection
    _, slog, b1 = _solve(still)
    assert b1 == b0 and [rec["builds"] for rec in slog] == [b0 + 1, b0 + 2] and len(slog) == len(ref) == 2
    for a, b in zip(slog, ref):
        assert a["t"] == b["t"] and np.abs(a["q"]).max() > 0.0
        assert np.array_equal(a["vel"], b["vel"]) and np.array_equal(a["vort"], b["vort"]) and np.array_equal(a["q"], b["q"])
    assert [f[0] for f in still.getForces()] == [rec["t"] for rec in slog]
