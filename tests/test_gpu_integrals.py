"""GPU tests of the mesh integrals (pynama_amd/csrc/pyn_integrals.hip) against the numpy model of tests/integrals_model.py.

Bars.
  parity      |dev - model| <= 2e-13 S for every entry, S = the sum of the absolute contributions of that entry over all cells and
              points: the project's oracle-parity bar, independent of cancellation in `value`.  The order of summation moves a moment
              by about 2e-15 S (tests/test_integrals_model_host.py), the sum-factorised interpolation adds O(ngl eps).
              Measured on an MI355X: at most 0.034 of the bar (3-D ngl 8), 0.002 to 0.014 elsewhere.
  diagnostics the same bar for every entry of a record; div_l2 and curl_l2 of the smooth solenoidal Taylor-Green field take the
              scale of the absolute gradient components (im.component_scale): div u is a sum of cancelling gradient components,
              each rounded relative to itself, and against |contribution| alone the difference, the model's rounding included,
              was 1.95 bars.
  exact       uniform boxes of cell size 2^-3, ngl 2, nodal rule, integer nodal values: every weight det J is a power of two, so
              volume, value and square equal the integer-arithmetic result bit for bit.
  closed      1e-13 relative for volumes and constants, 1e-12 for the polynomial of the element's own degree."""
import math
import os

import numpy as np
import pytest
import yaml

from oracle import fem_oracle as fo
from tests import ho_general_meshes as gm
from tests import integrals_model as im
from tests.test_gpu_ho3 import make_ctx

pytestmark = pytest.mark.gpu

BAR = 2e-13
CASES_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pynama_amd", "cases")


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


MESHES = {
    "warped2d_5x3_ngl2": lambda: gm.warped_lattice(2, [5, 3], 2),
    "warped2d_5x3_ngl3": lambda: gm.warped_lattice(2, [5, 3], 3),
    "warped2d_5x3_ngl4": lambda: gm.warped_lattice(2, [5, 3], 4),
    "warped2d_5x3_ngl6": lambda: gm.warped_lattice(2, [5, 3], 6),
    "warped2d_2x1_ngl12": lambda: gm.warped_lattice(2, [2, 1], 12),
    "warped3d_3x2x2_ngl2": lambda: gm.warped_lattice(3, [3, 2, 2], 2),
    "warped3d_2x2x3_ngl3": lambda: gm.warped_lattice(3, [2, 2, 3], 3),
    "warped3d_2x1x2_ngl5": lambda: gm.warped_lattice(3, [2, 1, 2], 5),
    "warped3d_1x1x2_ngl8": lambda: gm.warped_lattice(3, [1, 1, 2], 8),
    "imported2d_4x3_ngl3": lambda: gm.imported(2, [4, 3], 3),
    "imported2d_4x3_ngl5": lambda: gm.imported(2, [4, 3], 5),
    "imported3d_2x2x2_ngl3": lambda: gm.imported(3, [2, 2, 2], 3),
    "imported3d_2x2x2_ngl4": lambda: gm.imported(3, [2, 2, 2], 4),
    "star3_ngl4": lambda: gm.star(3, 4),
    "star5_ngl3": lambda: gm.star(5, 3),
    "star5_ngl3_layers2": lambda: gm.star(5, 3, layers=2),
    "onecell2d_ngl3": lambda: gm.warped_lattice(2, [1, 1], 3),
    "onecell3d_ngl3": lambda: gm.warped_lattice(3, [1, 1, 1], 3),
}
TAILS = {
    "warped2d_37x29_ngl2": lambda: gm.warped_lattice(2, [37, 29], 2),
    "warped3d_7x5x3_ngl2": lambda: gm.warped_lattice(3, [7, 5, 3], 2),
    "warped2d_257x257_ngl2": lambda: gm.warped_lattice(2, [257, 257], 2),     # more partials than the summing workgroup has lanes
}
_MESH = {}


def mesh_of(name):
    if name not in _MESH:
        _MESH[name] = (MESHES.get(name) or TAILS[name])()
    return _MESH[name]


def set_vec(ctx, u):
    u = np.asarray(u, dtype=np.float64)
    v = ctx.vec_create(1 if u.ndim == 1 else u.shape[1])
    ctx.vec_set(v, u.ravel())
    return v


def check_parity(lib, ctx, mesh, bs, seed, combos=None):
    rng = np.random.default_rng(seed)
    ua, ub = rng.uniform(-1.0, 1.0, (mesh.n_node, bs)), rng.uniform(-1.0, 1.0, (mesh.n_node, bs))
    va, vb = set_vec(ctx, ua), set_vec(ctx, ub)
    worst = 0.0
    for rule, grad, minus in combos or [(r, g, m) for r in (im.NODAL, im.GAUSS) for g in (False, True) for m in (False, True)]:
        dev = ctx.integrate(va, vb if minus else None, rule, grad)
        ref, S = im.moments(mesh, ua, rule, grad, ub if minus else None)
        assert len(dev) == len(ref) == lib.integrate_len(mesh.dim, bs, grad) == im.n_entries(mesh.dim, bs, grad)
        ratio = np.abs(dev - ref) / (BAR * S)
        worst = max(worst, ratio.max())
        assert ratio.max() <= 1.0, (rule, grad, minus, bs, ratio)
    ctx.vec_destroy(va)
    ctx.vec_destroy(vb)
    return worst


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_parity_with_the_model(lib, name):
    mesh = mesh_of(name)
    dim = mesh.dim
    ctx = make_ctx(lib, mesh, ngl=mesh.ngl)
    worst = max(check_parity(lib, ctx, mesh, bs, seed) for seed, bs in enumerate((1, dim, 3 if dim == 2 else 6, 6)))
    print(f"{name}: worst |dev - model| / (2e-13 S) = {worst:.3f}")
    ctx.close()


@pytest.mark.parametrize("name", sorted(TAILS))
def test_second_pass_tails(lib, name):
    mesh = mesh_of(name)
    ctx = lib.Context(0)
    ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
    worst = check_parity(lib, ctx, mesh, mesh.dim, 11, combos=[(im.NODAL, True, False), (im.GAUSS, True, True)])
    print(f"{name}: worst |dev - model| / (2e-13 S) = {worst:.3f}")
    ctx.close()


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nelem", [(37, 29), (7, 5, 3), (257, 257)])
def test_exact_arithmetic(lib, nelem):
    dim = len(nelem)
    mesh = fo.box_mesh(list(nelem), [0.0] * dim, [n / 8.0 for n in nelem], 2)
    assert np.array_equal(mesh.xyz * 8.0, np.round(mesh.xyz * 8.0))
    ctx = lib.Context(0)
    ctx.mesh_set(dim, mesh.conn, mesh.xyz)
    rng = np.random.default_rng(4)
    for bs in (1, dim):
        ua, ub = rng.integers(-8, 9, (mesh.n_node, bs)), rng.integers(-4, 5, (mesh.n_node, bs))
        va, vb = set_vec(ctx, ua), set_vec(ctx, ub)
        for minus in (False, True):
            u = ua - ub if minus else ua
            ue = u[mesh.conn].astype(np.int64)                       # [E, nn, bs]
            w = 2.0 ** (-4 * dim)                                    # weight 1 per axis, det J = (2^-4)^dim
            ref = np.concatenate([[mesh.n_elem * 2 ** dim * w], ue.sum(axis=(0, 1)) * w, (ue * ue).sum(axis=(0, 1)) * w])
            dev = ctx.integrate(va, vb if minus else None, im.NODAL, False)
            assert np.array_equal(dev, ref), (bs, minus, dev, ref)
    ctx.close()


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("name", ["warped2d_5x3_ngl2", "warped2d_5x3_ngl4", "warped2d_2x1_ngl12", "onecell2d_ngl3", "warped2d_37x29_ngl2"])
def test_shoelace_area(lib, name):
    mesh = mesh_of(name)
    ctx = make_ctx(lib, mesh, ngl=mesh.ngl)
    v = set_vec(ctx, np.zeros(mesh.n_node))
    for rule in (im.NODAL, im.GAUSS):
        assert _rel(ctx.integrate(v, None, rule, False)[0], im.shoelace_area(mesh)) <= 1e-13
    ctx.close()


@pytest.mark.parametrize("nelem,ngl", [((5, 3), 3), ((3, 2), 6), ((3, 2, 2), 2), ((2, 2, 3), 4)])
def test_constants_and_rotation_on_a_bent_lattice(lib, nelem, ngl):
    dim = len(nelem)
    mesh = gm.bent_lattice(dim, list(nelem), ngl, seed=2)
    box, c = math.prod(gm.UPPER[:dim]), -1.75
    ctx = make_ctx(lib, mesh, ngl=ngl)
    vc = set_vec(ctx, np.full((mesh.n_node, dim), c))
    rot = np.zeros((mesh.n_node, dim))
    rot[:, 0], rot[:, 1] = -mesh.xyz[:, 1], mesh.xyz[:, 0]           # u = (-y, x[, 0]): div u = 0, curl u = 2 e_z
    vr = set_vec(ctx, rot)
    for rule in (im.NODAL, im.GAUSS):
        m = im.named(ctx.integrate(vc, None, rule, True), dim, dim, True)
        assert _rel(m["volume"], box) <= 1e-13
        assert np.abs(m["square"] / (c * c * box) - 1.0).max() <= 1e-13 and np.abs(m["value"] / (c * box) - 1.0).max() <= 1e-13
        assert max(np.abs(m["grad2"]).max(), abs(m["div2"]), np.abs(m["curl2"]).max()) <= 1e-12 * c * c * box
    m = im.named(ctx.integrate(vr, None, im.GAUSS, True), dim, dim, True)
    assert abs(m["div2"]) <= 1e-12 * box
    assert _rel(m["curl2"][-1], 4.0 * box) <= 1e-12 and np.abs(m["curl2"][:-1]).max(initial=0.0) <= 1e-12 * box
    ctx.close()


@pytest.mark.parametrize("nelem,ngl", [((5, 3), 2), ((5, 3), 3), ((3, 2), 6), ((2, 1), 12), ((3, 2, 2), 2), ((2, 2, 3), 3), ((2, 1, 2), 5),
                                       ((1, 1, 2), 8)])
def test_polynomial_on_a_sheared_box(lib, nelem, ngl):
    dim, s = len(nelem), 0.3
    box = fo.box_mesh(list(nelem), [0.0] * dim, gm.UPPER[:dim], ngl)
    mesh = im.sheared(box, s)
    ctx = lib.Context(0)
    ctx.mesh_set(dim, mesh.conn, mesh.xyz)
    m = im.named(ctx.integrate(set_vec(ctx, im.poly_nodal(box)), None, im.GAUSS, True), dim, 1, True)
    sq, g2 = im.poly_closed_form(ngl, gm.UPPER[:dim], s)
    assert _rel(m["volume"], math.prod(gm.UPPER[:dim])) <= 1e-13
    assert _rel(m["square"][0], sq) <= 1e-12 and _rel(m["grad2"][0], g2) <= 1e-12
    ctx.close()


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_determinism_and_grid_independence(lib):
    saved = os.environ.pop("PYNAMA_INTEGRATE_MAX_GRID", None)
    try:
        for name in ("warped2d_37x29_ngl2", "warped3d_2x1x2_ngl5", "warped2d_257x257_ngl2"):
            mesh = mesh_of(name)
            ctx = lib.Context(0)
            ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
            rng = np.random.default_rng(8)
            va, vb = (set_vec(ctx, rng.uniform(-1.0, 1.0, (mesh.n_node, mesh.dim))) for _ in range(2))
            for rule in (im.NODAL, im.GAUSS):
                first = ctx.integrate(va, vb, rule, True)
                for _ in range(19):
                    assert ctx.integrate(va, vb, rule, True).tobytes() == first.tobytes()
                for cap in ("1", "3"):
                    os.environ["PYNAMA_INTEGRATE_MAX_GRID"] = cap
                    assert ctx.integrate(va, vb, rule, True).tobytes() == first.tobytes(), (name, rule, cap)
                del os.environ["PYNAMA_INTEGRATE_MAX_GRID"]
                same = ctx.integrate(va, va, rule, True)
                assert same[0] == first[0] and np.all(same[1:] == 0.0)
            ctx.close()
    finally:
        if saved is not None:
            os.environ["PYNAMA_INTEGRATE_MAX_GRID"] = saved


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    ctx = lib.Context(0)
    tri = fo.simplex_box_mesh([2, 2], [0.0, 0.0], [1.0, 1.0])
    ctx.mesh_set(2, tri.conn, tri.xyz)
    v = ctx.vec_create(1)
    with pytest.raises(lib.PynamaHipError, match="simplices"):
        ctx.integrate(v)
    ctx.close()
    big = fo.box_mesh([1, 1], [0.0, 0.0], [1.0, 1.0], 13)
    ctx = lib.Context(0)
    ctx.mesh_set(2, big.conn, big.xyz)
    with pytest.raises(lib.PynamaHipError, match="ngl 13 is above the limit.*ngl <= 12"):
        ctx.integrate(ctx.vec_create(1))
    ctx.close()
    quad = fo.box_mesh([3, 2], [0.0, 0.0], [1.0, 1.0], 3)
    small = fo.box_mesh([2, 2], [0.0, 0.0], [1.0, 1.0], 3)
    ctx = lib.Context(0)
    ctx.mesh_set(2, small.conn, small.xyz)
    old = ctx.vec_create(1)                                          # a vector of the mesh before this one
    ctx.mesh_set(2, quad.conn, quad.xyz)
    v1, v2 = ctx.vec_create(1), ctx.vec_create(2)
    with pytest.raises(lib.PynamaHipError, match="the vector holds 25 nodes, the mesh has 35"):
        ctx.integrate(old)
    with pytest.raises(lib.PynamaHipError, match="vec_b holds 25 nodes, the mesh has 35"):
        ctx.integrate(v1, old)
    with pytest.raises(lib.PynamaHipError, match="vec_b has block size 2, vec_a has 1"):
        ctx.integrate(v1, v2)
    with pytest.raises(lib.PynamaHipError, match="unknown rule 7"):
        ctx.integrate(v1, None, 7)
    # a cell with two corners swapped: det J < 0, the message names the cell; the context goes on working
    bad = quad.conn.copy()
    bad[4, [0, 1]] = bad[4, [1, 0]]
    ctx.mesh_set(2, bad, quad.xyz)
    v = set_vec(ctx, np.ones(quad.n_node))
    for rule in (im.NODAL, im.GAUSS):
        with pytest.raises(lib.PynamaHipError, match="cell 4 has det J <= 0"):
            ctx.integrate(v, None, rule)
    # the next mesh: the call works on it
    ctx.mesh_set(2, quad.conn, quad.xyz)
    v = set_vec(ctx, np.ones(quad.n_node))
    assert _rel(ctx.integrate(v)[1], 1.0) <= 1e-13
    # a NaN node: NaN value and square, the volume stays
    u = np.ones(quad.n_node)
    u[7] = np.nan
    vn = set_vec(ctx, u)
    for rule in (im.NODAL, im.GAUSS):
        out = ctx.integrate(vn, None, rule, True)
        assert _rel(out[0], 1.0) <= 1e-13 and np.isnan(out[1:]).all()
    other = gm.warped_lattice(3, [2, 1, 2], 3)
    ctx.mesh_set(3, other.conn, other.xyz)
    check_parity(lib, ctx, other, 3, 5, combos=[(im.GAUSS, True, True)])
    ctx.close()


# ---- facade ----------------------------------------------------------------------------------------------------------------------
def _dom_mesh(dom, ngl):
    return fo.BoxMesh(dom.dim, ngl, (), (), np.ascontiguousarray(dom.conn, dtype=np.int32), np.asarray(dom.xyz, dtype=np.float64),
                      np.zeros(0, np.int64), {})


@pytest.mark.parametrize("jitter,ngl", [(0.0, 3), (0.2, 2)])        # (a domain bends its own box only at ngl 2)
def test_domain_methods(lib, jitter, ngl):
    from pynama_amd.domain.dmplex import DMPlexDom
    dom = DMPlexDom(boxMesh={'nelem': [4, 3], 'lower': [0.0, 0.0], 'upper': [1.0, 0.8]}, jitter=jitter)
    dom.setFemIndexing(ngl)
    mesh = _dom_mesh(dom, ngl)
    rng = np.random.default_rng(2)
    ua, ub = rng.uniform(-1.0, 1.0, (mesh.n_node, 2)), rng.uniform(-1.0, 1.0, (mesh.n_node, 2))
    va, vb = dom.createGlobalVec(2), dom.createGlobalVec(2)
    va.setArray(ua.ravel())
    vb.setArray(ub.ravel())
    vol, Svol = (a[0] for a in im.moments(mesh, np.zeros(mesh.n_node), im.GAUSS))
    first = dom.volume()
    assert abs(first - vol) <= BAR * Svol and _rel(vol, 0.8) <= 1e-13
    kept = dom._volumeVec
    assert dom.volume() == first and dom._volumeVec is kept        # the second call reuses the vector of the first
    for rule, code in (("gauss", im.GAUSS), ("nodal", im.NODAL)):
        ref, S = im.moments(mesh, ua, code, True, ub)
        r = im.named(ref, 2, 2, True)
        m = dom.integrate(va, minus=vb, rule=rule, grad=True)
        flat = np.concatenate([[m.volume], m.value, m.square, m.grad2, [m.div2], m.curl2])
        assert np.all(np.abs(flat - ref) <= BAR * S)
        assert _rel(dom.normL2(va, minus=vb, rule=rule), math.sqrt(r["square"].sum())) <= 1e-12
        assert _rel(dom.seminormH1(va, minus=vb, rule=rule), math.sqrt(r["grad2"].sum())) <= 1e-12
    plain = dom.integrate(va)
    assert plain.grad2 is None and plain.div2 is None and plain.curl2 is None and plain.value.shape == (2,)
    scalar = dom.createGlobalVec(1)
    scalar.set(2.0)
    sg = dom.integrate(scalar, grad=True)
    assert sg.div2 is None and sg.curl2 is None and sg.grad2.shape == (1,)
    with pytest.raises(ValueError, match="rule"):
        dom.integrate(va, rule="simpson")


def _uniform(nelem):
    from tests.test_gpu_api import setFemProblem
    return setFemProblem('uniform', nelem=nelem, ngl=3)


def test_kle_error_norms(lib):
    found = {}
    for n in (4, 8):
        fem = _uniform([n, n])
        solve, seen = fem.solveKLE, []

        def recording(t, vort):                                      # what every norm must be, taken right after each solve
            solve(t, vort)
            ev, _ = fem.generateExactVecs(t)
            seen.append({"l2": (ev - fem.vel).norm(norm_type=2),     # the expression getKLEError had before it took a norm
                         "L2": fem.dom.normL2(ev, minus=fem.vel), "H1": fem.dom.seminormH1(ev, minus=fem.vel),
                         "lumped": fem.dom.normL2(ev, minus=fem.vel, rule="nodal")})

        fem.solveKLE = recording
        default = fem.getKLEError(viscousTimes=[0.3, 0.5])
        assert default == [s["l2"] for s in seen] and len(default) == 2
        assert fem.getKLEError(viscousTimes=[0.3, 0.5], norm="l2") == [s["l2"] for s in seen[2:]]
        del seen[:]
        L2 = fem.getKLEError(viscousTimes=[0.3], norm="L2")
        H1 = fem.getKLEError(viscousTimes=[0.3], norm="H1")
        lumped = fem.getKLEError(viscousTimes=[0.3], norm="lumped")
        assert (L2, H1, lumped) == ([seen[0]["L2"]], [seen[1]["H1"]], [seen[2]["lumped"]])
        default = [seen[2]["l2"]]
        assert L2[0] < 1e-12 and lumped[0] < 1e-12                   # the reference's velocity bar (src/tests/test_solver.py:20-27)
        # the lumped norm is the algebraic one with every node weighted: sum w e^2 <= max w sum e^2, and max w shrinks like h^dim
        assert lumped[0] <= math.sqrt(fem.operator.weights.max()) * default[0] * (1.0 + 1e-9) + 1e-300
        # a nodal difference of the same size everywhere, 2^-10 in every DOF: the algebraic norm counts the nodes, the integral does not
        a, b = fem.dom.createGlobalVec(fem.dim), fem.dom.createGlobalVec(fem.dim)
        a.set(1.0)
        b.set(1.0 - 2.0 ** -10)
        n_dof = fem.dom.ctx.n_owned * fem.dim
        fixed = ((a - b).norm(norm_type=2), fem.dom.normL2(a, minus=b), fem.dom.volume())
        assert _rel(fixed[0], 2.0 ** -10 * math.sqrt(n_dof)) <= 1e-13
        assert _rel(fixed[1], 2.0 ** -10 * math.sqrt(fem.dim * fixed[2])) <= 1e-13
        found[n] = (default[0], L2[0], lumped[0], math.sqrt(fem.operator.weights.max()), fixed[0], fixed[1], n_dof)
        with pytest.raises(ValueError, match="norm"):
            fem.getKLEError(viscousTimes=[0.3], norm="max")
    print("n: (l2, L2, lumped, sqrt(max weight), l2 of the fixed difference, L2 of it, DOFs)", found)
    assert found[8][3] < 0.6 * found[4][3]
    assert found[8][0] > found[4][0]                                 # the default grows with the mesh (1.2e-14 -> 9.2e-14 measured) ...
    assert found[8][1] < 1e-12 and found[4][1] < 1e-12               # ... where the integral norm stays under the bar
    # and where it can be proved, not only observed: the same pointwise difference on both meshes
    assert _rel(found[8][4] / found[4][4], math.sqrt(found[8][6] / found[4][6])) <= 1e-13 and found[8][4] > 1.8 * found[4][4]
    assert _rel(found[8][5], found[4][5]) <= 1e-13


def test_nodal_rule_is_the_lumped_weights(lib):
    for kw in (dict(nelem=[5, 4], ngl=3), dict(nelem=[2, 3], ngl=6), dict(lower=[0, 0, 0], upper=[1, 1, 1], nelem=[3, 2, 2], ngl=3)):
        from tests.test_gpu_api import setFemProblem
        fem = setFemProblem('uniform', **kw)
        w = np.asarray(fem.operator.weights)
        u = np.random.default_rng(6).uniform(-1.0, 1.0, (w.size, fem.dim))
        vec = fem.dom.createGlobalVec(fem.dim)
        vec.setArray(u.ravel())
        m = fem.dom.integrate(vec, rule="nodal")
        S = np.abs(u).T @ w
        assert np.all(np.abs(m.value - u.T @ w) <= BAR * S)
        assert abs(m.volume - w.sum()) <= BAR * w.sum()


def _taylor_green(config=None, **kw):
    from pynama_amd.cases.custom_func import CustomFuncCase
    with open(os.path.join(CASES_DIR, "taylor-green.yaml")) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    cfg.update(config or {})
    fem = CustomFuncCase(cfg, case="taylor-green", nelem=[8, 8], ngl=5, maxSteps=3, endTime=1.0, **kw)
    fem.setUp()
    fem.setUpSolver()
    fem.setUpTimeSolver()
    fem.ts.setAdaptType("none")
    fem.ts.setTimeStep(0.01)
    return fem


def test_diagnostics_block_records_every_step(lib):
    fem = _taylor_green({"diagnostics": {"every": 1}})
    mesh = _dom_mesh(fem.dom, 5)
    taken = []

    def hook(ts):
        fem.convergedStepFunction(ts)
        ev, ew = fem.generateExactVecs(ts.getTime())
        taken.append((ts.getTime(), fem.vel.getArray().copy(), fem.vort.getArray().copy(), ev.getArray().copy(), ew.getArray().copy()))

    fem.ts.setPostStep(hook)
    fem.startSolver()
    series = fem.getDiagnosticsSeries()
    assert len(series) == len(taken) == 3
    for rec, (t, vel, vort, ev, ew) in zip(series, taken):
        assert rec["t"] == t
        mv, Sv = (im.named(a, 2, 2, True) for a in im.moments(mesh, vel.reshape(-1, 2), im.GAUSS, True))
        mw, Sw = (im.named(a, 2, 1, False) for a in im.moments(mesh, vort.reshape(-1, 1), im.GAUSS, False))
        me, Se = (im.named(a, 2, 2, False) for a in im.moments(mesh, vel.reshape(-1, 2), im.GAUSS, False, ev.reshape(-1, 2)))
        mo, So = (im.named(a, 2, 1, False) for a in im.moments(mesh, vort.reshape(-1, 1), im.GAUSS, False, ew.reshape(-1, 1)))
        assert abs(rec["kinetic_energy"] - 0.5 * fem.rho * mv["square"].sum()) <= 0.5 * fem.rho * BAR * Sv["square"].sum()
        assert abs(rec["enstrophy"] - 0.5 * mw["square"].sum()) <= 0.5 * BAR * Sw["square"].sum()
        assert np.all(np.abs(rec["circulation"] - mw["value"]) <= BAR * Sw["value"])
        # the square roots: compared as squares, with four roundings of the result for the root and its square.  div u and curl u
        # of this smooth solenoidal field are sums of gradient components that cancel (|div u| ~ 1e-3 |grad u|), each rounded
        # relative to itself: their scale is taken from the absolute gradient components (im.component_scale); |contribution|
        # alone gave a ratio of 1.95 for div_l2 on an MI355X, the model's own rounding included
        Sdiv, Scurl = im.component_scale(mesh, vel.reshape(-1, 2))
        for key, ref, S in (("div_l2", mv["div2"], Sdiv), ("curl_l2", mv["curl2"].sum(), Scurl.sum()),
                            ("vel_error_l2", me["square"].sum(), Se["square"].sum()), ("vort_error_l2", mo["square"].sum(), So["square"].sum())):
            print(f"{key}: |dev^2 - model| / (2e-13 S) = {abs(rec[key] ** 2 - ref) / (BAR * S):.2e}")
            assert abs(rec[key] ** 2 - ref) <= BAR * S + 4.0 * np.finfo(float).eps * ref, key
    ke = [rec["kinetic_energy"] for rec in series]
    assert ke[0] > 0.0 and ke[0] >= ke[1] >= ke[2]


def test_no_diagnostics_block_makes_no_call(lib):
    from pynama_amd.domain import integrals
    fem = _taylor_green()
    before = integrals.calls
    fem.startSolver()
    assert fem.getDiagnosticsSeries() == [] and integrals.calls == before
    assert fem.dom.ctx.timers()["integrate_ms"] == 0.0
    fem2 = _taylor_green({"diagnostics": {"every": 2, "rule": "nodal"}})
    fem2.startSolver()
    assert len(fem2.getDiagnosticsSeries()) == 1 and fem2.dom.ctx.timers()["integrate_ms"] > 0.0


def test_cavity_diagnostics_have_no_error_entries(lib):
    """a no-slip case has no exact fields: the record carries the six integral entries and neither error"""
    from pynama_amd.cases.cavity import Cavity
    with open(os.path.join(CASES_DIR, "cavity.yaml")) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    cfg["diagnostics"] = {"every": 1}
    fem = Cavity(cfg, case="cavity", nelem=[6, 6], ngl=3, maxSteps=3, endTime=1.0)
    fem.setUp()
    fem.setUpSolver()
    fem.setUpTimeSolver()
    fem.ts.setAdaptType("none")
    fem.ts.setTimeStep(0.001)
    mesh = _dom_mesh(fem.dom, 3)
    taken = []

    def hook(ts):
        fem.convergedStepFunction(ts)
        taken.append((ts.getTime(), fem.vel.getArray().copy(), fem.vort.getArray().copy()))

    fem.ts.setPostStep(hook)
    fem.startSolver()
    series = fem.getDiagnosticsSeries()
    assert len(series) == len(taken) == 3
    for rec, (t, vel, vort) in zip(series, taken):
        assert set(rec) == {"t", "kinetic_energy", "enstrophy", "circulation", "div_l2", "curl_l2"} and rec["t"] == t
        mv, Sv = (im.named(a, 2, 2, True) for a in im.moments(mesh, vel.reshape(-1, 2), im.GAUSS, True))
        mw, Sw = (im.named(a, 2, 1, False) for a in im.moments(mesh, vort.reshape(-1, 1), im.GAUSS, False))
        assert rec["kinetic_energy"] > 0.0
        assert abs(rec["kinetic_energy"] - 0.5 * fem.rho * mv["square"].sum()) <= 0.5 * fem.rho * BAR * Sv["square"].sum()
        assert abs(rec["enstrophy"] - 0.5 * mw["square"].sum()) <= 0.5 * BAR * Sw["square"].sum()
        Sdiv, Scurl = im.component_scale(mesh, vel.reshape(-1, 2))
        for key, ref, S in (("div_l2", mv["div2"], Sdiv), ("curl_l2", mv["curl2"].sum(), Scurl.sum())):
            print(f"cavity {key}: |dev^2 - model| / (2e-13 S) = {abs(rec[key] ** 2 - ref) / (BAR * S):.2e}, against |contribution| "
                  f"{abs(rec[key] ** 2 - ref) / (BAR * Sv['div2' if key == 'div_l2' else 'curl2'].sum()):.2e}")
            assert abs(rec[key] ** 2 - ref) <= BAR * S + 4.0 * np.finfo(float).eps * ref, key
