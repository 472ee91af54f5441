"""GPU tests of the point probes (pynama_amd/csrc/pyn_probe.hip) against the numpy model of tests/probe_model.py: which points are
found, where (cell and reference position), what is sampled there, exactness on linear functions and tensor polynomials, the transfer
of a field between two orders, determinism, lifetime, the refusals and the facade (DMPlexDom.createProbe, the `probes:` yaml block,
Cavity.centerlines).

Bars.
  location   |x(xi) - p|_inf of the device's own (cell, xi), evaluated in numpy, against max(8 x the model's largest residual on the
             same points, 64 eps x the largest corner coordinate): Newton ends at the rounding level of evaluating the map.
  cells      path 0: the model's lowest accepting cell (= the lower cell on a face) at every point.  Path 1: the same wherever no
             candidate's margin |xi|_inf - 1 lies within 1e-12 of the acceptance threshold 1e-10, where rounding could decide either
             way.  (A window of 1e-9 would hold margin 0, that is every point on a face; the narrower window checks those too.)  The
             points left out are counted and must stay below 2 %; there are none.
  sampling   per component |dev - model| <= (nn + 2 dim ngl + 8) eps sum_a |phi_a| |u_a| with the model at the device's (cell, xi):
             an nn-term sum plus the rounding of the product-form 1-D values.  Two summation orders of the model differ by <= 2.5 eps
             sum |phi| |u| (tests/test_probe_host.py), far inside it, so the constant stands as it is.
  exactness  linear function: 64 eps max|f| at every found point of every mesh; tensor polynomial of degree ngl - 1 per axis, box
             meshes only: the same times ngl^dim.
  transfer   ngl 3 -> ngl 5 -> ngl 3 on the same cells: the sampling bound applied twice (the first one carried through the second)."""
import os

import numpy as np
import pytest
import yaml

from oracle import fem_oracle as fo
from tests import ho_general_meshes as gm
from tests import probe_model as pm
from tests.test_gpu_ho3 import make_ctx

pytestmark = pytest.mark.gpu

EPS = pm.EPS
CASES_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pynama_amd", "cases")


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


def _box(dim, ngl):
    return fo.box_mesh([4, 3] if dim == 2 else [2, 3, 2], [0.0] * dim, gm.UPPER[:dim], ngl)


MESHES = {}
for _n in (2, 3, 5, 12):
    MESHES[f"box2d_ngl{_n}"] = (lambda n=_n: _box(2, n))
for _n in (2, 3, 4, 8):
    MESHES[f"box3d_ngl{_n}"] = (lambda n=_n: _box(3, n))
MESHES.update({
    "bent2d_ngl3": lambda: gm.bent_lattice(2, [4, 3], 3, seed=3),
    "bent2d_ngl5": lambda: gm.bent_lattice(2, [4, 3], 5, seed=3),
    "bent3d_ngl3": lambda: gm.bent_lattice(3, [2, 3, 2], 3, seed=3),
    "bent3d_ngl4": lambda: gm.bent_lattice(3, [2, 3, 2], 4, seed=3),
    "warped2d_ngl3": lambda: gm.warped_lattice(2, [1, 1], 3),
    "warped3d_ngl3": lambda: gm.warped_lattice(3, [2, 1, 2], 3),
    "imported2d_ngl4": lambda: gm.imported(2, [4, 3], 4),
    "imported3d_ngl3": lambda: gm.imported(3, [2, 3, 2], 3),
    "star3_ngl4": lambda: gm.star(3, 4),
    "star5_ngl4": lambda: gm.star(5, 4),
    "star5_ngl3_layers2": lambda: gm.star(5, 3, layers=2),
})
NAMES = sorted(MESHES)
_CPU = {}


def cpu_case(name, reduced):
    """mesh, its points (every mesh node; reduced: 120 of them and the corners, for the checks whose model loops over points in
    Python) and the model's location of them: computed once per module"""
    key = (name, reduced)
    if key not in _CPU:
        mesh = _CPU[(name, not reduced)][0] if (name, not reduced) in _CPU else MESHES[name]()
        extra = pm.bbox_corners(mesh) if name.startswith(("star", "warped")) else None
        P = pm.probe_points(mesh, seed=1, box_boundary=name.startswith("box"), extra_outside=extra, max_nodes=120 if reduced else None)
        _CPU[key] = (mesh, P, pm.locate(mesh, P["pts"]))
    return _CPU[key]


def open_case(lib, name, reduced=False):
    mesh, P, L = cpu_case(name, reduced)
    ctx = make_ctx(lib, mesh, ngl=mesh.ngl)
    return mesh, P, L, ctx, ctx.probe_create(P["pts"])


def set_vec(ctx, u):
    u = np.asarray(u, dtype=np.float64)
    v = ctx.vec_create(1 if u.ndim == 1 else u.shape[1])
    ctx.vec_set(v, u.ravel())
    return v


# ---- found set and location ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_found_set_and_location(lib, name):
    mesh, P, L, ctx, pid = open_case(lib, name)
    dim = mesh.dim
    info, (cell, xi) = ctx.probe_info(pid), ctx.probe_get(pid)
    found = cell >= 0
    assert found[P["inside"]].all(), "a point built as the image of a cell was not found"
    assert (cell[P["outside"]] == -1).all()
    assert info["n"] == len(cell) and info["found"] == found.sum()
    assert info["path"] == (0 if name.startswith("box") else 1)
    assert cell.max() < mesh.n_elem and np.isnan(xi[~found]).all()
    for bs in (1, dim):
        s = ctx.probe_sample(pid, set_vec(ctx, np.ones((mesh.n_node, bs))))
        assert np.isnan(s[~found]).all() and not np.isnan(s[found]).any()
    assert np.abs(xi[found]).max() <= 1.0
    res_dev = np.nanmax(pm.residual(mesh, P["pts"], cell.astype(np.int64), xi))
    res_mod = np.nanmax(pm.residual(mesh, P["pts"], L["cell"], L["xi"]))
    bar = max(8.0 * res_mod, 64.0 * EPS * np.abs(pm.corners(mesh)).max())
    print(f"{name}: path {info['path']}, {info['found']} / {info['n']} found, Newton steps <= {info['max_newton']}, candidates <= "
          f"{info['max_candidates']}; residual {res_dev:.2e} (model {res_mod:.2e}, ratio {res_dev / max(res_mod, 1e-300):.2f}, bar {bar:.2e})")
    assert res_dev <= bar
    assert np.array_equal(found, L["cell"] >= 0)
    keep = np.ones(len(cell), bool) if info["path"] == 0 else ~L["near"]
    print(f"{name}: {np.count_nonzero(~keep)} of {len(cell)} points left out as too near the acceptance threshold")
    assert np.count_nonzero(~keep) < 0.02 * len(cell)
    assert np.array_equal(cell[keep], L["cell"][keep])
    if info["path"] == 1:
        assert 1 <= info["max_newton"] <= pm.NEWTON_CAP and info["max_candidates"] >= 1
    ctx.close()


# ---- sampling against the model at the device's own (cell, xi) -------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_sampling_against_model(lib, name):
    mesh, P, L, ctx, pid = open_case(lib, name, reduced=True)
    dim, ngl = mesh.dim, mesh.ngl
    cell, xi = ctx.probe_get(pid)
    cell = cell.astype(np.int64)
    found = cell >= 0
    const = ngl ** dim + 2 * dim * ngl + 8
    rng = np.random.default_rng(4)
    ph = pm.phi(ngl, dim, xi[found])
    for bs in (1, dim, 3 if dim == 2 else 6):
        u = rng.standard_normal((mesh.n_node, bs))
        dev = ctx.probe_sample(pid, set_vec(ctx, u))
        ref, bound = pm.sample(mesh, cell, xi, u, with_bound=True, ph=ph)
        ratio = (np.abs(dev - ref)[found] / (EPS * bound[found])).max()
        print(f"{name} bs {bs}: |dev - model| <= {ratio:.2f} eps sum|phi||u| (bound {const})")
        assert dev.shape == (len(cell), bs) and np.isnan(dev[~found]).all()
        assert ratio <= const
    ctx.close()


# ---- exactness -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exactness(lib, name):
    mesh, P, L, ctx, pid = open_case(lib, name)
    found = ctx.probe_get(pid)[0] >= 0
    s = ctx.probe_sample(pid, set_vec(ctx, pm.linear_field(mesh)))[:, 0]
    f = pm.linear_field(mesh, P["pts"])
    err = np.abs(s - f)[found].max()
    print(f"{name}: linear function to {err:.2e} (bar {64 * EPS * np.abs(f[found]).max():.2e})")
    assert err <= 64 * EPS * np.abs(f[found]).max()
    if name.startswith("box"):
        s = ctx.probe_sample(pid, set_vec(ctx, pm.tensor_poly(mesh)))[:, 0]
        f = pm.tensor_poly(mesh, P["pts"])
        err, bar = np.abs(s - f)[found].max(), 64 * EPS * mesh.ngl ** mesh.dim * np.abs(f[found]).max()
        print(f"{name}: polynomial of degree {mesh.ngl - 1} to {err:.2e} (bar {bar:.2e})")
        assert err <= bar
    ctx.close()


# ---- order transfer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box", "bent"])
def test_order_transfer(lib, kind):
    build = (lambda n: _box(2, n)) if kind == "box" else (lambda n: gm.bent_lattice(2, [4, 3], n, seed=3))
    m3, m5 = build(3), build(5)
    assert np.array_equal(pm.corners(m3), pm.corners(m5))
    c3, c5 = make_ctx(lib, m3, ngl=3), make_ctx(lib, m5, ngl=5)
    u3 = np.random.default_rng(6).standard_normal((m3.n_node, 2))
    up = c3.probe_create(m5.xyz)                                      # the ngl 3 field at the ngl 5 nodes
    cell_a, xi_a = c3.probe_get(up)
    assert (cell_a >= 0).all()
    u5 = c3.probe_sample(up, set_vec(c3, u3))
    down = c5.probe_create(m3.xyz)                                    # ... set as the ngl 5 field and sampled back at the ngl 3 nodes
    cell_b, xi_b = c5.probe_get(down)
    assert (cell_b >= 0).all()
    back = c5.probe_sample(down, set_vec(c5, u5))
    k3, k5 = 9 + 2 * 2 * 3 + 8, 25 + 2 * 2 * 5 + 8
    b1 = k3 * EPS * pm.sample(m3, cell_a.astype(np.int64), xi_a, u3, with_bound=True)[1]            # at the ngl 5 nodes
    _, s5 = pm.sample(m5, cell_b.astype(np.int64), xi_b, u5, with_bound=True)
    _, carried = pm.sample(m5, cell_b.astype(np.int64), xi_b, b1, with_bound=True)
    bound = k5 * EPS * s5 + carried
    ratio = (np.abs(back - u3) / bound).max()
    print(f"{kind}: ngl 3 -> 5 -> 3 returns the field to {np.abs(back - u3).max():.2e}, {ratio:.3f} of the bound")
    assert ratio <= 1.0
    c3.close()
    c5.close()


# ---- determinism and lifetime ----------------------------------------------------------------------------------------------------
def test_determinism_and_lifetime(lib):
    mesh, P, _ = cpu_case("bent3d_ngl4", True)
    ctx = make_ctx(lib, mesh, ngl=mesh.ngl)
    v = set_vec(ctx, np.random.default_rng(8).standard_normal((mesh.n_node, 3)))
    before = lib.alloc_live()
    a = ctx.probe_create(P["pts"])
    sa = ctx.probe_sample(a, v)
    assert np.array_equal(sa, ctx.probe_sample(a, v), equal_nan=True)                # identical bits
    again = ctx.probe_create(P["pts"])                                               # and the location is deterministic too
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ctx.probe_get(a), ctx.probe_get(again)))
    ctx.probe_destroy(again)
    b = ctx.probe_create(P["pts"][::-1][:50])
    sb = ctx.probe_sample(b, v)
    assert b != a and np.array_equal(sb, sa[::-1][:50], equal_nan=True)
    assert np.array_equal(ctx.probe_sample(a, v), sa, equal_nan=True)                # b did not disturb a
    ctx.probe_destroy(a)
    assert np.array_equal(ctx.probe_sample(b, v), sb, equal_nan=True)                # nor a's end b
    with pytest.raises(lib.PynamaHipError, match="invalid probe handle"):
        ctx.probe_sample(a, v)
    ctx.probe_destroy(b)
    assert lib.alloc_live() == before
    # a new mesh ends every probe set: the old id is an error, not a fault
    c = ctx.probe_create(P["pts"])
    other = fo.box_mesh([2, 2, 2], [0.0] * 3, [1.0] * 3, 3)
    ctx.mesh_set(3, other.conn, other.xyz)
    for call in (lambda: ctx.probe_info(c), lambda: ctx.probe_get(c), lambda: ctx.probe_sample(c, v, 3), lambda: ctx.probe_destroy(c)):
        with pytest.raises(lib.PynamaHipError, match="invalid probe handle.*pyn_mesh_set"):
            call()
    # ... and the vector of the old mesh is refused by a probe set of the new one
    d = ctx.probe_create(np.full((1, 3), 0.5))
    with pytest.raises(lib.PynamaHipError, match="the vector holds .* nodes, the mesh has"):
        ctx.probe_sample(d, v, 3)
    w = set_vec(ctx, np.ones((other.n_node, 3)))
    assert np.array_equal(ctx.probe_sample(d, w), np.ones((1, 3)))
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    pts = np.full((3, 2), 0.25)
    ctx = lib.Context(0)
    ctx.dim = 2                                                       # (the wrapper learns the dimension from mesh_set)
    with pytest.raises(lib.PynamaHipError, match="pyn_mesh_set first"):
        ctx.probe_create(pts)
    # simplices
    tri = fo.simplex_box_mesh([2, 2], [0.0, 0.0], [1.0, 1.0])
    ctx.mesh_set(2, tri.conn, tri.xyz)
    with pytest.raises(lib.PynamaHipError, match="simplices"):
        ctx.probe_create(pts)
    # nn that is not ngl^dim: the mesh itself is refused, and no probe can be made of it
    quad = fo.box_mesh([2, 2], [0.0, 0.0], [1.0, 1.0], 3)
    with pytest.raises(lib.PynamaHipError, match="neither ngl\\^dim"):
        ctx.mesh_set(2, quad.conn[:, :5], quad.xyz)
    ctx.close()
    # n < 1, NaN and infinite coordinates
    ctx = make_ctx(lib, quad, ngl=3)
    with pytest.raises(lib.PynamaHipError, match="no points"):
        ctx.probe_create(np.zeros((0, 2)))
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[1, 1] = bad
        with pytest.raises(lib.PynamaHipError, match="point 1 has a coordinate that is not finite"):
            ctx.probe_create(p)
    # a vector whose node count is not the mesh's
    v = ctx.vec_create(1)
    ctx.mesh_set(2, *(lambda m: (m.conn, m.xyz))(fo.box_mesh([3, 2], [0.0, 0.0], [1.0, 1.0], 3)))
    pid = ctx.probe_create(pts)
    with pytest.raises(lib.PynamaHipError, match="the vector holds 25 nodes, the mesh has 35"):
        ctx.probe_sample(pid, v)
    ctx.close()
    # an order above the limit
    for dim, big in ((2, 13), (3, 9)):
        mesh = fo.box_mesh([1] * dim, [0.0] * dim, [1.0] * dim, big)
        ctx = lib.Context(0)
        ctx.mesh_set(dim, mesh.conn, mesh.xyz)
        with pytest.raises(lib.PynamaHipError, match=f"ngl {big} is above the limit.*ngl <= {big - 1}"):
            ctx.probe_create(np.full((1, dim), 0.5))
        ctx.close()
    # a rank's slab (detached context with a ghost tail)
    dom = DMPlexDom(boxMesh={'nelem': [2, 7], 'lower': [0.0, 0.0], 'upper': [1.0, 1.0]}, comm=Comm(0, 3))
    dom.setFemIndexing(3)
    ctx = lib.Context(0)
    ctx.comm_init(0, 3, None)
    ctx.halo_set(*dom._halo_plan())
    ctx.mesh_set(2, dom.conn, dom.xyz)
    with pytest.raises(lib.PynamaHipError, match="one rank"):
        ctx.probe_create(pts)
    ctx.close()


# ---- facade ----------------------------------------------------------------------------------------------------------------------
def test_create_probe_on_a_domain(lib):
    from pynama_amd.domain.dmplex import DMPlexDom
    dom = DMPlexDom(boxMesh={'nelem': [4, 3], 'lower': [0.0, 0.0], 'upper': [1.0, 0.8]})
    dom.setFemIndexing(3)
    pts = np.array([[0.5, 0.4], [0.1, 0.7], [1.0, 0.8], [1.5, 0.4]])
    probe = dom.createProbe(pts)
    assert len(probe) == 4 and probe.info["path"] == 0
    assert probe.found.tolist() == [True, True, True, False] and probe.cells[3] == -1 and probe.xi.shape == (4, 2)
    vec = dom.createGlobalVec(2)
    xyz = dom.xyz
    vec.setArray(np.column_stack([xyz[:, 0], 2.0 * xyz[:, 1] - xyz[:, 0]]))
    s = probe.sample(vec)
    assert s.shape == (4, 2) and np.isnan(s[3]).all()
    assert np.abs(s[:3] - np.column_stack([pts[:3, 0], 2.0 * pts[:3, 1] - pts[:3, 0]])).max() <= 64 * EPS * 2.0
    probe.destroy()
    with pytest.raises(RuntimeError, match="destroyed"):
        probe.sample(vec)


def _taylor_green(config=None, **kw):
    from pynama_amd.cases.custom_func import CustomFuncCase
    with open(os.path.join(CASES_DIR, "taylor-green.yaml")) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    cfg.update(config or {})
    fem = CustomFuncCase(cfg, case="taylor-green", nelem=[4, 4], ngl=5, maxSteps=3, endTime=1.0, **kw)
    fem.setUp()
    fem.setUpSolver()
    fem.setUpTimeSolver()
    fem.ts.setAdaptType("none")
    fem.ts.setTimeStep(0.01)
    return fem


def test_probes_block_records_every_step(lib):
    block = {"points": [[0.5, 0.5], [0.75, 0.5]], "line": {"from": [0.5, 0.0], "to": [0.5, 1.0], "n": 5}}
    fem = _taylor_green({"probes": block})
    pts = np.array(block["points"] + [[0.5, y] for y in np.linspace(0.0, 1.0, 5)])
    mine = fem.dom.createProbe(pts)
    taken = []

    def hook(ts):
        fem.convergedStepFunction(ts)
        taken.append((ts.getTime(), mine.sample(fem.vel), mine.sample(fem.vort)))

    fem.ts.setPostStep(hook)
    fem.startSolver()
    series = fem.getProbeSeries()
    assert len(series) == len(taken) == 3
    assert np.array_equal(fem.getProbe().points, pts)
    for (t, vel, vort), (t_ref, vel_ref, vort_ref) in zip(series, taken):
        assert t == t_ref and vel.shape == (7, 2) and vort.shape == (7, 1)
        assert np.array_equal(vel, vel_ref) and np.array_equal(vort, vort_ref)
    assert np.abs(series[-1][1]).max() > 0.0


def test_no_probes_block_creates_nothing(lib):
    fem = _taylor_green()
    live = []

    def hook(ts):
        fem.convergedStepFunction(ts)
        live.append(lib.alloc_live())

    fem.ts.setPostStep(hook)
    fem.startSolver()
    assert len(live) == 3 and live[0] == live[1] == live[2]
    before = lib.alloc_live()
    assert fem.getProbe() is None and fem.getProbeSeries() == []
    assert lib.alloc_live() == before and getattr(fem, "_probe", None) is None


def test_cavity_centerlines(lib):
    from pynama_amd.cases.cavity import Cavity
    with open(os.path.join(CASES_DIR, "cavity.yaml")) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    fem = Cavity(cfg, case="cavity", nelem=[6, 6], ngl=3)
    fem.setUp()
    fem.setUpSolver()
    lid = float(cfg["boundary-conditions"]["no-slip"]["up"][0])
    for solve in (False, True):
        fem.applyBoundaryConditions(0.0)
        if solve:
            fem.solveKLE(0.0, fem.vort)
        (y, u), (x, v) = fem.centerlines(9)
        assert y.shape == u.shape == x.shape == v.shape == (9,) and y[0] == 0.0 and y[-1] == 1.0
        nodal = fem.vel.getArray().reshape(-1, 2)
        xyz = fem.dom.xyz
        top = np.nonzero((xyz[:, 0] == 0.5) & (xyz[:, 1] == 1.0))[0]
        bottom = np.nonzero((xyz[:, 0] == 0.5) & (xyz[:, 1] == 0.0))[0]
        assert len(top) == len(bottom) == 1
        assert u[-1] == nodal[top[0], 0] and u[0] == nodal[bottom[0], 0]      # node values: phi is the Kronecker delta there
        if not solve:
            assert u[-1] == lid and u[0] == 0.0
        else:
            assert abs(u[-1] - lid) < 1e-12 and abs(u[0]) < 1e-12 and np.abs(u[1:-1]).max() > 0.0
    assert fem.centerlines(9)[0][1].shape == (9,) and len(fem._centerProbes) == 5
