"""Analytic boundary / initial fields and constant values on node sets, evaluated on the device (pyn_fields.hip): every field
against a numpy restatement of the same formulas, untouched entries and ghosts, pyn_vec_set_nodes bit for bit, the refusals, the
case classes with and without -pynama_device_fields, the constant-value cases, a short time loop, and two ranks sharing the GPU.

Bar of the field comparisons: |device - numpy| <= 32 * 2^-52 * A, A the product of the field's constant factors.  Phases and
constants are the same bits on both sides; each trigonometric factor may differ by the sum of the two libraries' error bounds; there
are at most three such factors and four roundings of products.  Largest ratio measured on an MI355X: 1.43, the sinusoidal diffusive
field on the 3 x 2 meshes, where the device cos(4 pi x) is one ulp from numpy's at two phases."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import yaml

import pynama_amd
from oracle import fem_oracle as fo
from pynama_amd.cases import fields
from pynama_amd.common.options import Options
from tests import fields_model as fm

pytestmark = pytest.mark.gpu
pynama_amd.install_reference_layout()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(os.path.dirname(pynama_amd.__file__), "cases")
FILL = 7.25
NU = 0.02
TIMES = (0.0, 0.37)          # in this order on the same vector: a stale time factor fails


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@pytest.fixture(autouse=True)
def clean_options():
    saved = Options._db
    Options(argv=[])
    yield
    Options._db = saved


MESHES = {
    "2d-3x2-ngl2": dict(nelem=[3, 2], lower=[-0.3, 0.2], upper=[1.7, 0.9], ngl=2),      # phases past 2 pi and negative
    "2d-3x2-ngl5": dict(nelem=[3, 2], lower=[-0.3, 0.2], upper=[1.7, 0.9], ngl=5),
    "2d-16x16-ngl2": dict(nelem=[16, 16], lower=[0.0, 0.0], upper=[1.0, 1.0], ngl=2),   # 289 nodes: a full workgroup and a tail
    "3d-2x2x2-ngl3": dict(nelem=[2, 2, 2], lower=[0.0] * 3, upper=[1.0] * 3, ngl=3),
    "3d-2x2x3-ngl2-jitter": dict(nelem=[2, 2, 3], lower=[0.0] * 3, upper=[1.0] * 3, ngl=2, jitter=0.2),   # no lattice
}


@pytest.fixture(scope="module")
def meshes(lib):
    """name -> (ctx, xyz as the device holds it, boundary nodes), made on first use"""
    made = {}

    def get(name):
        if name not in made:
            mesh = fo.box_mesh(**MESHES[name])
            ctx = lib.Context(0)
            ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
            made[name] = (ctx, ctx.mesh_get(conn=False)[1], np.asarray(mesh.boundary, dtype=np.int64))
        return made[name]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


def _ratio(got, ref, amp):
    return float(np.abs(got - ref).max() / (fm.ULP * amp)) if got.size else 0.0


# ---- 1. every field against the numpy restatement, entries outside the set ---------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_fields_against_numpy(lib, meshes, name):
    ctx, xyz, boundary = meshes(name)
    n, dim = ctx.n_owned, ctx.dim
    assert name != "2d-16x16-ngl2" or n == 289
    sets = {"boundary": boundary, "all": None, "empty": np.zeros(0, np.int64), "last": np.array([n - 1])}
    ids = {k: (-1 if v is None else ctx.nodeset_create(v)) for k, v in sets.items()}
    worst, where = 0.0, "no field"
    for f in (f for f in fields.FIELDS if f.dim == dim):
        vid = ctx.vec_create(f.bs)
        for what, nodes in sets.items():
            ctx.vec_fill(vid, FILL)
            nodes = np.arange(n) if nodes is None else nodes
            for t in TIMES:
                p = f.params(NU, t)
                ctx.field_eval(f.id, p, ids[what], vid)
                got = ctx.vec_get(vid, f.bs).reshape(n, f.bs)
                ref = fm.restate(f.id, p, xyz[nodes])
                r = _ratio(got[nodes], ref, fm.amplitude(f.id, p))
                if r > worst:
                    worst, where = r, f"{f.name} on '{what}' at t = {t}"
                assert r <= 32.0, f"{f.name} on '{what}' at t = {t}: {r:.1f} ulp of the amplitude"
                rest = np.ones(n, bool)
                rest[nodes] = False
                assert np.all(got[rest] == FILL), f"{f.name} on '{what}': an entry outside the set changed"
            if f.bs == 3 and f.name != "taylorGreenVel_3D" and nodes.size:
                assert np.all(got[nodes, 2] == 0.0)
        ctx.vec_destroy(vid)
    print(f"{name}: largest |device - numpy| / (2^-52 A) = {worst:.2f} ({where})")
    for k, i in ids.items():
        if i >= 0:
            ctx.nodeset_destroy(i)


def test_time_factor_matters(lib, meshes):
    """the two times of the test above really give different vectors (so a stale factor cannot pass)"""
    ctx, xyz, _ = meshes("3d-2x2x2-ngl3")
    f = fields.taylorGreenVel_3D
    vid = ctx.vec_create(3)
    out = []
    for t in TIMES:
        ctx.field_eval(f.id, f.params(NU, t), -1, vid)
        out.append(ctx.vec_get(vid, 3))
    assert np.abs(out[0] - out[1]).max() > 1e-3
    ctx.vec_destroy(vid)


# ---- 2. ghosts: a rank's slab, detached ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ghosted(lib):
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    dom = DMPlexDom(boxMesh={'nelem': [2, 2, 4], 'lower': [0.0] * 3, 'upper': [1.0] * 3}, comm=Comm(1, 2))
    dom.setFemIndexing(3)
    ctx = lib.Context(0)
    ctx.comm_init(1, 2, None)
    ctx.halo_set(*dom._halo_plan())
    ctx.mesh_set(3, dom.conn, dom.xyz)
    ctx.csr_symbolic()
    assert ctx.n_ghost > 0 and ctx.n_owned < dom.nNodesGlobal
    yield dom, ctx
    ctx.close()


def test_ghost_entries_never_change(lib, ghosted):
    """fields and constant values over every owned node and over the boundary of a slab whose ghosts hold 7.25: the ghosts are
    read back through a product that is 1 on every ghost column"""
    from tests.test_gpu_vec_algebra import GhostProbe
    dom, ctx = ghosted
    n, ng = ctx.n_owned, ctx.n_ghost
    xyz = ctx.mesh_get(conn=False)[1]
    bc = dom.nodeSet(dom.getNodesFromLabel("External Boundary")).localNodes
    sid = ctx.nodeset_create(bc)
    probe = GhostProbe(ctx, 3)
    vid = ctx.vec_create(3)
    for f in (f for f in fields.FIELDS if f.dim == 3):
        for set_id, nodes in ((sid, bc), (-1, np.arange(n))):
            ctx.vec_set_local(vid, np.full((n + ng) * 3, FILL))
            p = f.params(NU, 0.37)
            ctx.field_eval(f.id, p, set_id, vid)
            got = ctx.vec_get(vid, 3).reshape(n, 3)
            assert _ratio(got[nodes], fm.restate(f.id, p, xyz[nodes]), fm.amplitude(f.id, p)) <= 32.0
            assert np.array_equal(probe.sums(vid), probe.expect(np.full(ng * 3, FILL))), f"{f.name}: a ghost entry changed"
    ctx.vec_set_local(vid, np.full((n + ng) * 3, FILL))
    ctx.vec_set_nodes(vid, -1, [1.0, 2.0, 3.0])
    assert np.array_equal(ctx.vec_get(vid, 3).reshape(n, 3), np.tile([1.0, 2.0, 3.0], (n, 1)))
    assert np.array_equal(probe.sums(vid), probe.expect(np.full(ng * 3, FILL)))
    with pytest.raises(lib.PynamaHipError):
        ctx.nodeset_create([0, n])                      # n is the first ghost: not owned


# ---- 3. vec_set_nodes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d-16x16-ngl2", "3d-2x2x2-ngl3"])
def test_vec_set_nodes_bit_equal(lib, meshes, name):
    ctx, _, boundary = meshes(name)
    n, dim = ctx.n_owned, ctx.dim
    sid, empty = ctx.nodeset_create(boundary), ctx.nodeset_create([])
    values = np.array([0.1, -2.5e-7, 3.0e11][:dim])
    cases = [(sid, boundary, None), (empty, np.zeros(0, np.int64), None), (-1, np.arange(n), None)]
    flags = [0, 1, 0][:dim] if dim == 3 else [0, 1]
    cases += [(sid, boundary, flags), (sid, boundary, [0] * dim)]
    vid = ctx.vec_create(dim)
    for set_id, nodes, dofs in cases:
        ctx.vec_fill(vid, FILL)
        ctx.vec_set_nodes(vid, set_id, values, dofs)
        ref = np.full((n, dim), FILL)
        cols = np.arange(dim) if dofs is None else np.nonzero(dofs)[0]
        ref[np.ix_(nodes, cols)] = values[cols]
        assert np.array_equal(ctx.vec_get(vid, dim).reshape(n, dim), ref), (set_id, dofs)
    # every block size the library has a kernel for
    for bs in range(1, 7):
        v = ctx.vec_create(bs)
        ctx.vec_fill(v, FILL)
        vals = np.arange(1.0, bs + 1)
        ctx.vec_set_nodes(v, sid, vals)
        ref = np.full((n, bs), FILL)
        ref[boundary] = vals
        assert np.array_equal(ctx.vec_get(v, bs).reshape(n, bs), ref)
        ctx.vec_destroy(v)
    ctx.vec_destroy(vid)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    mesh2 = fo.box_mesh([3, 2], [0.0, 0.0], [1.0, 1.0], 2)
    mesh3 = fo.box_mesh([2, 2, 2], [0.0] * 3, [1.0] * 3, 2)
    ctx, other = lib.Context(0), lib.Context(0)
    ctx.mesh_set(2, mesh2.conn, mesh2.xyz)
    other.mesh_set(3, mesh3.conn, mesh3.xyz)
    n = ctx.n_owned
    v1, v2 = ctx.vec_create(1), ctx.vec_create(2)
    ctx.vec_fill(v1, FILL)
    ctx.vec_fill(v2, FILL)
    sid = ctx.nodeset_create(mesh2.boundary)
    foreign = [other.nodeset_create([0, 1]) for _ in range(3)][-1]        # id 2: never handed out by ctx
    dead = ctx.nodeset_create([0, 1, 2])
    ctx.nodeset_destroy(dead)
    vel, vort = fields.taylorGreenVel_2D, fields.taylorGreenVort_2D
    pv, pw = vel.params(NU, 0.1), vort.params(NU, 0.1)
    bad_calls = [
        lambda: ctx.field_eval(lib.FIELD_COUNT, pv, sid, v2),                             # unknown field
        lambda: ctx.field_eval(-1, pv, sid, v2),
        lambda: ctx.field_eval(lib.FIELD_TG3D_VEL, pv, sid, v2),                          # a 3-D field on a 2-D mesh
        lambda: ctx.field_eval(vel.id, pv, sid, v1),                                      # block size 1 for 2 components
        lambda: ctx.field_eval(vort.id, pw, sid, v2),
        lambda: ctx.field_eval(vel.id, pv + [1.0], sid, v2),                              # wrong nparams
        lambda: ctx.field_eval(vort.id, pw[:2], sid, v1),
        lambda: ctx.field_eval(vel.id, pv, dead, v2),                                     # dead set
        lambda: ctx.field_eval(vel.id, pv, foreign, v2),                                  # another context's id
        lambda: ctx.field_eval(vel.id, pv, -2, v2),
        lambda: ctx.field_eval(vel.id, pv, sid, 12345),                                   # invalid vector
        lambda: ctx.vec_set_nodes(v2, dead, [1.0, 2.0]),
        lambda: ctx.vec_set_nodes(v2, foreign, [1.0, 2.0]),
        lambda: ctx.vec_set_nodes(v2, sid, [1.0]),                                        # values do not fit the block size
        lambda: ctx.vec_set_nodes(v2, sid, [1.0, 2.0, 3.0]),
        lambda: ctx.nodeset_destroy(dead),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(lib.PynamaHipError):
            call()
        assert np.all(ctx.vec_get(v1, 1) == FILL) and np.all(ctx.vec_get(v2, 2) == FILL), f"refusal {k} changed a vector"
    for nodes in ([2, 1, 3], [1, 1, 2], [0, 1, n], [-1, 0], [0, 2 ** 31 + 5]):           # unsorted, duplicate, n_owned, negative
        with pytest.raises(lib.PynamaHipError):
            ctx.nodeset_create(nodes)
    ctx.field_eval(vel.id, pv, sid, v2)                                                   # the live set still works
    assert np.any(ctx.vec_get(v2, 2) != FILL)
    ctx.mesh_set(2, mesh2.conn, mesh2.xyz)                                                # a new mesh takes every set with it
    v2 = ctx.vec_create(2)
    with pytest.raises(lib.PynamaHipError):
        ctx.field_eval(vel.id, pv, sid, v2)
    fresh = ctx.nodeset_create(mesh2.boundary)
    assert fresh != sid                                                                   # ids are not handed out again
    ctx.field_eval(vel.id, pv, fresh, v2)
    ctx.close()
    other.close()


# ---- case classes ---------------------------------------------------------------------------------------------------------------
def _case(kind, case=None, **kwargs):
    from cases.cavity import Cavity
    from cases.custom_func import CustomFuncCase
    from cases.uniform import UniformFlow
    with open(os.path.join(CASES, f"{kind}.yaml")) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    cls = {"uniform": UniformFlow, "cavity": Cavity}.get(kind, CustomFuncCase)
    fem = cls(cfg, case=case or kind, **kwargs)
    fem.setUp()
    fem.setUpSolver()
    return fem


def _on(values, fem, fill):
    """`values` on the boundary nodes, `fill` elsewhere"""
    out = np.full(values.shape, fill)
    bc = np.asarray(sorted(fem.bcNodes), dtype=np.int64)
    out[bc] = values[bc]
    return out


def _host_field(fem, function, nodes, t, bs, fill):
    """direct host evaluation: the static method of custom_func.py at the domain's coordinates"""
    out = np.full((fem.dom.nOwned, bs), fill)
    nodes = np.asarray(sorted(nodes), dtype=np.int64)
    out[nodes] = [function(c, fem.nu, t=t) for c in fem.dom.getNodesCoordinates(nodes)]
    return out


# ---- 5. facade: CustomFuncCase with and without the option ------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(nelem=[4, 4], ngl=5), dict(nelem=[2, 2, 2], ngl=3, lower=[0.0] * 3, upper=[1.0] * 3)],
                         ids=["2d-4x4-ngl5", "3d-2x2x2-ngl3"])
def test_custom_func_case_with_and_without_the_option(lib, kw, monkeypatch):
    from pynama_amd.cases.custom_func import CustomFuncCase as C
    fem = _case("taylor-green", **kw)
    dim, dw, n = fem.dim, fem.dim_w, fem.dom.nOwned
    velF, vortF = (C.taylorGreenVel_2D, C.taylorGreenVort_2D) if dim == 2 else (C.taylorGreenVel_3D, C.taylorGreenVort_3D)
    calls = []
    real = fem.dom.ctx.field_eval
    monkeypatch.setattr(fem.dom.ctx, "field_eval", lambda *a: (calls.append(a[0]), real(*a))[1])

    def run():
        fem.vort.set(FILL)
        fem.applyBoundaryConditions(0.2)
        bc = fem.vel.getArray().reshape(n, dim), fem.vort.getArray().reshape(n, dw)
        fem.computeInitialCondition(0.0)
        return bc + (fem.vort.getArray().reshape(n, dw),)

    host = run()
    assert not calls, "pyn_field_eval was called without -pynama_device_fields"
    allNodes = range(n)
    assert np.array_equal(host[0], _host_field(fem, velF, fem.bcNodes, 0.2, dim, 0.0))        # bit-equal to the host functions
    assert np.array_equal(host[1], _host_field(fem, vortF, fem.bcNodes, 0.2, dw, FILL))
    assert np.array_equal(host[2], _host_field(fem, vortF, allNodes, 0.0, dw, FILL))
    Options().setValue("pynama_device_fields", "1")
    scatter = []
    real_scatter = fem.dom.ctx.vec_scatter
    monkeypatch.setattr(fem.dom.ctx, "vec_scatter", lambda *a, **k: (scatter.append(a), real_scatter(*a, **k))[1])
    dev = run()
    exact = fem.generateExactVecs(0.2)
    assert len(calls) == 5 and not scatter, "with the option every field goes through pyn_field_eval, none through the host scatter"
    amps = (fm.amplitude(fem.velFunction.id, fem.velFunction.params(fem.nu, 0.2)),
            fm.amplitude(fem.vortFunction.id, fem.vortFunction.params(fem.nu, 0.2)),
            fm.amplitude(fem.vortFunction.id, fem.vortFunction.params(fem.nu, 0.0)))
    for what, h, d, a in zip(("vel bc", "vort bc", "vort ic"), host, dev, amps):
        r = _ratio(d, h, a)
        print(f"{what}: device against host {r:.2f} ulp of the amplitude")
        assert r <= 32.0, what
    assert _ratio(exact[0].getArray().reshape(n, dim), _host_field(fem, velF, allNodes, 0.2, dim, 0.0), amps[0]) <= 32.0
    # a plain callable keeps the host path, bit for bit, with the option on
    before = len(calls)
    v = fem.vel.duplicate()
    v.set(FILL)
    plain = lambda c: velF(c, fem.nu, t=0.2)      # noqa: E731
    fem.dom.applyFunctionVecToVec(fem.bcNodeSet, plain, v, dim)
    assert np.array_equal(v.getArray().reshape(n, dim), _host_field(fem, velF, fem.bcNodes, 0.2, dim, FILL))
    v.set(FILL)
    fem.dom.applyFunctionVecToVec(fem.bcNodes, plain, v, dim)                                 # ... and a plain set of nodes
    assert np.array_equal(v.getArray().reshape(n, dim), _host_field(fem, velF, fem.bcNodes, 0.2, dim, FILL))
    assert len(calls) == before and len(scatter) == 2
    # a bound field over a plain set of nodes: the device path through a one-off set that is released again
    made, gone = [], []
    real_create, real_destroy = fem.dom.ctx.nodeset_create, fem.dom.ctx.nodeset_destroy
    monkeypatch.setattr(fem.dom.ctx, "nodeset_create", lambda nodes: (made.append(real_create(nodes)), made[-1])[1])
    monkeypatch.setattr(fem.dom.ctx, "nodeset_destroy", lambda i: (gone.append(i), real_destroy(i))[1])
    w = fem.vel.duplicate()
    for nodes in (fem.bcNodeSet, fem.bcNodes):
        w.set(FILL)
        fem.dom.applyFunctionVecToVec(nodes, fem.velFunction.bind(fem.nu, 0.2), w, dim)
        assert np.array_equal(w.getArray().reshape(n, dim), _on(dev[0], fem, FILL))
    assert len(made) == 1 and gone == made and len(calls) == before + 2
    with pytest.raises(lib.PynamaHipError):
        real(fem.velFunction.id, fem.velFunction.params(fem.nu, 0.2), made[0], w.id)          # the one-off set is dead


def test_operator_study_fields_on_the_device(lib):
    """generateExactOperVecs of the sinusoidal case: four fields, device against host"""
    fem = _case("taylor-green", case="senoidal", nelem=[3, 3], ngl=3)
    assert fem.velFunction is fields.senoidalVel_2D and fem.diffusiveFunction is fields.senoidalDiffusive
    host = [v.getArray() for v in fem.generateExactOperVecs(0.3)]
    Options().setValue("pynama_device_fields", "1")
    dev = [v.getArray() for v in fem.generateExactOperVecs(0.3)]
    for f, h, d in zip((fem.velFunction, fem.vortFunction, fem.convectiveFunction, fem.diffusiveFunction), host, dev):
        assert _ratio(d, h, fm.amplitude(f.id, f.params(fem.nu, 0.3))) <= 32.0, f.name


# ---- 6. constant-value cases -------------------------------------------------------------------------------------------------------
def test_uniform_flow_bit_equal_and_sets_reused(lib, monkeypatch):
    fem = _case("uniform", nelem=[2, 2, 2], ngl=3, lower=[0.0] * 3, upper=[1.0] * 3)
    n = fem.dom.nOwned
    scatter = []
    monkeypatch.setattr(fem.dom.ctx, "vec_scatter", lambda *a, **k: scatter.append(a))
    bcSet, allSet, ids = fem.bcNodeSet, fem.allNodeSet, None
    for _ in range(2):
        fem.vel.set(FILL)
        fem.applyBoundaryConditions(0.0)
        ref = np.zeros((n, 3))
        ref[sorted(fem.bcNodes)] = [1.0, 0.0, 0.0]
        assert np.array_equal(fem.vel.getArray().reshape(n, 3), ref)
        assert fem.bcNodeSet is bcSet and fem.allNodeSet is allSet and ids in (None, bcSet.id)     # nothing rebuilt
        ids = bcSet.id
    vel, vort = fem.generateExactVecs()
    assert np.array_equal(vel.getArray().reshape(n, 3), np.tile([1.0, 0.0, 0.0], (n, 1))) and not vort.getArray().any()
    assert not scatter, "the constant values went through the host scatter"
    assert set(bcSet.globalNodes.tolist()) == set(fem.bcNodes)                                  # bcNodes is still the set of ids


def test_cavity_walls_bit_equal_and_sets_reused(lib, monkeypatch):
    fem = _case("cavity", nelem=[3, 3], ngl=3)
    n = fem.dom.nOwned
    scatter = []
    monkeypatch.setattr(fem.dom.ctx, "vec_scatter", lambda *a, **k: scatter.append(a))
    sets = dict(fem.wallNodeSets)
    assert sorted(sets) == ["down", "left", "right", "up"]
    ids = None
    for _ in range(2):
        fem.vel.set(FILL)
        fem.applyBoundaryConditions()
        ref = np.zeros((n, 2))
        ref[fem.dom.getBorderNodes("up"), 0] = 1.0                                              # the lid: cavity.yaml
        assert np.array_equal(fem.vel.getArray().reshape(n, 2), ref)
        fem.velFS.set(FILL)
        fem.applyBoundaryConditionsFS()
        ref = np.full((n, 2), FILL)
        ref[fem.dom.getBorderNodes("up"), 0] = 1.0
        for wall, dof in (("left", 1), ("right", 1), ("down", 0)):                              # tangential DOFs at rest, in this order
            ref[fem.dom.getBorderNodes(wall), dof] = 0.0
        assert np.array_equal(fem.velFS.getArray().reshape(n, 2), ref)
        now = {w: s.id for w, s in fem.wallNodeSets.items()}
        assert all(fem.wallNodeSets[w] is s for w, s in sets.items()) and (ids is None or ids == now)
        ids = now
    assert not scatter


# ---- 7. time loop --------------------------------------------------------------------------------------------------------------------
def test_time_loop_with_and_without_the_option(lib):
    def run(on):
        Options(["-ts_rk_type", "4", "-ts_adapt_type", "none"] + (["-pynama_device_fields"] if on else []))
        fem = _case("taylor-green", nelem=[4, 4], ngl=5, maxSteps=5, endTime=1.0)
        assert fem.dom.nOwned * fem.dim == 578
        fem.setUpTimeSolver()
        fem.ts.setTimeStep(0.01)
        fem.startSolver()
        assert fem.ts.getStepNumber() == 5 and fem.ts.getStepRejections() == 0
        w = fem.vort.getArray()
        exact = fem.generateExactVecs(fem.ts.getTime())[1].getArray()
        return w, np.linalg.norm(w - exact) / np.linalg.norm(exact)

    w0, e0 = run(False)
    w1, e1 = run(True)
    diff = np.abs(w1 - w0).max() / np.abs(w0).max()
    print(f"time loop: max |w_device - w_host| / max |w| = {diff:.3e}; relative L2 errors {e0:.6e} (host) {e1:.6e} (device), "
          f"relative difference {abs(e1 - e0) / e0:.3e}")
    assert diff <= 1e-9
    assert abs(e1 - e0) <= 1e-6 * e0


# ---- 8. two ranks sharing the GPU --------------------------------------------------------------------------------------------------
def test_two_ranks_fields(lib):
    size, cap, limit = 2, 4 << 20, 120
    with tempfile.NamedTemporaryFile(dir="/dev/shm" if os.path.isdir("/dev/shm") else None, prefix="pynama_shm_") as f:
        f.truncate(lib.Context.shm_size(size, cap))
        f.flush()
        env = dict(os.environ, PYNAMA_SHM_CAP=str(cap))
        # each process under its own time limit; both ranks must be up for the collectives, nothing is started afterwards
        procs = [subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "tests", "fields_dist_gpu_worker.py"),
                                   str(r), str(size), f.name], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                 for r in range(size)]
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=limit + 30)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                pytest.fail("distributed GPU worker timed out")
        print("\n".join(outs))
        assert all(p.returncode == 0 for p in procs), "\n".join(outs)
