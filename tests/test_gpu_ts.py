"""TsSolver on the device: the two RK vector passes against numpy, observed orders, the adaptive controller against a numpy
model of the same step sequence, the Taylor-Green vortex end to end through the case classes, parity with a restatement over
oracle/, uniform flow, the post-step callback with HDF5 output, and two ranks sharing one GPU."""
import os
import subprocess
import sys
import tempfile
from fractions import Fraction as Fr

import numpy as np
import pytest
import yaml

import pynama_amd
from pynama_amd.common.options import Options
from pynama_amd.solver.ts_solver import TABLEAUX, TsSolver
from pynama_amd.vectors import Vec

pytestmark = pytest.mark.gpu
pynama_amd.install_reference_layout()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(os.path.dirname(pynama_amd.__file__), "cases")


@pytest.fixture(autouse=True)
def clean_options():
    saved = Options._db
    Options(argv=[])
    yield
    Options._db = saved


def _ctx(nelem):
    from pynama_amd.domain.dmplex import DMPlexDom
    dom = DMPlexDom(boxMesh={"nelem": nelem, "lower": [0.0] * len(nelem), "upper": [1.0] * len(nelem)})
    dom.setFemIndexing(2)
    return dom, dom.ctx


# ---- 1. kernels against numpy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nelem", [[4, 2], [5, 3, 2]])       # 15 and 72 nodes: odd and even lengths for every bs
@pytest.mark.parametrize("bs", [1, 2, 3, 6])
def test_maxpy_and_finish_against_numpy(nelem, bs):
    dom, ctx = _ctx(nelem)
    n = ctx.n_owned * bs
    rng = np.random.default_rng(bs * 100 + len(nelem))
    x = Vec(ctx, bs)
    K = [Vec(ctx, bs) for _ in range(8)]
    ka = [rng.standard_normal(n) for _ in range(8)]
    for v, a in zip(K, ka):
        v.setArray(a)
    xa = rng.standard_normal(n)
    y = Vec(ctx, bs)
    for m in range(9):
        w = rng.standard_normal(m)
        x.setArray(xa)
        ctx.vec_maxpy(y.id, x.id, [v.id for v in K[:m]], w)
        ref = xa.copy()
        for j in range(m):
            ref = ref + w[j] * ka[j]
        assert np.abs(y.getArray() - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
        ctx.vec_maxpy(x.id, x.id, [v.id for v in K[:m]], w)               # y aliasing x
        assert np.abs(x.getArray() - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
        # finish, with and without the error estimate, and the roll-back
        hb, hd = 0.1 * rng.standard_normal(m), 0.01 * rng.standard_normal(m)
        atol, rtol = 1e-3, 1e-2
        x.setArray(xa)
        assert ctx.ts_step_finish(x.id, [v.id for v in K[:m]], hb) is None
        xn = xa.copy()
        d = np.zeros(n)
        for j in range(m):
            xn = xn + hb[j] * ka[j]
            d = d + hd[j] * ka[j]
        assert np.abs(x.getArray() - xn).max() <= 1e-14 * np.abs(xn).max()
        x.setArray(xa)
        wn = ctx.ts_step_finish(x.id, [v.id for v in K[:m]], hb, hd, atol, rtol)
        xg = x.getArray()
        assert np.abs(xg - xn).max() <= 1e-14 * np.abs(xn).max()
        ref_wn = np.sqrt(np.mean((np.abs(d) / (atol + rtol * np.maximum(np.abs(xn), np.abs(xn + d)))) ** 2))
        assert abs(wn - ref_wn) <= 1e-13 * max(ref_wn, 1e-300) or (m == 0 and wn == 0.0)
        ctx.vec_maxpy(x.id, x.id, [v.id for v in K[:m]], -hb)             # roll back
        assert np.abs(x.getArray() - xa).max() <= 1e-14 * max(1.0, np.abs(xa).max())


def test_argument_checks():
    dom, ctx = _ctx([4, 2])
    x, k, k3 = Vec(ctx, 1), Vec(ctx, 1), Vec(ctx, 3)
    with pytest.raises(pynama_amd._lib.PynamaHipError):
        ctx.vec_maxpy(x.id, x.id, [k3.id], [1.0])                            # block sizes differ
    with pytest.raises(pynama_amd._lib.PynamaHipError):
        ctx.vec_maxpy(x.id, x.id, [k.id] * 9, [1.0] * 9)                     # more than 8 stage vectors
    with pytest.raises(pynama_amd._lib.PynamaHipError):
        ctx.ts_step_finish(x.id, [k.id, x.id], [1.0, 1.0])                  # x among the stages
    with pytest.raises(pynama_amd._lib.PynamaHipError):
        ctx.vec_maxpy(x.id, x.id, [12345], [1.0])                            # invalid handle


# ---- the linear test problem y' = lam .* y ---------------------------------------------------------------------------------
def _linear_problem(ctx, bs, stiff=None, seed=3):
    n = ctx.n_owned * bs
    rng = np.random.default_rng(seed)
    lam = rng.uniform(-2.0, -0.5, n)
    if stiff is not None:
        lam[n // 3] = stiff
    y0 = rng.uniform(0.5, 1.5, n)
    lv, u = Vec(ctx, bs), Vec(ctx, bs)
    lv.setArray(lam)
    u.setArray(y0)
    return lam, y0, lv, u


def _rhs(ts, t, X, F, lv):
    F.pointwiseMult(lv, X)


def _fma(w, k, r):
    """w * k + r rounded once per entry, as the kernels' fma (exact in rationals, then correctly rounded)"""
    w = Fr(float(w))
    return np.array([float(w * Fr(float(a)) + Fr(float(b))) for a, b in zip(k, r)])


def np_rk_model(lam, y0, rk_type, dt, T, rtol, atol, adapt, max_steps=10 ** 6):
    """numpy restatement of the spec on y' = lam .* y: stages, FSAL, in-place finish, weighted RMS norm, TSADAPTBASIC, roll-back,
    MATCHSTEP.  The vector passes round as the kernels do (one fma per term, terms in index order, zero weights skipped): the
    error estimate is a difference of nearly equal stage sums, so anything else moves the step sizes at 1e-10."""
    tab = TABLEAUX[rk_type]
    x = y0.copy()
    K = [np.zeros_like(x) for _ in range(tab.s)]
    t, h, hs, rejects, have_k0 = 0.0, dt, [], 0, False
    while len(hs) < max_steps and t < T:
        rejected = 0
        while True:
            hh, last = (T - t, True) if t + h >= T else (h, False)
            for i in range(tab.s):
                if i == 0 and have_k0:
                    continue
                Y = x.copy()
                for j in range(i):
                    if tab.a_f[i][j] != 0.0:
                        Y = _fma(hh * tab.a_f[i][j], K[j], Y)
                K[i] = lam * Y
            have_k0 = tab.fsal
            js = [j for j in range(tab.s) if tab.b_f[j] != 0.0 or (adapt and tab.d_f[j] != 0.0)]
            xn, dd = x.copy(), np.zeros_like(x)
            for j in js:
                xn = _fma(hh * tab.b_f[j], K[j], xn)
                if adapt:
                    dd = _fma(hh * tab.d_f[j], K[j], dd)
            if not adapt:
                x, h_next = xn, h
                break
            e = np.sqrt(np.mean((np.abs(dd) / (atol + rtol * np.maximum(np.abs(xn), np.abs(xn + dd)))) ** 2))
            accept = e <= 1.0
            safety = 0.9 * (0.5 if (not accept and rejected) else 1.0)
            fac = 10.0 if e == 0.0 else min(max(safety * e ** (-1.0 / tab.order), 0.1), 10.0)
            h_next = hh * fac
            if accept:
                x = xn
                break
            for j in js:                                          # roll back: the same pass with -h b
                if tab.b_f[j] != 0.0:
                    xn = _fma(-(hh * tab.b_f[j]), K[j], xn)
            x = xn
            rejects += 1
            rejected += 1
            h = h_next
        t = T if last else t + hh
        hs.append(hh)
        h = h_next
        if tab.fsal:
            K[0], K[-1] = K[-1], K[0]
    return x, hs, rejects


# ---- 2. observed order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rk_type,order", [("5bs", 5), ("3bs", 3), ("4", 4)])
def test_observed_order(rk_type, order):
    dom, ctx = _ctx([7, 5])
    errs = []
    for h in (0.1, 0.05, 0.025):       # 5bs is at 5e-13 at 0.025 (round-off follows); at 0.2 it is not yet asymptotic (3.7)
        lam, y0, lv, u = _linear_problem(ctx, 3)
        ts = TsSolver()
        ts.setRKType(rk_type)
        ts.setAdaptType("none")
        ts.setTimeStep(h)
        ts.setMaxTime(1.0)
        ts.setRHSFunction(_rhs, args=(lv,))
        ts.solve(u)
        assert ts.getConvergedReason() == 1 and ts.getTime() == 1.0 and ts.getStepRejections() == 0
        errs.append(np.abs(u.getArray() - y0 * np.exp(lam)).max())
    rates = [np.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print(f"{rk_type}: errors {errs}, observed orders {rates}")
    assert all(abs(r - order) <= 0.3 for r in rates), (errs, rates)


# ---- 3. adaptive run against the numpy model ---------------------------------------------------------------------------------
def test_adaptive_matches_model():
    dom, ctx = _ctx([7, 5])
    lam, y0, lv, u = _linear_problem(ctx, 2, stiff=-30.0)
    ts = TsSolver()
    ts.setTimeStep(0.5)
    ts.setMaxTime(1.0)
    ts.setTolerances(rtol=1e-8, atol=1e-8)
    ts.setRHSFunction(_rhs, args=(lv,))
    hs, last_t = [], [0.0]

    def post(t):
        hs.append(t.getTime() - last_t[0])
        last_t[0] = t.getTime()
    ts.setPostStep(post)
    ts.solve(u)
    x_ref, hs_ref, rej_ref = np_rk_model(lam, y0, "5bs", 0.5, 1.0, 1e-8, 1e-8, True)
    assert ts.getConvergedReason() == 1 and ts.getTime() == 1.0
    assert ts.getStepRejections() >= 1 and ts.getStepRejections() == rej_ref
    assert len(hs) == len(hs_ref) == ts.getStepNumber()
    assert np.all(np.abs(np.array(hs) - np.array(hs_ref)) <= 1e-12 * np.array(hs_ref)), (hs, hs_ref)
    assert np.abs(u.getArray() - x_ref).max() <= 1e-12
    assert np.abs(u.getArray() - y0 * np.exp(lam)).max() < 1e-6
    assert ts.rhs_evals == 8 + 7 * (ts.getStepNumber() + ts.getStepRejections() - 1)


# ---- case classes ---------------------------------------------------------------------------------------------------------------
def setFemProblem(case, config=None, **kwargs):
    from cases.custom_func import CustomFuncCase
    from cases.uniform import UniformFlow
    with open(os.path.join(CASES, f'{case}.yaml')) as f:
        yamlData = yaml.load(f, Loader=yaml.Loader)
    yamlData.update(config or {})
    fem = UniformFlow(yamlData, case=case, **kwargs) if case == 'uniform' else CustomFuncCase(yamlData, case=case, **kwargs)
    fem.setUp()
    fem.setUpSolver()
    return fem


def _rel_l2(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# ---- 4. Taylor-Green 2-D end to end ------------------------------------------------------------------------------------------
def test_taylor_green_2d_end_to_end():
    fem = setFemProblem('taylor-green', nelem=[8, 8], ngl=5, endTime=0.5)
    fem.setUpTimeSolver()
    fem.ts.setTimeStep(0.1)
    fem.ts.setTolerances(rtol=1e-6, atol=1e-6)
    fem.startSolver()
    ts = fem.ts
    assert ts.getConvergedReason() == 1 and ts.getTime() == 0.5
    _, exactVort = fem.generateExactVecs(0.5)
    err = _rel_l2(fem.vort.getArray(), exactVort.getArray())
    print(f"taylor-green 8x8 ngl 5: {ts.getStepNumber()} steps, {ts.getStepRejections()} rejected, "
          f"{ts.rhs_evals} RHS evaluations, relative L2 error {err:.3e}")
    assert err < 1e-2


# ---- 5. parity with a restatement over oracle/ ---------------------------------------------------------------------------------
def test_oracle_parity_fixed_steps():
    import scipy.linalg as sla
    from oracle import fem_oracle as fo
    from pynama_amd.cases.custom_func import CustomFuncCase as C
    fem = setFemProblem('taylor-green', nelem=[5, 5], ngl=3, maxSteps=20, endTime=1.0)
    fem.setUpTimeSolver()
    fem.ts.setAdaptType("none")
    fem.ts.setTimeStep(0.025)
    fem.startSolver()
    assert fem.ts.getConvergedReason() == 2 and fem.ts.getStepNumber() == 20

    mesh = fo.box_mesh([5, 5], [0, 0], [1, 1], 3)
    tb = fo.Tables(3, 2)
    mats = fo.assemble_kle_freeslip(mesh, tb)
    ops = fo.assemble_operators(mesh, tb)
    lu = sla.lu_factor(mats["K"].toarray())
    rho, mu = fem.rho, fem.mu
    nu = mu / rho
    bn = mesh.boundary
    xyz = mesh.xyz

    def evalRHS(t, Y, X):
        vel_bc = np.zeros(mesh.n_node * 2)
        vel_bc.reshape(-1, 2)[bn] = [C.taylorGreenVel_2D(p, nu, t) for p in xyz[bn]]
        X[bn] = [C.taylorGreenVort_2D(p, nu, t)[0] for p in xyz[bn]]            # the boundary reset of the state
        vel = sla.lu_solve(lu, mats["Rw"] @ Y + mats["Krhs"] @ vel_bc)
        v = vel.reshape(-1, 2)
        vv = np.stack([v[:, 0] * v[:, 0], v[:, 0] * v[:, 1], v[:, 1] * v[:, 1]], axis=1).ravel()
        stress = 2.0 * mu * (ops["SrT"] @ vel) - rho * vv
        return ops["Curl"] @ ((ops["DivSrT"] @ stress) / rho)

    tab = TABLEAUX["5bs"]
    X = np.array([C.taylorGreenVort_2D(p, nu, 0.0)[0] for p in xyz])
    K = [None] * tab.s
    t, h = 0.0, 0.025
    for step in range(20):
        for i in range(tab.s):
            if i == 0 and step > 0:
                continue
            Y = X.copy()
            for j in range(i):
                if tab.a_f[i][j] != 0.0:
                    Y = Y + h * tab.a_f[i][j] * K[j]
            K[i] = evalRHS(t + tab.c_f[i] * h, Y, X)
        for j in range(tab.s):
            if tab.b_f[j] != 0.0:
                X = X + h * tab.b_f[j] * K[j]
        t += h
        K[0], K[-1] = K[-1], K[0]
    got = fem.vort.getArray()
    exact = np.array([C.taylorGreenVort_2D(p, nu, t)[0] for p in xyz])
    print(f"oracle parity: device vs restatement {np.abs(got - X).max() / np.abs(X).max():.2e}, "
          f"error against the exact field {_rel_l2(X, exact):.3e}")
    assert np.abs(got - X).max() <= 1e-9 * np.abs(X).max()


# ---- 6. uniform flow ------------------------------------------------------------------------------------------------------------
def test_uniform_flow_stays_still():
    # the step grows tenfold per step (the RHS is round-off); from 1e-5 it stays far inside the stability limit of the
    # explicit scheme, past which round-off would grow and be rejected
    fem = setFemProblem('uniform', maxSteps=5, endTime=1.0)
    fem.setUpTimeSolver()
    fem.ts.setTimeStep(1e-5)
    dts = []
    fem.ts.setPostStep(lambda ts: dts.append(ts.getTimeStep()))
    fem.startSolver()
    assert fem.ts.getStepNumber() == 5 and fem.ts.getStepRejections() == 0 and fem.ts.getConvergedReason() == 2
    assert all(b >= a for a, b in zip([1e-5] + dts, dts))
    assert np.abs(fem.vort.getArray()).max() < 1e-8


# ---- 7. post-step callback and output ----------------------------------------------------------------------------------------------
def test_post_step_callback_and_files(tmp_path):
    fem = setFemProblem('taylor-green', config={"save-output": True, "save-dir": str(tmp_path), "save-n-steps": 2},
                        maxSteps=5)
    fem.setUpTimeSolver()
    fem.ts.setTimeStep(0.01)
    steps = []
    inner = fem.convergedStepFunction

    def spy(ts):
        steps.append(ts.getStepNumber())
        inner(ts)
    fem.ts.setPostStep(spy)
    fem.startSolver()
    assert steps == [1, 2, 3, 4, 5] and fem.ts.getStepNumber() == 5
    files = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("vec-data"))
    assert files == ["vec-data-00002.h5", "vec-data-00004.h5"]
    assert (tmp_path / "mesh.h5").exists()


def test_no_files_by_default(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    fem = setFemProblem('taylor-green', maxSteps=2)
    fem.startSolver()                                   # creates the time solver itself
    assert fem.ts.getStepNumber() == 2 and not list(tmp_path.iterdir())


# ---- 8. two ranks on one GPU ------------------------------------------------------------------------------------------------------
def test_two_ranks_adaptive(tmp_path):
    from pynama_amd import _lib
    nelem = [5, 4, 9]
    dom, ctx = _ctx(nelem)
    lam, y0, lv, u = _linear_problem(ctx, 3, stiff=-30.0, seed=8)
    ts = TsSolver()
    ts.setTimeStep(0.5)
    ts.setMaxTime(1.0)
    ts.setTolerances(rtol=1e-8, atol=1e-8)
    ts.setRHSFunction(_rhs, args=(lv,))
    times = []
    ts.setPostStep(lambda t: times.append(t.getTime()))
    ts.solve(u)
    ref = str(tmp_path / "serial.npz")
    np.savez(ref, lam=lam, y0=y0, x=u.getArray(), times=np.array(times), rejects=ts.getStepRejections())
    size, cap = 2, 4 << 20
    with tempfile.NamedTemporaryFile(dir="/dev/shm" if os.path.isdir("/dev/shm") else None, prefix="pynama_shm_") as f:
        f.truncate(_lib.Context.shm_size(size, cap))
        f.flush()
        env = dict(os.environ, PYNAMA_SHM_CAP=str(cap))
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ts_dist_gpu_worker.py"), str(r), str(size), f.name,
                                   ",".join(map(str, nelem)), ref], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                  text=True) for r in range(size)]
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=280)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                pytest.fail("distributed GPU worker timed out")
        print("\n".join(outs))
        assert all(p.returncode == 0 for p in procs), "\n".join(outs)
