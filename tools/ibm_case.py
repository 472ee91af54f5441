#!/usr/bin/env python3
"""Immersed-boundary case through the case classes: a circle in a uniform stream (ibm-static.yaml / ibm-dynamic.yaml with the
resolution given here), fixed steps of rk 3bs.  Prints the markers, the affected lattice nodes and cond(A) (host, from
pyn_ibm_matrix_get); after each step max |H vel - U_B| and the drag / lift coefficients; and the wall time per step split into the
RHS evaluations of the stages, the KLE solve of the post-step, pyn_ibm_set and pyn_ibm_correct (host clock around a device
synchronise each; single run, the first step apart because it carries the factorisation of K and first-launch costs).
usage: ibm_case.py [static|dynamic] [nelem_x] [nelem_y] [steps] [dt]"""
import os
import sys
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pynama_amd  # noqa: E402
from pynama_amd import _lib  # noqa: E402
from pynama_amd.cases.immersed_boundary import ImmersedBoundaryDynamic, ImmersedBoundaryStatic  # noqa: E402
from pynama_amd.common.options import Options  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "static"
nx = int(sys.argv[2]) if len(sys.argv) > 2 else 48
ny = int(sys.argv[3]) if len(sys.argv) > 3 else 32
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
dt = float(sys.argv[5]) if len(sys.argv) > 5 else 1e-3
if kind not in ("static", "dynamic"):
    sys.exit(__doc__)
Options(argv=["-ts_adapt_type", "none", "-ts_dt", str(dt), "-ts_rk_type", "3bs"])

with open(os.path.join(os.path.dirname(pynama_amd.__file__), "cases", f"ibm-{kind}.yaml")) as f:
    cfg = yaml.load(f, Loader=yaml.Loader)
cls = ImmersedBoundaryDynamic if kind == "dynamic" else ImmersedBoundaryStatic
t0 = time.perf_counter()
fem = cls(cfg, case=f"ibm-{kind}", nelem=[nx, ny], maxSteps=steps, endTime=1e9)
fem.setUp()
fem.setUpSolver()
fem.setUpTimeSolver()
ctx = fem.dom.ctx
ctx.sync()
t_setup = time.perf_counter() - t0

info = ctx.ibm_info()
A = ctx.ibm_matrix()
print(f"ibm-{kind}: {nx} x {ny} cells ngl {fem.ngl} ({ctx.n_owned} nodes, h = {fem.h[0]:.5g} x {fem.h[1]:.5g}), "
      f"kernel sources {_lib.source_hash()}, setup {t_setup:.2f} s")
print(f"M = {info['markers']} markers ({fem.body.getKernel()}-point delta, spacing {fem.body.spacing} h), "
      f"{info['affected_nodes']} affected nodes, cond(A) = {np.linalg.cond(A):.4g}, KLE rows {ctx.n_owned * fem.dim}")

acc = {"rhs": 0.0, "kle": 0.0, "set": 0.0, "correct": 0.0}
marks = []


def timed(key, fn):
    def call(*a, **kw):
        ctx.sync()
        s = time.perf_counter()
        out = fn(*a, **kw)
        ctx.sync()
        acc[key] += time.perf_counter() - s
        return out
    return call


ctx.ibm_set = timed("set", ctx.ibm_set)
ctx.ibm_correct = timed("correct", ctx.ibm_correct)
rhs, post, kle = fem.evalRHS, fem.convergedStepFunction, fem.solveKLE
in_rhs = [False]


def timed_rhs(ts_, t, X, F):
    in_rhs[0] = True
    timed("rhs", rhs)(ts_, t, X, F)
    in_rhs[0] = False


def timed_kle(t, vort):
    return kle(t, vort) if in_rhs[0] else timed("kle", kle)(t, vort)      # the KLE solves of the stages belong to the RHS


def timed_post(ts_):
    post(ts_)
    t = ts_.getTime()
    res = np.abs(ctx.ibm_interp(fem.vel.id) - fem.body.getVelocity(t)).max()
    _, _, C = fem.getForces()[-1]
    print(f"step {ts_.getStepNumber():3d} t = {t:.4e}: max|H vel - U_B| = {res:.2e}, C_d = {C[0]:+.5e}, C_l = {C[1]:+.5e}")
    ctx.sync()
    marks.append((time.perf_counter(), dict(acc)))


fem.solveKLE = timed_kle
fem.ts.setRHSFunction(timed_rhs)
fem.ts.setPostStep(timed_post)
ctx.sync()
start = time.perf_counter()
fem.startSolver()
ctx.sync()
n = fem.ts.getStepNumber()
print(f"{n} steps of dt = {dt:g}, {fem.ts.rhs_evals} RHS evaluations, pyn_ibm_set builds {ctx.ibm_info()['builds']}")


def split(wall, a, b, count):
    parts = {k: 1e3 * (b[k] - a[k]) / count for k in acc}
    rest = 1e3 * wall / count - sum(parts.values())
    return (f"{1e3 * wall / count:.3f} ms per step: RHS {parts['rhs']:.3f}, KLE solve {parts['kle']:.3f}, pyn_ibm_set {parts['set']:.3f}, "
            f"pyn_ibm_correct {parts['correct']:.3f}, rest (Curl, RK passes, this tool's residual check) {rest:.3f}")


zero = {k: 0.0 for k in acc}
print("first step: " + split(marks[0][0] - start, zero, marks[0][1], 1))
if n > 1:
    print(f"steps 2..{n}: " + split(marks[-1][0] - marks[0][0], marks[0][1], marks[-1][1], n - 1))
